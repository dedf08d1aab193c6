// Compressed linear algebra on packed uint8 DDC column groups (ops/compress.py CLAPack;
// reference: ColGroupDDC1.rightMultByVector over many groups per row block and
// CompressedMatrixBlock.chainMatrixMultOperations).
//
// Layout: codes is n x Gp uint8 row-major, Gp a multiple of 16, so a row is Gp / 16 16-byte
// vectors.  toff[g] is the first row of group g's tuples in a concatenated table of T rows plus
// the extra row T that every padding column points at (zero in a product table P; a bin table
// has no such row, the padding columns are skipped).  The pack is validated when it is built
// (code < T_g), which is what bounds every LDS index below.
//
//   dictmm   P[t, :]   = D_g[t, :] %*% V[cols_g, :]          one launch for all groups
//   rmm      out[i, :] = u0[i, :] + sum_g P[toff[g] + codes[i, g], :]
//   lmm      bins[toff[g] + codes[i, g], :] += Y[i, :]        fp64 LDS bins, per-block slab
//   dicttmm  out[cols_g[j], :] = sum_t D_g[t, j] * bins[t, :]
//   chain    t(X) %*% f(X %*% v), K = 1, one pass: gather, f, scatter
//   decomp   out[i - r0, d] = D_g[codes[i, g], j] for rows r0 <= i < r1 (a dense row window;
//            reference: ColGroupDDC1.decompressToBlock(target, rl, ru)), lanes along the row
//
// Thread mapping: a row is served by a team of L lanes (L = the power of two >= its vector
// count, at most 64), lane j taking vectors j, j + L, ...: a wave's loads are contiguous 16-byte
// pieces of consecutive rows, and the row sum is an xor butterfly inside the team (the same
// value on every lane, no atomics).  Four rows per team are loaded before any is used, to keep
// enough bytes in flight.  All accumulation is fp64.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int NT = 256;
// the binning kernels (lmm, chain) run 1024 threads: their LDS tables allow one or two workgroups
// per CU, and the one-pass chain was 0.74 ms with 256 threads, 0.56 ms with 1024 (4M x 128 groups)
constexpr int NB = 1024;
constexpr int UNR = 4;
// LDS bytes one workgroup may spend on the staged product table and / or the fp64 bins.  128 KiB
// by the 32 / 64 / 128 KiB sweep in profiles/cla_kbench.txt: a product table of 64 .. 128 KiB
// gathers 2.6x faster from LDS at one or two workgroups per CU than through the cache.
constexpr int kLdsBudget = 128 * 1024;
int g_budget = kLdsBudget;

__device__ __forceinline__ int code_of(const uint4& q, int b) {
  const uint32_t w = (b >> 2) == 0 ? q.x : (b >> 2) == 1 ? q.y : (b >> 2) == 2 ? q.z : q.w;
  return (int)((w >> (8 * (b & 3))) & 0xffu);
}

template <typename T>
__global__ void __launch_bounds__(NT) dictmm_kernel(const T* __restrict__ dv, const int* __restrict__ tup_off,
                                                    const int* __restrict__ tup_nc, const int* __restrict__ tup_c0,
                                                    const int* __restrict__ colidx, const T* __restrict__ V, int K,
                                                    int KP, int Tn, T* __restrict__ P) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)(Tn + 1) * KP) return;
  const int t = (int)(idx / KP), k = (int)(idx % KP);
  double acc = 0.0;
  if (t < Tn && k < K) {
    const int o = tup_off[t], nc = tup_nc[t], c0 = tup_c0[t];
    for (int j = 0; j < nc; ++j) acc += (double)dv[o + j] * (double)V[(int64_t)colidx[c0 + j] * K + k];
  }
  P[idx] = (T)acc;
}

template <typename T>
__global__ void __launch_bounds__(NT) dicttmm_kernel(const T* __restrict__ dv, const int* __restrict__ col_out,
                                                     const int* __restrict__ col_doff, const int* __restrict__ col_nc,
                                                     const int* __restrict__ col_t0, const int* __restrict__ col_T,
                                                     int C, const double* __restrict__ bins, int K, int KP,
                                                     T* __restrict__ out, int ldo) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)C * K) return;
  const int c = (int)(idx / K), k = (int)(idx % K);
  const int o = col_doff[c], nc = col_nc[c], t0 = col_t0[c], nt = col_T[c];
  double acc = 0.0;
  for (int t = 0; t < nt; ++t) acc += (double)dv[o + (int64_t)t * nc] * bins[(int64_t)(t0 + t) * KP + k];
  out[(int64_t)col_out[c] * ldo + k] = (T)acc;
}

// bins[c] = sum_b slab[b, c], in a fixed order: 16 columns (one 128-byte line of a slab row) by
// 16 row slices per block; slice s adds rows s, s + 16, ..., then the slices are added in order.
// (A thread per column walking all rows serially took longer than the binning pass itself.)
__global__ void __launch_bounds__(NT) fold_kernel(const double* __restrict__ slab, double* __restrict__ bins, int nb,
                                                  int64_t width) {
  __shared__ double part[16][17];
  const int cx = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int64_t col = (int64_t)blockIdx.x * 16 + cx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (col < width) {
    int b = slice;
    for (; b + 48 < nb; b += 64) {
      a0 += slab[(int64_t)b * width + col];
      a1 += slab[(int64_t)(b + 16) * width + col];
      a2 += slab[(int64_t)(b + 32) * width + col];
      a3 += slab[(int64_t)(b + 48) * width + col];
    }
    for (; b < nb; b += 16) a0 += slab[(int64_t)b * width + col];
  }
  part[slice][cx] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (slice == 0 && col < width) {
    double r = part[0][cx];
#pragma unroll
    for (int q = 1; q < 16; ++q) r += part[q][cx];
    bins[col] = r;
  }
}

// epilogue of the K = 1 product: the chain's row function
template <typename T>
__device__ __forceinline__ double row_fn(int epi, double u, const T* __restrict__ w, int64_t i) {
  if (epi == 1) return (double)w[i] * u;
  if (epi == 2) return u - (double)w[i];
  return u;
}

template <typename T, int KP, bool LDSP>
__global__ void __launch_bounds__(NT) rmm_kernel(const uint8_t* __restrict__ codes, int64_t n, int Gp, int L,
                                                 const int* __restrict__ toff, const T* __restrict__ P, int Tn,
                                                 const T* __restrict__ u0, int ldu, int K, T* __restrict__ out, int ldo,
                                                 int epi, const T* __restrict__ w, int64_t rpb) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* s_toff = (int*)smem;
  T* s_P = (T*)(smem + (size_t)Gp * 4);
  for (int e = threadIdx.x; e < Gp; e += NT) s_toff[e] = toff[e];
  if (LDSP)
    for (int e = threadIdx.x; e < (Tn + 1) * KP; e += NT) s_P[e] = P[e];
  __syncthreads();
  const T* Pt = LDSP ? s_P : P;
  const int V = Gp >> 4, teams = NT / L, team = threadIdx.x / L, j = threadIdx.x % L;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n ? r0 + rpb : n;
  for (int64_t base = r0; base < r1; base += (int64_t)teams * UNR) {
    double acc[UNR][KP];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int k = 0; k < KP; ++k) acc[u][k] = 0.0;
    for (int c0 = 0; c0 < V; c0 += L) {
      const int c = c0 + j;
      uint4 q[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t i = base + (int64_t)u * teams + team;
        q[u] = make_uint4(0, 0, 0, 0);
        if (i < r1 && c < V) q[u] = ((const uint4*)(codes + i * Gp))[c];
      }
      if (c < V) {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          const int tb = s_toff[c * 16 + b];
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int row = tb + code_of(q[u], b);
#pragma unroll
            for (int k = 0; k < KP; ++k) acc[u][k] += (double)Pt[row * KP + k];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      for (int m = L >> 1; m > 0; m >>= 1)
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[u][k] += __shfl_xor(acc[u][k], m);
      const int64_t i = base + (int64_t)u * teams + team;
      if (i < r1 && j == 0) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) {
            double r = acc[u][k] + (u0 ? (double)u0[i * ldu + k] : 0.0);
            if (KP == 1) r = row_fn<T>(epi, r, w, i);
            out[i * ldo + k] = (T)r;
          }
      }
    }
  }
}

// grid (blocks, chunks): chunk y bins the groups [y * gpc, (y + 1) * gpc) of every row, reading
// only the 16-byte code vectors that hold them.  gpc is a multiple of 16, or a divisor of 16
// when the bins of 16 groups do not fit (then the chunk is a part of one vector).  The bins have
// no row for the padding columns: those are skipped.
template <typename T, int KP>
__global__ void __launch_bounds__(NB) lmm_kernel(const uint8_t* __restrict__ codes, int64_t n, int Gp, int gpc, int L,
                                                 const int* __restrict__ toff, int Tn, const T* __restrict__ Y, int ldy,
                                                 int K, double* __restrict__ slab, int64_t rpb) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int g0 = blockIdx.y * gpc, g1 = g0 + gpc < Gp ? g0 + gpc : Gp;
  const int v0 = g0 >> 4, v1 = (g1 + 15) >> 4;
  const int lo = toff[g0], hi = g1 < Gp ? toff[g1] : Tn;
  const int nb = (hi - lo) * KP, pad = Tn - lo;
  double* bins = (double*)smem;
  int* s_toff = (int*)(smem + (size_t)nb * 8);
  for (int e = threadIdx.x; e < nb; e += NB) bins[e] = 0.0;
  for (int e = threadIdx.x; e < g1 - g0; e += NB) s_toff[e] = toff[g0 + e] - lo;
  __syncthreads();
  const int teams = NB / L, team = threadIdx.x / L, j = threadIdx.x % L;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n ? r0 + rpb : n;
  for (int64_t base = r0; base < r1; base += (int64_t)teams * UNR) {
    for (int c = v0 + j; c < v1; c += L) {
      uint4 q[UNR];
      double y[UNR][KP];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t i = base + (int64_t)u * teams + team;
        q[u] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < KP; ++k) y[u][k] = 0.0;
        if (i < r1) {
          q[u] = ((const uint4*)(codes + i * Gp))[c];
#pragma unroll
          for (int k = 0; k < KP; ++k)
            if (k < K) y[u][k] = (double)Y[i * ldy + k];
        }
      }
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int g = c * 16 + b;
        if (g < g0 || g >= g1) continue;  // another chunk's group
        const int tb = s_toff[g - g0];
        if (tb == pad) continue;          // padding column
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int64_t i = base + (int64_t)u * teams + team;
          if (i < r1) {
            const int row = tb + code_of(q[u], b);
#pragma unroll
            for (int k = 0; k < KP; ++k)
              if (k < K) atomicAdd(&bins[row * KP + k], y[u][k]);
          }
        }
      }
    }
  }
  __syncthreads();
  double* dst = slab + (int64_t)blockIdx.x * Tn * KP + (int64_t)lo * KP;
  for (int e = threadIdx.x; e < nb; e += NB) dst[e] = bins[e];
}

// one pass, K = 1, at most 64 code vectors per row (one per lane of the row's team)
template <typename T>
__global__ void __launch_bounds__(NB) chain_kernel(const uint8_t* __restrict__ codes, int64_t n, int Gp, int L,
                                                   const int* __restrict__ toff, const T* __restrict__ P, int Tn,
                                                   const T* __restrict__ u0, const T* __restrict__ w, int epi,
                                                   T* __restrict__ gout, double* __restrict__ slab, int64_t rpb) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* bins = (double*)smem;
  T* s_P = (T*)(smem + (size_t)Tn * 8);
  int* s_toff = (int*)(smem + (size_t)Tn * 8 + (size_t)(Tn + 1) * sizeof(T));
  for (int e = threadIdx.x; e < Tn; e += NB) bins[e] = 0.0;
  for (int e = threadIdx.x; e <= Tn; e += NB) s_P[e] = P[e];
  for (int e = threadIdx.x; e < Gp; e += NB) s_toff[e] = toff[e];
  __syncthreads();
  const int V = Gp >> 4, teams = NB / L, team = threadIdx.x / L, j = threadIdx.x % L;
  const bool lane_on = j < V;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < n ? r0 + rpb : n;
  for (int64_t base = r0; base < r1; base += (int64_t)teams * UNR) {
    uint4 q[UNR];
    double acc[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t i = base + (int64_t)u * teams + team;
      q[u] = make_uint4(0, 0, 0, 0);
      acc[u] = 0.0;
      if (i < r1 && lane_on) q[u] = ((const uint4*)(codes + i * Gp))[j];
    }
    if (lane_on) {
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int tb = s_toff[j * 16 + b];
#pragma unroll
        for (int u = 0; u < UNR; ++u) acc[u] += (double)s_P[tb + code_of(q[u], b)];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      for (int m = L >> 1; m > 0; m >>= 1) acc[u] += __shfl_xor(acc[u], m);
      const int64_t i = base + (int64_t)u * teams + team;
      if (i < r1) {
        const double g = row_fn<T>(epi, acc[u] + (u0 ? (double)u0[i] : 0.0), w, i);
        acc[u] = g;
        if (gout && j == 0) gout[i] = (T)g;
      }
    }
    if (lane_on) {
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int tb = s_toff[j * 16 + b];
        if (tb == Tn) continue;           // padding column
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int64_t i = base + (int64_t)u * teams + team;
          if (i < r1) atomicAdd(&bins[tb + code_of(q[u], b)], acc[u]);
        }
      }
    }
  }
  __syncthreads();
  double* dst = slab + (int64_t)blockIdx.x * Tn;
  for (int e = threadIdx.x; e < Tn; e += NB) dst[e] = bins[e];
}

// Row-window decompression: out[(i - r0) * ldo + d] = the dictionary value of column d in row i,
// or zero for a column outside the packed groups (mc_grp[d] < 0), for r0 <= i < r1 and d < D.
// A workgroup takes tiles of R consecutive rows: their code vectors are one contiguous piece of
// the code matrix, copied to LDS with 16-byte loads.  Then a team of LR lanes walks along an
// output row, lane j writing the columns [c * W, c * W + W) of chunks c = j, j + LR, ... (W = one
// 16-byte store when VEC, else one value), so a wave's stores are contiguous; the chunk's column
// tables are read once per tile and chunk, not per row.  LDSD: the flattened dictionaries are
// staged in LDS, else read through the cache.  Tiles are independent: no atomics, no order.
template <typename T, bool VEC, bool LDSD>
__global__ void __launch_bounds__(NT) decomp_kernel(const uint8_t* __restrict__ codes, int Gp, int64_t r0, int64_t r1,
                                                    int D, const int* __restrict__ mc_grp,
                                                    const int* __restrict__ mc_doff, const int* __restrict__ mc_nc,
                                                    const T* __restrict__ dvals, int ndv, T* __restrict__ out,
                                                    int64_t ldo, int R, int LR) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int W = VEC ? (int)(16 / sizeof(T)) : 1;
  typedef T Pack __attribute__((ext_vector_type(W)));   // W = 4 / 2: one 16-byte store
  uint8_t* s_codes = smem;                           // R * Gp bytes, a multiple of 16
  T* s_dv = (T*)(smem + (size_t)R * Gp);
  if (LDSD)
    for (int e = threadIdx.x; e < ndv; e += NT) s_dv[e] = dvals[e];
  const T* dv = LDSD ? s_dv : dvals;
  const int V = Gp >> 4, CH = (D + W - 1) / W;
  const int teams = NT / LR, team = threadIdx.x / LR, j = threadIdx.x % LR;
  const int64_t ntiles = (r1 - r0 + R - 1) / R;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = r0 + t * R;
    const int rows = (int)(r1 - row0 < R ? r1 - row0 : R);
    __syncthreads();                                 // the previous tile's codes are no longer read
    const uint4* src = (const uint4*)(codes + row0 * Gp);
    for (int e = threadIdx.x; e < rows * V; e += NT) ((uint4*)s_codes)[e] = src[e];
    __syncthreads();
    for (int c = j; c < CH; c += LR) {
      // a column outside the packed groups reads group 0's code and dvals[0], and writes zero
      int grp[W], off[W], nc[W];
      bool on[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int d = c * W + w;
        const int g = d < D ? mc_grp[d] : -1;
        on[w] = g >= 0;
        grp[w] = on[w] ? g : 0;
        off[w] = on[w] ? mc_doff[d] : 0;
        nc[w] = on[w] ? mc_nc[d] : 0;
      }
      for (int r = team; r < rows; r += teams) {
        Pack p;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const T x = dv[off[w] + (int)s_codes[r * Gp + grp[w]] * nc[w]];
          p[w] = on[w] ? x : (T)0;
        }
        T* dst = out + (row0 - r0 + r) * ldo + (int64_t)c * W;
        if (c * W + W <= D) {
          *(Pack*)dst = p;
        } else {
#pragma unroll
          for (int w = 0; w < W; ++w)
            if (c * W + w < D) dst[w] = p[w];
        }
      }
    }
  }
}

// rows of a decompression tile: 16 KiB of codes, at most 256 rows
int decomp_tile_rows(int Gp) {
  const int R = 16384 / Gp;
  return R < 1 ? 1 : R > 256 ? 256 : R;
}

// rows per block: an even share, rounded up to whole iterations of the block's teams
int64_t rows_per_block(int64_t n, int grid, int L, int nt = NT) {
  const int64_t span = (int64_t)(nt / L) * UNR;
  return ((n + grid - 1) / grid + span - 1) / span * span;
}

int team_lanes(int nv) {
  int L = 1;
  while (L < nv && L < 64) L <<= 1;
  return L;
}

template <typename F>
int allow_lds(F* fn, size_t lds) {
  if (lds <= 64 * 1024) return 0;
  return (int)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

constexpr size_t kMaxLds = 160 * 1024;

template <typename T, int KP>
int rmm_launch(const uint8_t* codes, int64_t n, int Gp, const int* toff, const T* P, int Tn, int K, const T* u0,
               int ldu, T* out, int ldo, int epi, const T* w, int grid, hipStream_t st) {
  const size_t pb = (size_t)(Tn + 1) * KP * sizeof(T);
  const bool in_lds = pb <= (size_t)g_budget && (size_t)Gp * 4 + pb <= kMaxLds;
  const size_t lds = (size_t)Gp * 4 + (in_lds ? pb : 0);
  const int L = team_lanes(Gp >> 4);
  const int64_t rpb = rows_per_block(n, grid, L);
  if (in_lds) {
    auto fn = rmm_kernel<T, KP, true>;
    if (int rc = allow_lds(fn, lds)) return rc;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), lds, st, codes, n, Gp, L, toff, P, Tn, u0, ldu, K, out, ldo, epi, w,
                       rpb);
  } else {
    auto fn = rmm_kernel<T, KP, false>;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), lds, st, codes, n, Gp, L, toff, P, Tn, u0, ldu, K, out, ldo, epi, w,
                       rpb);
  }
  return (int)hipGetLastError();
}

template <typename T>
int rmm_kp(int KP, const uint8_t* codes, int64_t n, int Gp, const int* toff, const void* P, int Tn, int K,
           const void* u0, int ldu, void* out, int ldo, int epi, const void* w, int grid, hipStream_t st) {
#define RMM(KP_) \
  return rmm_launch<T, KP_>(codes, n, Gp, toff, (const T*)P, Tn, K, (const T*)u0, ldu, (T*)out, ldo, epi, \
                            (const T*)w, grid, st)
  switch (KP) {
    case 1: RMM(1);
    case 2: RMM(2);
    case 4: RMM(4);
    case 8: RMM(8);
  }
#undef RMM
  return -1;
}

template <typename T, int KP>
int lmm_launch(const uint8_t* codes, int64_t n, int Gp, const int* toff, int Tn, const T* Y, int ldy, int K, int gpc,
               size_t lds, double* slab, int grid, hipStream_t st) {
  auto fn = lmm_kernel<T, KP>;
  if (int rc = allow_lds(fn, lds)) return rc;
  const int chunks = (Gp + gpc - 1) / gpc, L = team_lanes((gpc + 15) >> 4);
  const int64_t rpb = rows_per_block(n, grid, L, NB);
  hipLaunchKernelGGL(fn, dim3(grid, chunks), dim3(NB), lds, st, codes, n, Gp, gpc, L, toff, Tn, Y, ldy, K, slab, rpb);
  return (int)hipGetLastError();
}

template <typename T>
int lmm_kp(int KP, const uint8_t* codes, int64_t n, int Gp, const int* toff, int Tn, const void* Y, int ldy, int K,
           int gpc, size_t lds, double* slab, int grid, hipStream_t st) {
#define LMM(KP_) return lmm_launch<T, KP_>(codes, n, Gp, toff, Tn, (const T*)Y, ldy, K, gpc, lds, slab, grid, st)
  switch (KP) {
    case 1: LMM(1);
    case 2: LMM(2);
    case 4: LMM(4);
    case 8: LMM(8);
  }
#undef LMM
  return -1;
}

template <typename T>
int chain_launch(const uint8_t* codes, int64_t n, int Gp, const int* toff, const T* P, int Tn, const T* u0, const T* w,
                 int epi, T* gout, double* slab, int grid, hipStream_t st) {
  const size_t tab = (size_t)Tn * 8 + (size_t)(Tn + 1) * sizeof(T), lds = tab + (size_t)Gp * 4;
  if (tab > (size_t)g_budget || Gp > 1024 || lds > kMaxLds) return -1;
  auto fn = chain_kernel<T>;
  if (int rc = allow_lds(fn, lds)) return rc;
  const int64_t rpb = rows_per_block(n, grid, team_lanes(Gp >> 4), NB);
  hipLaunchKernelGGL(fn, dim3(grid), dim3(NB), lds, st, codes, n, Gp, team_lanes(Gp >> 4), toff, P, Tn, u0, w, epi,
                     gout, slab, rpb);
  return (int)hipGetLastError();
}

template <typename T>
int decomp_launch(const uint8_t* codes, int Gp, int64_t r0, int64_t r1, int D, const int* mc_grp, const int* mc_doff,
                  const int* mc_nc, const T* dvals, int ndv, T* out, int64_t ldo, int grid, hipStream_t st) {
  const int R = decomp_tile_rows(Gp);
  const size_t cb = (size_t)R * Gp, db = (size_t)ndv * sizeof(T);
  const bool in_lds = db <= (size_t)g_budget && cb + db <= kMaxLds;
  const size_t lds = cb + (in_lds ? db : 0);
  const bool vec = (ldo * sizeof(T)) % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int W = vec ? (int)(16 / sizeof(T)) : 1, CH = (D + W - 1) / W;
  int LR = 1;
  while (LR < CH && LR < NT) LR <<= 1;
  const int64_t ntiles = (r1 - r0 + R - 1) / R;
  if (grid > ntiles) grid = (int)ntiles;
#define DECOMP(VEC_, LDS_)                                                                                         \
  do {                                                                                                             \
    auto fn = decomp_kernel<T, VEC_, LDS_>;                                                                        \
    if (int rc = allow_lds(fn, lds)) return rc;                                                                    \
    hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), lds, st, codes, Gp, r0, r1, D, mc_grp, mc_doff, mc_nc, dvals, ndv, \
                       out, ldo, R, LR);                                                                           \
  } while (0)
  if (vec && in_lds)
    DECOMP(true, true);
  else if (vec)
    DECOMP(true, false);
  else if (in_lds)
    DECOMP(false, true);
  else
    DECOMP(false, false);
#undef DECOMP
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// threads of a workgroup of the binning kernels: each workgroup writes one row of the slab
int sysml_cla_threads() { return NB; }

int sysml_cla_budget() { return g_budget; }

// tuning hook of tools/bench_cla.py (the budget sweep); 0 restores the built-in constant
void sysml_cla_set_budget(int bytes) {
  g_budget = bytes <= 0 ? kLdsBudget : (bytes > 144 * 1024 ? 144 * 1024 : bytes);
}

// dt: 1 = fp32, 2 = fp64 (values, V, P)
int sysml_cla_dictmm(int dt, const void* dv, const int* tup_off, const int* tup_nc, const int* tup_c0,
                     const int* colidx, const void* V, int K, int KP, int Tn, void* P, void* stream) {
  const int64_t tot = (int64_t)(Tn + 1) * KP;
  const dim3 g((unsigned)((tot + NT - 1) / NT)), t(NT);
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    hipLaunchKernelGGL(dictmm_kernel<float>, g, t, 0, st, (const float*)dv, tup_off, tup_nc, tup_c0, colidx,
                       (const float*)V, K, KP, Tn, (float*)P);
  else if (dt == 2)
    hipLaunchKernelGGL(dictmm_kernel<double>, g, t, 0, st, (const double*)dv, tup_off, tup_nc, tup_c0, colidx,
                       (const double*)V, K, KP, Tn, (double*)P);
  else
    return -1;
  return (int)hipGetLastError();
}

// bins (width fp64) = the sum of the nb rows of slab, in a fixed order
int sysml_cla_fold(const double* slab, double* bins, int nb, int64_t width, void* stream) {
  if (nb < 1 || width < 1) return -1;
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((width + 15) / 16)), dim3(NT), 0, (hipStream_t)stream, slab, bins,
                     nb, width);
  return (int)hipGetLastError();
}

int sysml_cla_dicttmm(int dt, const void* dv, const int* col_out, const int* col_doff, const int* col_nc,
                      const int* col_t0, const int* col_T, int C, const double* bins, int K, int KP, void* out, int ldo,
                      void* stream) {
  const int64_t tot = (int64_t)C * K;
  const dim3 g((unsigned)((tot + NT - 1) / NT)), t(NT);
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    hipLaunchKernelGGL(dicttmm_kernel<float>, g, t, 0, st, (const float*)dv, col_out, col_doff, col_nc, col_t0, col_T,
                       C, bins, K, KP, (float*)out, ldo);
  else if (dt == 2)
    hipLaunchKernelGGL(dicttmm_kernel<double>, g, t, 0, st, (const double*)dv, col_out, col_doff, col_nc, col_t0,
                       col_T, C, bins, K, KP, (double*)out, ldo);
  else
    return -1;
  return (int)hipGetLastError();
}

// out (n x K, leading dimension ldo) = u0 + gather of P; epi / w: the K = 1 row function
int sysml_cla_rmm(int dt, const void* codes, int64_t n, int Gp, const int* toff, const void* P, int Tn, int K, int KP,
                  const void* u0, int ldu, void* out, int ldo, int epi, const void* w, int grid, void* stream) {
  if (n <= 0 || Gp <= 0 || (Gp & 15) || Gp > 16384 || grid <= 0 || K < 1 || K > KP) return -1;
  if (epi != 0 && (KP != 1 || !w)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    return rmm_kp<float>(KP, (const uint8_t*)codes, n, Gp, toff, P, Tn, K, u0, ldu, out, ldo, epi, w, grid, st);
  if (dt == 2)
    return rmm_kp<double>(KP, (const uint8_t*)codes, n, Gp, toff, P, Tn, K, u0, ldu, out, ldo, epi, w, grid, st);
  return -1;
}

// slab (grid x Tn * KP fp64): every block's bins; gpc groups per chunk (a multiple or a divisor
// of 16), lds the bytes of the largest chunk's bins plus its offsets (ops/kernels.py _cla_chunks)
int sysml_cla_lmm(int dt, const void* codes, int64_t n, int Gp, const int* toff, int Tn, const void* Y, int ldy, int K,
                  int KP, int gpc, int64_t lds, double* slab, int grid, void* stream) {
  if (n <= 0 || Gp <= 0 || (Gp & 15) || grid <= 0 || K < 1 || K > KP || lds <= 0 || (size_t)lds > kMaxLds) return -1;
  if (gpc < 1 || (gpc & 15 && 16 % gpc)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    return lmm_kp<float>(KP, (const uint8_t*)codes, n, Gp, toff, Tn, Y, ldy, K, gpc, (size_t)lds, slab, grid, st);
  if (dt == 2)
    return lmm_kp<double>(KP, (const uint8_t*)codes, n, Gp, toff, Tn, Y, ldy, K, gpc, (size_t)lds, slab, grid, st);
  return -1;
}

// slab (grid x Tn fp64); -1 when P plus the bins exceed the budget or a row has more than
// 64 code vectors
int sysml_cla_chain(int dt, const void* codes, int64_t n, int Gp, const int* toff, const void* P, int Tn,
                    const void* u0, const void* w, int epi, void* gout, double* slab, int grid, void* stream) {
  if (n <= 0 || Gp <= 0 || (Gp & 15) || grid <= 0 || (epi != 0 && !w)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    return chain_launch<float>((const uint8_t*)codes, n, Gp, toff, (const float*)P, Tn, (const float*)u0,
                               (const float*)w, epi, (float*)gout, slab, grid, st);
  if (dt == 2)
    return chain_launch<double>((const uint8_t*)codes, n, Gp, toff, (const double*)P, Tn, (const double*)u0,
                                (const double*)w, epi, (double*)gout, slab, grid, st);
  return -1;
}

// out ((r1 - r0) x D, leading dimension ldo >= D) = rows [r0, r1) of the packed groups, zero in
// the columns of the other groups (mc_grp < 0); n rows of codes, ndv values in dvals.  16-byte
// stores when ldo and out allow them.  grid: workgroups at most (one tile of rows each at least)
int sysml_cla_decompress(int dt, const void* codes, int64_t n, int Gp, int64_t r0, int64_t r1, int D,
                         const int* mc_grp, const int* mc_doff, const int* mc_nc, const void* dvals, int ndv,
                         void* out, int64_t ldo, int grid, void* stream) {
  if (Gp <= 0 || (Gp & 15) || Gp > 16384 || r0 < 0 || r0 >= r1 || r1 > n || D < 1 || ldo < D || ndv < 1 || grid <= 0)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dt == 1)
    return decomp_launch<float>((const uint8_t*)codes, Gp, r0, r1, D, mc_grp, mc_doff, mc_nc, (const float*)dvals, ndv,
                                (float*)out, ldo, grid, st);
  if (dt == 2)
    return decomp_launch<double>((const uint8_t*)codes, Gp, r0, r1, D, mc_grp, mc_doff, mc_nc, (const double*)dvals,
                                 ndv, (double*)out, ldo, grid, st);
  return -1;
}

}  // extern "C"
