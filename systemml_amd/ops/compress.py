"""Compressed linear algebra (reference: runtime/compress/{CompressedMatrixBlock,ColGroupDDC*,
ColGroupOLE,ColGroupRLE,ColGroupUncompressed}.java, compress/cocode/*, compress/estim/*;
enabled by sysml.compressed.linalg = auto | true | false).

A column group G is a set of columns whose rows take few distinct value tuples; it stores a
dictionary D_G (#tuples x |G|) plus one of four row encodings, chosen per group by the
smallest in-memory size (reference: CompressedSizeEstimator + the planner's per-group choice):

* DDC  one uint8 / int16 / int32 code per row (dense dictionary coding);
* OLE  offset lists: for every non-zero tuple the rows holding it (the all-zero tuple is
       implicit), stored as one int32 row stream grouped by tuple + per-tuple counts;
* RLE  runs: (tuple, start, length) per maximal run of equal non-zero tuples, zero runs
       implicit -- sorted / clustered columns compress to a handful of runs;
* UNC  columns that do not compress, kept dense.

MI355X design: every operation is expressed as a small dictionary product plus one gather /
scatter over the encoded rows, so the row stream is read once and the work per row is a few
bytes -- the GPU form of the reference's per-group kernels:

* X %*% V   = sum_G  (D_G V_G)[codes_G]            DDC: gather by code; OLE / RLE: scatter-add
                                                    of the tuple's product row into its rows
* t(X) %*% Y = D_G^T  (rows of Y binned per tuple)  DDC: index_add by code; OLE / RLE: by the
                                                    entries' tuple ids
* sum / rowSums / colSums operate on dictionaries, tuple counts and entry lists.

The DDC groups with uint8 codes of a matrix in HBM are packed into one row-major code block
(CLAPack, built on first use) and their X %*% V, t(X) %*% Y (K <= 8) and single-column
mmchains run on ops/hip/cla.hip: one pass over the codes for all groups instead of one pass
over the output per group (reference: ColGroupDDC1.rightMultByVector over a group array,
CompressedMatrixBlock.chainMatrixMultOperations).  The other groups keep the per-group code
below and are added to the kernels' results; so do all host matrices.

decompress(r0, r1) produces a dense row window (reference: ColGroup*.decompressToBlock(target,
rl, ru)): the packed groups in one launch, the others per group on the window's rows.  Right
indexing decompresses only its rows, and t(X) %*% X is the sum over such windows of the dense
tsmm (reference: CompressedMatrixBlock.transposeSelfMatrixMultOperations), so neither holds
the dense matrix.

Planning (cocode): per-column distinct counts on a sample, columns with few distinct values
are greedily merged while the joint tuple count stays <= 255 (uint8 codes).
"""
from __future__ import annotations

import math

import torch

MAX_TUPLES_U8 = 255
MAX_TUPLES = 32767
MIN_CELLS = 1 << 20
KINDS = ("ddc", "ole", "rle", "unc")


class ColGroup:
    """One column group.  ddc: codes (n,); ole: rows (nnz,) int32 grouped by tuple with
    tid (nnz,) tuple ids; rle: starts / lens / tid per run; unc: dict is the column block."""
    __slots__ = ("kind", "cols", "dict", "codes", "rows", "tid", "starts", "lens", "nrows")

    def __init__(self, kind, cols, dictionary, nrows, codes=None, rows=None, tid=None, starts=None, lens=None):
        self.kind = kind
        self.cols = cols              # int64 column indices
        self.dict = dictionary        # (#tuples x |cols|), compute dtype
        self.nrows = nrows
        self.codes = codes
        self.rows = rows
        self.tid = tid
        self.starts = starts
        self.lens = lens

    @property
    def uncompressed(self):
        return self.kind == "unc"

    def nbytes(self):
        b = self.dict.numel() * self.dict.element_size()
        for t in (self.codes, self.rows, self.tid, self.starts, self.lens):
            if t is not None:
                b += t.numel() * t.element_size()
        return b

    def entries(self):
        """(row indices, tuple ids) of the stored (non-implicit) cells, int64."""
        if self.kind == "ddc":
            return torch.arange(self.nrows, device=self.codes.device), self.codes.long()
        if self.kind == "ole":
            return self.rows.long(), self.tid.long()
        if self.kind == "rle":
            lens = self.lens.long()
            total = int(lens.sum().item())
            first = torch.cumsum(lens, 0) - lens
            rid = torch.repeat_interleave(torch.arange(lens.numel(), device=lens.device), lens)
            rows = self.starts.long()[rid] + (torch.arange(total, device=lens.device) - first[rid])
            return rows, self.tid.long()[rid]
        raise ValueError(self.kind)

    def counts(self):
        """Number of rows holding each dictionary tuple."""
        T = self.dict.shape[0]
        if self.kind == "ddc":
            c = torch.bincount(self.codes.long(), minlength=T)
        elif self.kind == "ole":
            c = torch.bincount(self.tid.long(), minlength=T)
        else:
            c = torch.zeros(T, dtype=torch.int64, device=self.dict.device)
            c.index_add_(0, self.tid.long(), self.lens.long())
        return c.to(self.dict.dtype)

    def with_dict(self, d):
        return ColGroup(self.kind, self.cols, d, self.nrows, self.codes, self.rows, self.tid, self.starts, self.lens)


class CLAPack:
    """The uint8 DDC groups of one matrix in the layout of ops/hip/cla.hip.

    codes   uint8 n x Gp row-major, Gp = 16 * ceil(G / 16); padding columns hold code 0.
    toff    int32 [Gp]: row of each group's tuple 0 in the concatenated table of T = sum T_g
            rows plus the extra row T, which every padding column points at.
    dvals   all dictionaries, flattened row-major, in the matrix dtype.
    tup_*   per tuple (T): offset of its values in dvals, its group's column count and the
            offset of its group's columns in colidx -- the dictionary product P = D V is one
            launch over the tuples.
    col_*   per packed column (C): its matrix column, the offset of its first value in dvals,
            the value stride (column count), and its group's first tuple / tuple count -- the
            transposed dictionary product is one launch over the columns.
    mc_*    per matrix column (D): its group's column in codes (-1 for a column outside the packed
            groups), the offset of its first value in dvals and the value stride -- a row window
            is decompressed by one launch over the window's cells.
    valid   every code is below its group's tuple count (checked once, here)."""
    __slots__ = ("codes", "toff", "toff_host", "G", "Gp", "T", "index", "dvals", "tup_off", "tup_nc", "tup_c0",
                 "colidx", "col_out", "col_doff", "col_nc", "col_t0", "col_T", "C", "mc_grp", "mc_doff", "mc_nc",
                 "valid", "_chunks")

    def with_dicts(self, groups):
        """The pack of a matrix with the same codes and other dictionary values (scale)."""
        p = CLAPack()
        for a in self.__slots__:
            setattr(p, a, getattr(self, a))
        p._chunks = {}
        p.dvals = torch.cat([groups[i].dict.reshape(-1) for i in self.index])
        return p


def _packable(g):
    return g.kind == "ddc" and g.codes is not None and g.codes.dtype == torch.uint8


def _build_pack(cm):
    """Pack the uint8 DDC groups of `cm` (plain tensor code: any device) and rebind their codes
    to column views of the packed block; None when no group qualifies."""
    index = [i for i, g in enumerate(cm.groups) if _packable(g)]
    if not index:
        return None
    gs = [cm.groups[i] for i in index]
    n, dev = cm.shape[0], cm.device
    G = len(gs)
    Gp = 16 * ((G + 15) // 16)
    p = CLAPack()
    p.G, p.Gp, p.index, p._chunks = G, Gp, index, {}
    Ts = [int(g.dict.shape[0]) for g in gs]
    ncs = [int(g.cols.numel()) for g in gs]
    T = sum(Ts)
    toff = [0] * G
    for j in range(1, G):
        toff[j] = toff[j - 1] + Ts[j - 1]
    p.T = T
    p.toff_host = toff + [T] * (Gp - G)
    i32 = dict(dtype=torch.int32, device=dev)
    p.toff = torch.tensor(p.toff_host, **i32)
    codes = torch.zeros((n, Gp), dtype=torch.uint8, device=dev)
    if n > 0:
        codes[:, :G] = torch.stack([g.codes for g in gs], dim=1)
    # one reduction and one host read: the kernels index LDS tables by these codes
    p.valid = n == 0 or bool((codes[:, :G].amax(0).to(torch.int32) < torch.tensor(Ts, **i32)).all().item())
    p.codes = codes
    for j, g in enumerate(gs):
        g.codes = codes[:, j]
    p.dvals = torch.cat([g.dict.reshape(-1) for g in gs])
    doff, coff = [0] * G, [0] * G
    for j in range(1, G):
        doff[j] = doff[j - 1] + Ts[j - 1] * ncs[j - 1]
        coff[j] = coff[j - 1] + ncs[j - 1]
    tid = torch.arange(T, **i32)
    grp = torch.repeat_interleave(torch.arange(G, device=dev), torch.tensor(Ts, device=dev))
    t_nc = torch.tensor(ncs, **i32)[grp]
    p.tup_nc = t_nc
    p.tup_off = torch.tensor(doff, **i32)[grp] + (tid - p.toff[:G][grp]) * t_nc
    p.tup_c0 = torch.tensor(coff, **i32)[grp]
    p.colidx = torch.cat([g.cols for g in gs]).to(torch.int32)
    p.C = int(p.colidx.numel())
    cgrp = torch.repeat_interleave(torch.arange(G, device=dev), torch.tensor(ncs, device=dev))
    p.col_out = p.colidx
    p.col_nc = torch.tensor(ncs, **i32)[cgrp]
    p.col_doff = torch.tensor(doff, **i32)[cgrp] + (torch.arange(p.C, **i32) - torch.tensor(coff, **i32)[cgrp])
    p.col_t0 = p.toff[:G][cgrp]
    p.col_T = torch.tensor(Ts, **i32)[cgrp]
    at = p.colidx.long()
    p.mc_grp = torch.full((cm.shape[1],), -1, **i32)
    p.mc_grp[at] = cgrp.to(torch.int32)
    p.mc_doff = torch.zeros(cm.shape[1], **i32)
    p.mc_doff[at] = p.col_doff
    p.mc_nc = torch.zeros(cm.shape[1], **i32)
    p.mc_nc[at] = p.col_nc
    return p


class CompressedMatrix:
    def __init__(self, nrows, ncols, groups, dtype, device):
        self.shape = (nrows, ncols)
        self.groups = groups
        self.dtype = dtype
        self.device = device
        self._pack = False            # False: not built yet; None: no uint8 DDC group

    # ------------------------------------------------------------------ packed DDC block
    def pack(self):
        """The packed uint8 DDC groups (CLAPack), built on first use and kept; None for host
        matrices and when no group qualifies."""
        if self._pack is False:
            if torch.device(self.device).type != "cuda":
                return None
            self._pack = _build_pack(self)
        return self._pack

    def _cla_on(self):
        """The HIP kernels of ops/hip/cla.hip serve this matrix (HBM, fp32 / fp64, kernels on)."""
        if torch.device(self.device).type != "cuda" or self.dtype not in (torch.float32, torch.float64):
            return False
        from .backend import backend
        from . import kernels
        return bool(backend.use_kernels and kernels.CLA)

    def _cla(self, K):
        """The pack when a product with K columns runs on the HIP kernels."""
        if K < 1 or K > 8 or not self._cla_on():
            return None
        p = self.pack()
        return p if p is not None and p.valid else None

    def _rest(self, p):
        packed = set(p.index)
        return [g for i, g in enumerate(self.groups) if i not in packed]

    # ------------------------------------------------------------------ info
    def nbytes(self):
        b = sum(g.nbytes() for g in self.groups)
        p = self._pack
        if p:
            b += self.shape[0] * (p.Gp - p.G)      # the padding columns of the packed codes
        return b

    def ratio(self):
        return self.shape[0] * self.shape[1] * torch.empty((), dtype=self.dtype).element_size() / max(self.nbytes(), 1)

    def kinds(self):
        out = {}
        for g in self.groups:
            out[g.kind] = out.get(g.kind, 0) + 1
        return out

    def __repr__(self):
        return (f"CompressedMatrix({self.shape[0]}x{self.shape[1]}, {len(self.groups)} groups {self.kinds()}, "
                f"ratio {self.ratio():.1f})")

    # ------------------------------------------------------------------ decompress
    def decompress(self, r0=0, r1=None):
        """The dense matrix, or with a range its rows [r0, r1) only (reference:
        ColGroup*.decompressToBlock(target, rl, ru)): the packed groups of a matrix in HBM in one
        launch of ops/hip/cla.hip, the other groups -- and every group of a host matrix -- by
        the per-group code on the window's rows.  An isolated window costs O(window) for UNC and
        DDC groups and O(stored entries) for OLE / RLE groups."""
        n = self.shape[0]
        r0, r1 = int(r0), n if r1 is None else int(r1)
        if not 0 <= r0 <= r1 <= n:
            raise ValueError(f"row window [{r0}, {r1}) outside the {n} rows of the matrix")
        out = torch.empty((r1 - r0, self.shape[1]), dtype=self.dtype, device=self.device)
        self._window(out, r0, r1)
        return out

    def _window(self, out, r0, r1, ordered=None):
        """Fill out ((r1 - r0) x D, any row pitch) with the rows [r0, r1); every cell is written.
        `ordered`: the OLE / RLE entries by row (_row_ordered) with r0 and r1 among their cuts.
        True when the packed groups were written by the HIP kernel."""
        if r1 <= r0:
            return False
        groups, hip = self.groups, False
        p = self._cla(1)
        if p is not None:
            from . import kernels
            if kernels.cla_decompress(p, r0, r1, out) is not None:
                groups, hip = self._rest(p), True
        if not hip:
            out.zero_()
        for g in groups:
            if g.kind == "unc":
                out[:, g.cols] = g.dict[r0:r1]
            elif g.kind == "ddc":
                out[:, g.cols] = g.dict.index_select(0, g.codes[r0:r1].long())
            else:
                if ordered is not None:
                    rows, tid, cuts = ordered[id(g)]
                    lo, hi = cuts[r0], cuts[r1]
                    rows, tid = rows[lo:hi] - r0, tid[lo:hi]
                else:
                    rows, tid = g.entries()
                    if r0 > 0 or r1 < self.shape[0]:
                        m = (rows >= r0) & (rows < r1)
                        rows, tid = rows[m] - r0, tid[m]
                blk = torch.zeros((r1 - r0, g.cols.numel()), dtype=self.dtype, device=self.device)
                blk[rows] = g.dict.index_select(0, tid)
                out[:, g.cols] = blk
        return hip

    def _row_ordered(self, bounds):
        """The stored entries of every OLE / RLE group ordered by row, and for each row in
        `bounds` the number of entries before it: expanded and sorted once for all the windows
        between consecutive bounds."""
        at = torch.tensor(bounds, device=self.device)
        res = {}
        for g in self.groups:
            if g.kind in ("ole", "rle"):
                rows, tid = g.entries()
                order = torch.argsort(rows)
                rows, tid = rows[order], tid[order]
                res[id(g)] = (rows, tid, dict(zip(bounds, torch.searchsorted(rows, at).tolist())))
        return res

    # ------------------------------------------------------------------ t(X) %*% X
    def tsmm(self):
        """t(X) %*% X without the dense matrix (reference: CompressedMatrixBlock.
        transposeSelfMatrixMultOperations): the sum, in row order, of the dense tsmm of row
        windows decompressed into one reused buffer of kernels._CLA_TSMM_SCRATCH bytes.  In HBM
        the window is written by ops/hip/cla.hip (packed groups) and multiplied by the exact
        fp32 / fp64 MFMA tsmm of ops/hip/gemm.hip; on the host by addmm."""
        from . import kernels
        from .backend import backend
        n, D = self.shape
        if n == 0 or D == 0:
            return torch.zeros((D, D), dtype=self.dtype, device=self.device)
        es = torch.empty((), dtype=self.dtype).element_size()
        step = max(1, min(n, kernels._CLA_TSMM_SCRATCH // (D * es)))
        bounds = list(range(0, n, step)) + [n]
        mfma = torch.device(self.device).type == "cuda" and backend.use_kernels and \
            self.dtype in (torch.float32, torch.float64)
        S = None if mfma else torch.zeros((D, D), dtype=self.dtype, device=self.device)
        ordered = self._row_ordered(bounds) if len(bounds) > 2 else None
        buf = torch.empty((step, D), dtype=self.dtype, device=self.device)
        hip = False
        for r0, r1 in zip(bounds, bounds[1:]):
            w = buf[:r1 - r0]
            hip = self._window(w, r0, r1, ordered) or hip
            if mfma:
                from . import gemm
                Sb = gemm.tsmm(w)
                S = Sb if S is None else S.add_(Sb)
            else:
                S.addmm_(w.t(), w)
        if hip:
            kernels._count("cla.tsmm")
        return S

    # ------------------------------------------------------------------ products
    def matmul(self, V):
        """X %*% V."""
        V = V.to(self.dtype)
        p = self._cla(V.shape[1]) if V.dim() == 2 else None
        if p is not None:
            from . import kernels
            rest = self._rest(p)
            r = kernels.cla_rmm(p, V, self._matmul_groups(rest, V) if rest else None)
            if r is not None:
                return r
        return self._matmul_groups(self.groups, V)

    def _matmul_groups(self, groups, V):
        out = torch.zeros((self.shape[0], V.shape[1]), dtype=self.dtype, device=self.device)
        for g in groups:
            Vg = V.index_select(0, g.cols)
            if g.kind == "unc":
                out += g.dict @ Vg
            elif g.kind == "ddc":
                out += (g.dict @ Vg).index_select(0, g.codes.long())
            else:
                rows, tid = g.entries()
                out.index_add_(0, rows, (g.dict @ Vg).index_select(0, tid))
        return out

    def tmatmul(self, Y):
        """t(X) %*% Y."""
        Y = Y.to(self.dtype)
        out = torch.zeros((self.shape[1], Y.shape[1]), dtype=self.dtype, device=self.device)
        p = self._cla(Y.shape[1]) if Y.dim() == 2 else None
        if p is not None:
            from . import kernels
            if kernels.cla_lmm(p, Y, out) is not None:
                return self._tmatmul_groups(self._rest(p), Y, out)
        return self._tmatmul_groups(self.groups, Y, out)

    def _tmatmul_groups(self, groups, Y, out):
        for g in groups:
            if g.kind == "unc":
                out[g.cols] = g.dict.t() @ Y
                continue
            bins = torch.zeros((g.dict.shape[0], Y.shape[1]), dtype=self.dtype, device=self.device)
            if g.kind == "ddc":
                bins.index_add_(0, g.codes.long(), Y)
            else:
                rows, tid = g.entries()
                bins.index_add_(0, tid, Y.index_select(0, rows))
            out[g.cols] = g.dict.t() @ bins
        return out

    def mmchain(self, ctype, v, w=None):
        """t(X) %*% f(X %*% v) for a single column v on the one-pass HIP chain (XtXv: f = id,
        XtwXv: w * u, XtXvy: u - y); None when it does not apply (host matrices, no packed
        group, other chain types, K > 1) and the caller composes the two products."""
        if ctype not in ("XtXv", "XtwXv", "XtXvy") or v.dim() != 2 or v.shape[1] != 1 or v.shape[0] != self.shape[1]:
            return None
        if (w is None) != (ctype == "XtXv") or (w is not None and tuple(w.shape) != (self.shape[0], 1)):
            return None
        p = self._cla(1)
        if p is None:
            return None
        from . import kernels
        v = v.to(device=self.device, dtype=self.dtype)
        w = w.to(device=self.device, dtype=self.dtype) if w is not None else None
        rest = self._rest(p)
        out = torch.zeros((self.shape[1], 1), dtype=self.dtype, device=self.device)
        g = kernels.cla_chain(p, ctype, v, w, self._matmul_groups(rest, v) if rest else None, out, bool(rest))
        if g is None:
            return None
        return self._tmatmul_groups(rest, g, out) if rest else out

    # ------------------------------------------------------------------ aggregates
    def colsums(self, sq=False):
        out = torch.zeros((1, self.shape[1]), dtype=self.dtype, device=self.device)
        for g in self.groups:
            d = g.dict * g.dict if sq else g.dict
            if g.kind == "unc":
                out[0, g.cols] = d.sum(0)
            else:
                out[0, g.cols] = g.counts() @ d
        return out

    def rowsums(self, sq=False):
        out = torch.zeros((self.shape[0], 1), dtype=self.dtype, device=self.device)
        for g in self.groups:
            d = g.dict * g.dict if sq else g.dict
            rs = d.sum(1, keepdim=True)
            if g.kind == "unc":
                out += rs
            elif g.kind == "ddc":
                out += rs.index_select(0, g.codes.long())
            else:
                rows, tid = g.entries()
                out.index_add_(0, rows, rs.index_select(0, tid))
        return out

    def scale(self, s):
        """X * s on the dictionaries; OLE / RLE keep their implicit zeros, so a non-finite
        factor (0 * inf = NaN) is applied to the decompressed matrix instead."""
        if not math.isfinite(s) and any(g.kind in ("ole", "rle") for g in self.groups):
            return self.decompress() * s
        if self._cla_on():
            self.pack()               # before the groups are copied: they share the packed codes
        gs = [g.with_dict(g.dict * s) for g in self.groups]
        cm = CompressedMatrix(self.shape[0], self.shape[1], gs, self.dtype, self.device)
        if self._pack is not False:   # same codes and offsets, new dictionary values
            cm._pack = self._pack.with_dicts(gs) if self._pack is not None else None
        return cm


def is_compressed(x):
    return isinstance(x, CompressedMatrix)


# ----------------------------------------------------------------------------
# planning + compression
# ----------------------------------------------------------------------------
def _encode(cols_data):
    """Distinct row tuples of an (n x k) block -> (dictionary, int64 codes)."""
    uniq, inv = torch.unique(cols_data, dim=0, return_inverse=True)
    return uniq, inv


def _code_dtype(ntup):
    return torch.uint8 if ntup <= MAX_TUPLES_U8 + 1 else torch.int16 if ntup <= MAX_TUPLES else torch.int32


def _sizes(d, codes, n):
    """Estimated bytes of the DDC / OLE / RLE encodings of one group (exact on the full data:
    the reference estimates them from a sample, CompressedSizeEstimatorSample)."""
    T, k = d.shape
    dict_b = T * k * d.element_size()
    zero = (d == 0).all(1)
    zid = int(torch.nonzero(zero)[0].item()) if bool(zero.any()) else -1
    nz = codes != zid if zid >= 0 else torch.ones_like(codes, dtype=torch.bool)
    nnz = int(nz.sum().item())
    change = torch.ones_like(codes, dtype=torch.bool)
    change[1:] = codes[1:] != codes[:-1]
    runs = int((change & nz).sum().item())
    ddc = n * torch.empty((), dtype=_code_dtype(T)).element_size() + dict_b
    ole = nnz * 4 + nnz * 2 + dict_b
    rle = runs * (4 + 4 + 2) + dict_b
    return {"ddc": ddc, "ole": ole, "rle": rle}, zid


def _make_group(kind, ci, d, codes, n, zid):
    if kind == "ddc":
        return ColGroup("ddc", ci, d.contiguous(), n, codes=codes.to(_code_dtype(d.shape[0])))
    # OLE / RLE: the all-zero tuple (if any) is implicit; renumber the remaining tuples
    keep = torch.ones(d.shape[0], dtype=torch.bool, device=d.device)
    if zid >= 0:
        keep[zid] = False
    newid = torch.cumsum(keep.long(), 0) - 1
    dd = d[keep].contiguous()
    tdt = torch.int16 if dd.shape[0] <= MAX_TUPLES else torch.int32
    nzmask = codes != zid if zid >= 0 else torch.ones_like(codes, dtype=torch.bool)
    if kind == "ole":
        rows = torch.nonzero(nzmask).flatten()
        tid = newid[codes[rows]]
        order = torch.argsort(tid, stable=True)           # offset lists grouped by tuple
        return ColGroup("ole", ci, dd, n, rows=rows[order].to(torch.int32), tid=tid[order].to(tdt))
    change = torch.ones_like(codes, dtype=torch.bool)
    change[1:] = codes[1:] != codes[:-1]
    bounds = torch.nonzero(change).flatten()
    lens = torch.diff(torch.cat([bounds, torch.tensor([n], device=codes.device)]))
    rcode = codes[bounds]
    nzr = rcode != zid if zid >= 0 else torch.ones_like(rcode, dtype=torch.bool)
    return ColGroup("rle", ci, dd, n, tid=newid[rcode[nzr]].to(tdt), starts=bounds[nzr].to(torch.int32),
                    lens=lens[nzr].to(torch.int32))


def compress(X: torch.Tensor, sample_rows=20000, force=False, kinds=None):
    """Compress a dense matrix; returns X itself when compression does not pay off.  `kinds`
    restricts the encodings the planner may choose (tests force OLE / RLE)."""
    allowed = tuple(kinds) if kinds else ("ddc", "ole", "rle")
    n, m = X.shape
    if n * m < MIN_CELLS and not force:
        return X
    Xc = X if X.dtype != torch.bfloat16 else X.float()
    # per-column distinct counts on a row sample (reference: compress/estim sampling estimators)
    if n > sample_rows:
        idx = torch.linspace(0, n - 1, sample_rows, device=X.device).long()
        S = Xc.index_select(0, idx)
    else:
        S = Xc
    distinct = [int(torch.unique(S[:, j]).numel()) for j in range(m)]
    cand = [j for j in range(m) if distinct[j] <= MAX_TUPLES_U8]
    others = [j for j in range(m) if distinct[j] > MAX_TUPLES_U8]
    # greedy co-coding: merge columns while the sample's joint tuple count stays small
    cand.sort(key=lambda j: distinct[j])
    plan = []
    cur = []
    for j in cand:
        trial = cur + [j]
        if cur and int(torch.unique(S[:, trial], dim=0).shape[0]) > MAX_TUPLES_U8:
            plan.append(cur)
            cur = [j]
        else:
            cur = trial
    if cur:
        plan.append(cur)
    groups = []
    for cols in plan:
        ci = torch.tensor(cols, dtype=torch.int64, device=X.device)
        d, codes = _encode(Xc.index_select(1, ci))
        if d.shape[0] > MAX_TUPLES:            # the sample under-estimated: keep dense
            others.extend(cols)
            continue
        sizes, zid = _sizes(d, codes, n)
        kind = min(allowed, key=lambda k_: sizes[k_])
        groups.append(_make_group(kind, ci, d, codes, n, zid))
    if others:
        ci = torch.tensor(sorted(others), dtype=torch.int64, device=X.device)
        groups.append(ColGroup("unc", ci, Xc.index_select(1, ci).contiguous(), n))
    cm = CompressedMatrix(n, m, groups, Xc.dtype, X.device)
    if not force and cm.nbytes() * 1.2 >= n * m * Xc.element_size():
        return X
    return cm
