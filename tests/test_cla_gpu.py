"""Compressed linear algebra on the HIP kernels of ops/hip/cla.hip: X %*% V, t(X) %*% Y and the
mmchains of matrices whose uint8 DDC groups are packed (ops/compress.CLAPack).

The reference is the fp64 product with the decompressed matrix, computed on the host from the
same dtype-rounded inputs.  Bounds: with A = |X| |V| (|X|^T |Y|; for a chain
|X|^T (|w| * (|X| |v|)), plus |y| inside for XtXvy), |got - ref| <= tol * A elementwise;
fp64 tol = 1e-11 (at most ~1000 fp64 additions per entry: ~1e-13, margin 100x), fp32
tol = 1e-6 (one fp32 rounding of the product table and one of the output around an fp64
accumulation: ~1.2e-7, margin 8x)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from systemml_amd.ops import compress as CMP
from systemml_amd.ops import core, kernels
from systemml_amd.ops.backend import backend

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-6, torch.float64: 1e-11}
DTYPES = [torch.float32, torch.float64]
CHAINS = ["XtXv", "XtwXv", "XtXvy"]


@pytest.fixture(autouse=True)
def _hip_kernels():
    kernels.load(required=True)
    old = backend.use_kernels
    backend.use_kernels = True
    yield
    backend.use_kernels = old


# ---------------------------------------------------------------------------- construction
def ddc_groups(n, Ts, dtype, seed, col0=0, ncols=2):
    """uint8 DDC groups built directly, on the host: seeded dictionaries and codes, with
    codes[0] = T_g - 1 and codes[1] = 0 in every group."""
    gen = torch.Generator().manual_seed(seed)
    gs, col = [], col0
    for T in Ts:
        codes = torch.randint(0, T, (n,), generator=gen).to(torch.uint8)
        codes[0] = T - 1
        if n > 1:
            codes[1] = 0
        d = torch.randn(T, ncols, generator=gen, dtype=torch.float64).to(dtype)
        gs.append(CMP.ColGroup("ddc", torch.arange(col, col + ncols), d, n, codes=codes))
        col += ncols
    return gs


def other_groups(n, dtype, seed, col0):
    """One UNC, one OLE, one RLE and one int16 DDC group (T_g = 300)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    gs = [CMP.ColGroup("unc", torch.tensor([col0]), rnd(n, 1), n)]
    d = rnd(4, 2)
    d[0] = 0                                                       # the implicit all-zero tuple
    sparse = torch.randint(0, 4, (n,), generator=gen) * (torch.rand(n, generator=gen) < 0.1)
    gs.append(CMP._make_group("ole", torch.tensor([col0 + 1, col0 + 2]), d, sparse, n, 0))
    runs = torch.sort(torch.randint(0, 4, (n,), generator=gen)).values
    gs.append(CMP._make_group("rle", torch.tensor([col0 + 3, col0 + 4]), d.clone(), runs, n, 0))
    wide = torch.randint(0, 300, (n,), generator=gen).to(torch.int16)
    gs.append(CMP.ColGroup("ddc", torch.tensor([col0 + 5]), rnd(300, 1), n, codes=wide))
    return gs


def matrix(groups, n, dtype):
    """(the compressed matrix in HBM, its decompressed fp64 host copy)."""
    D = sum(int(g.cols.numel()) for g in groups)
    Xd = CMP.CompressedMatrix(n, D, groups, dtype, torch.device("cpu")).decompress().double()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda t: None if t is None else t.to(dev)
    gg = [CMP.ColGroup(g.kind, up(g.cols), up(g.dict), n, up(g.codes), up(g.rows), up(g.tid), up(g.starts),
                       up(g.lens)) for g in groups]
    return CMP.CompressedMatrix(n, D, gg, dtype, dev), Xd


def rand(shape, dtype, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


# ---------------------------------------------------------------------------- checks
def within(got, ref, A, dtype, what):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    worst = float((err / A.clamp_min(1e-300)).max())
    print(f"{what}: max |got - ref| / A = {worst:.3e} (tol {TOL[dtype]:g})")
    assert bool((err <= TOL[dtype] * A).all()), (what, worst)


def grew(before, name):
    return kernels.counters.get(name, 0) - before.get(name, 0)


def check_matmul(C, Xd, K, dtype, seed=11):
    V = rand((Xd.shape[1], K), dtype, seed)
    within(C.matmul(V.cuda()), Xd @ V.double(), Xd.abs() @ V.double().abs(), dtype, f"matmul K={K}")


def check_tmatmul(C, Xd, K, dtype, seed=12):
    Y = rand((Xd.shape[0], K), dtype, seed)
    within(C.tmatmul(Y.cuda()), Xd.t() @ Y.double(), Xd.abs().t() @ Y.double().abs(), dtype, f"tmatmul K={K}")


def check_chain(C, Xd, ctype, dtype, seed=13):
    v = rand((Xd.shape[1], 1), dtype, seed)
    w = None if ctype == "XtXv" else rand((Xd.shape[0], 1), dtype, seed + 1)
    v64, w64 = v.double(), None if w is None else w.double()
    ref = core.mmchain_ref(ctype, Xd, v64, w64)
    assert ref.dtype == torch.float64 and not ref.is_cuda
    au = Xd.abs() @ v64.abs()
    if ctype == "XtwXv":
        au = w64.abs() * au
    elif ctype == "XtXvy":
        au = au + w64.abs()
    got = core.mmchain(ctype, C, v.cuda(), None if w is None else w.cuda())
    within(got, ref, Xd.abs().t() @ au, dtype, f"mmchain {ctype}")


def check_all(C, Xd, dtype, K=1, chains=("XtXv",)):
    before = dict(kernels.counters)
    check_matmul(C, Xd, K, dtype)
    check_tmatmul(C, Xd, K, dtype)
    for ctype in chains:
        check_chain(C, Xd, ctype, dtype)
    assert grew(before, "cla.rmm") == 1 and grew(before, "cla.lmm") == 1, kernels.counters
    assert grew(before, "cla.chain") + grew(before, "cla.chain2") == len(chains), kernels.counters


# ---------------------------------------------------------------------------- cases
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_row_edges(n, dtype):
    C, Xd = matrix(ddc_groups(n, [1, 2, 7], dtype, seed=n), n, dtype)
    check_all(C, Xd, dtype, K=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 15, 16, 17, 40])
def test_group_padding(G, dtype):
    C, Xd = matrix(ddc_groups(5000, [5] * G, dtype, seed=G), 5000, dtype)
    assert C.pack().Gp == 16 * ((G + 15) // 16)
    check_all(C, Xd, dtype, K=1, chains=CHAINS if G == 17 else ("XtXv",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_code_range(dtype):
    """T_g = 256: code 255 is the last tuple, not -1."""
    C, Xd = matrix(ddc_groups(5000, [256, 256], dtype, seed=3), 5000, dtype)
    assert int(C.pack().codes[0, 0]) == 255
    check_all(C, Xd, dtype, K=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 3, 8])
def test_columns(K, dtype):
    C, Xd = matrix(ddc_groups(5000, [5] * 17, dtype, seed=K), 5000, dtype)
    before = dict(kernels.counters)
    check_matmul(C, Xd, K, dtype)
    check_tmatmul(C, Xd, K, dtype)
    assert grew(before, "cla.rmm") == 1 and grew(before, "cla.lmm") == 1, kernels.counters


@pytest.mark.parametrize("dtype", DTYPES)
def test_nine_columns_stay_on_torch(dtype):
    C, Xd = matrix(ddc_groups(5000, [5] * 17, dtype, seed=9), 5000, dtype)
    before = dict(kernels.counters)
    check_matmul(C, Xd, 9, dtype)
    check_tmatmul(C, Xd, 9, dtype)
    assert kernels.counters == before


@pytest.mark.parametrize("dtype", DTYPES)
def test_lmm_forced_chunking(dtype):
    """G = 48, T_g = 256, K = 4: 393 KB of fp64 bins, more than a CU's 160 KiB of LDS, so the
    launch is split into at least 3 chunks of groups at any budget; one operator call."""
    C, Xd = matrix(ddc_groups(5000, [256] * 48, dtype, seed=48), 5000, dtype)
    p = C.pack()
    gpc, lds = kernels._cla_chunks(kernels.load(required=True), p, 4)
    assert -(-p.Gp // gpc) >= 3 and lds <= 160 * 1024
    before = dict(kernels.counters)
    check_tmatmul(C, Xd, 4, dtype)
    assert grew(before, "cla.lmm") == 1, kernels.counters


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ctype", CHAINS)
def test_chain_fused(ctype, dtype):
    """G = 16, T_g = 10: table and bins are 2.5 KB, one pass over the codes."""
    C, Xd = matrix(ddc_groups(5000, [10] * 16, dtype, seed=16), 5000, dtype)
    before = dict(kernels.counters)
    check_chain(C, Xd, ctype, dtype)
    assert grew(before, "cla.chain") == 1 and grew(before, "cla.chain2") == 0, kernels.counters


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ctype", CHAINS)
def test_chain_split(ctype, dtype):
    """G = 48, T_g = 256: table plus bins exceed a CU's LDS, so gather and binning are two passes."""
    C, Xd = matrix(ddc_groups(5000, [256] * 48, dtype, seed=49), 5000, dtype)
    before = dict(kernels.counters)
    check_chain(C, Xd, ctype, dtype)
    assert grew(before, "cla.chain2") == 1 and grew(before, "cla.chain") == 0, kernels.counters


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_matrix(dtype):
    """Packed groups beside UNC, OLE, RLE and int16 DDC groups: the other groups' products
    enter as u0 and use the written g of the chain."""
    n = 5000
    p0, p1, p2 = ddc_groups(n, [5, 40, 256], dtype, seed=21)       # columns 0..5
    unc, ole, rle, ddc16 = other_groups(n, dtype, seed=22, col0=6)  # columns 6..11
    C, Xd = matrix([p0, unc, p1, ole, rle, p2, ddc16], n, dtype)   # packed groups are not adjacent
    assert C.kinds() == {"ddc": 4, "unc": 1, "ole": 1, "rle": 1} and C.pack().G == 3
    check_all(C, Xd, dtype, K=3, chains=CHAINS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaled_matrix_shares_the_codes(dtype):
    C, Xd = matrix(ddc_groups(5000, [5] * 17, dtype, seed=5), 5000, dtype)
    S = C.scale(2.0)
    p, q = C.pack(), S.pack()
    assert q is not p and q.codes.data_ptr() == p.codes.data_ptr() and q.toff.data_ptr() == p.toff.data_ptr()
    check_all(S, 2.0 * Xd, dtype, K=3)


# ---------------------------------------------------------------------------- SYSML_CLA=0
def _child():
    """Run in a fresh process: every operator on a mixed matrix, then the counters."""
    backend.use_kernels = True
    kernels.load(required=True)
    for dtype in DTYPES:
        gs = ddc_groups(5000, [5] * 17, dtype, seed=31) + other_groups(5000, dtype, seed=32, col0=34)
        C, Xd = matrix(gs, 5000, dtype)
        check_matmul(C, Xd, 3, dtype)
        check_tmatmul(C, Xd, 3, dtype)
        for ctype in CHAINS:
            check_chain(C, Xd, ctype, dtype)
    print("COUNTERS", sorted(k for k in kernels.counters if k.startswith("cla.")))


def test_switch_off_in_a_fresh_process():
    env = dict(os.environ, SYSML_CLA="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_cla_gpu as t; t._child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "COUNTERS []" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------- end to end
def test_linreg_cg_end_to_end():
    """LinearRegCG on compressed X in HBM: beta matches the dense host run, and the solver's
    t(X) %*% (X %*% p) ran on the compressed chain (two incompressible columns: the other
    groups are on its path too)."""
    from systemml_amd.api.executor import run
    from systemml_amd.api.mlcontext import SCRIPTS_DIR
    from systemml_amd.conf import DMLConfig
    rng = np.random.default_rng(1)
    n = 80000
    cat = rng.integers(0, 5, (n, 6)).astype(float)                 # tests/test_compress.py _data(80000, 1)
    flags = (rng.random((n, 4)) < 0.3).astype(float)
    cont = rng.standard_normal((n, 2))
    X = np.hstack([cat, flags, cont, cat[:, :2] * 2 + 1])
    y = X @ np.linspace(-1, 1, X.shape[1]).reshape(-1, 1) + 0.01
    src = open(f"{SCRIPTS_DIR}/algorithms/LinearRegCG.dml").read()
    args = dict(X="X", Y="y", B="B", icpt=0, reg=1e-6, tol=1e-12, maxi=100)
    try:
        r1 = run(src, args=args, inputs={"X": X, "y": y}, outputs=["beta"], config=DMLConfig(gpu=False),
                 out=lambda s: None)
        before = dict(kernels.counters)
        r2 = run(src, args=args, inputs={"X": X, "y": y}, outputs=["beta"],
                 config=DMLConfig(gpu=True, compressed_linalg="true"), out=lambda s: None)
        b1, b2 = r1["beta"], r2["beta"]
        np.testing.assert_allclose(b2.cpu().numpy(), b1.cpu().numpy(), rtol=1e-8, atol=1e-10)
        assert grew(before, "cla.chain") + grew(before, "cla.chain2") > 0, kernels.counters
    finally:
        backend.configure(DMLConfig(gpu=False))
