"""Row-window decompression of the packed uint8 DDC groups on ops/hip/cla.hip (decomp_kernel),
and what is built on it: CompressedMatrix.decompress(r0, r1), the blocked t(X) %*% X that never
holds the dense matrix, and right indexing of a compressed matrix.

Windows are compared bit for bit with the rows of the host decompression: the kernel only
copies dictionary values.  tsmm: with the fp64 host product of the decompressed matrix as the
reference, |got - ref| <= 2 n u (|X|^T |X|) elementwise, u = 2^-24 (fp32) or 2^-53 (fp64) -- the
summation bound gamma_n for any order of an entry's n products, with a factor 2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from systemml_amd.ops import compress as CMP
from systemml_amd.ops import core, kernels
from systemml_amd.ops.backend import backend

from test_cla_gpu import ddc_groups, grew, matrix, other_groups
from test_cla_window import LOOP, minibatch_inputs, spy_on_decompress, tsmm_within, windows

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


@pytest.fixture(autouse=True)
def _hip_kernels():
    kernels.load(required=True)
    old = backend.use_kernels
    backend.use_kernels = True
    yield
    backend.use_kernels = old


def host_rows(C):
    """The host decompression of the same groups, in the matrix dtype (bit-exact reference)."""
    down = lambda t: None if t is None else t.cpu()
    gg = [CMP.ColGroup(g.kind, down(g.cols), down(g.dict), g.nrows, down(g.codes), down(g.rows), down(g.tid),
                       down(g.starts), down(g.lens)) for g in C.groups]
    return CMP.CompressedMatrix(C.shape[0], C.shape[1], gg, C.dtype, torch.device("cpu")).decompress()


def check_window(C, full, r0, r1):
    before = dict(kernels.counters)
    w = C.decompress(r0, r1)
    assert grew(before, "cla.decompress") == 1, kernels.counters
    assert w.is_cuda and w.dtype == C.dtype and w.shape == (r1 - r0, C.shape[1])
    assert torch.equal(w.cpu(), full[r0:r1]), (r0, r1)


def mixed(n, dtype):
    p0, p1, p2 = ddc_groups(n, [5, 40, 256], dtype, seed=21)       # columns 0..5
    unc, ole, rle, ddc16 = other_groups(n, dtype, seed=22, col0=6)  # columns 6..11
    return matrix([p0, unc, p1, ole, rle, p2, ddc16], n, dtype)


# ---------------------------------------------------------------------------- windows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_window_row_edges(n, dtype):
    C, _ = matrix(ddc_groups(n, [1, 2, 7], dtype, seed=n), n, dtype)
    full = host_rows(C)
    for r0, r1 in windows(n):
        check_window(C, full, r0, r1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 15, 16, 17, 40])
def test_window_group_padding(G, dtype):
    C, _ = matrix(ddc_groups(5000, [5] * G, dtype, seed=G), 5000, dtype)
    check_window(C, host_rows(C), 123, 4567)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_full_code_range(dtype):
    """T_g = 256 in two groups: code 255 is the last tuple."""
    C, _ = matrix(ddc_groups(5000, [256, 256], dtype, seed=3), 5000, dtype)
    assert int(C.pack().codes[0, 0]) == 255
    full = host_rows(C)
    check_window(C, full, 0, 5000)
    check_window(C, full, 123, 4567)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,ncols", [(3, 1), (16, 2)])
def test_store_variants(G, ncols, dtype):
    """D = 3: rows of 12 / 24 bytes take the scalar stores; D = 32: the 16-byte stores."""
    C, _ = matrix(ddc_groups(5000, [5] * G, dtype, seed=G, ncols=ncols), 5000, dtype)
    assert C.shape[1] == G * ncols
    full = host_rows(C)
    check_window(C, full, 0, 5000)
    check_window(C, full, 123, 4567)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width,col0", [(37, 1), (36, 1), (40, 4)])
def test_pitch_and_alignment(width, col0, dtype):
    """kernels.cla_decompress into a column window of a wider buffer: an odd pitch from a base
    that is not 16-byte aligned, a 16-byte pitch from such a base (both scalar stores), and an
    aligned window with a pitch (16-byte stores).  The cells around the window are left alone."""
    C, _ = matrix(ddc_groups(5000, [5] * 16, dtype, seed=7), 5000, dtype)
    full = host_rows(C)
    r0, r1, D = 123, 4567, 32
    buf = torch.full((r1 - r0, width), -7.0, dtype=dtype, device="cuda")
    out = buf[:, col0:col0 + D]
    assert (out.data_ptr() % 16 == 0) == (col0 == 4) and out.stride(0) == width
    before = dict(kernels.counters)
    assert kernels.cla_decompress(C.pack(), r0, r1, out) is out
    assert grew(before, "cla.decompress") == 1
    got = buf.cpu()
    assert torch.equal(got[:, col0:col0 + D], full[r0:r1])
    assert bool((got[:, :col0] == -7.0).all()) and bool((got[:, col0 + D:] == -7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_decompress_declines(dtype):
    """A host tensor, another dtype or a wrong shape: None, and nothing is written or counted."""
    C, _ = matrix(ddc_groups(100, [5] * 3, dtype, seed=1), 100, dtype)
    p = C.pack()
    before = dict(kernels.counters)
    assert kernels.cla_decompress(p, 0, 10, torch.zeros(10, 6, dtype=dtype)) is None
    other = torch.float64 if dtype == torch.float32 else torch.float32
    assert kernels.cla_decompress(p, 0, 10, torch.zeros(10, 6, dtype=other, device="cuda")) is None
    assert kernels.cla_decompress(p, 0, 10, torch.zeros(10, 6, dtype=torch.float16, device="cuda")) is None
    assert kernels.cla_decompress(p, 0, 10, torch.zeros(9, 6, dtype=dtype, device="cuda")) is None
    assert kernels.cla_decompress(p, 95, 101, torch.zeros(6, 6, dtype=dtype, device="cuda")) is None
    assert kernels.counters == before


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [256, 5])
def test_dictionary_beyond_the_lds_budget(T, dtype):
    """48 groups x 256 tuples x 2 columns: 196 KB in fp64, more than the 128 KiB budget, so the
    dictionaries are read through the cache; with 5 tuples they are staged in LDS."""
    C, _ = matrix(ddc_groups(5000, [T] * 48, dtype, seed=48), 5000, dtype)
    nbytes = C.pack().dvals.numel() * C.pack().dvals.element_size()
    budget = kernels.load(required=True).sysml_cla_budget()
    assert (nbytes > budget) == (T == 256 and dtype == torch.float64)
    full = host_rows(C)
    check_window(C, full, 0, 5000)
    check_window(C, full, 123, 4567)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_of_a_mixed_matrix(dtype):
    """Packed groups between UNC, OLE, RLE and int16 DDC groups."""
    C, Xd = mixed(5000, dtype)
    assert C.kinds() == {"ddc": 4, "unc": 1, "ole": 1, "rle": 1} and C.pack().G == 3
    full = host_rows(C)
    assert torch.equal(full.double(), Xd)
    check_window(C, full, 1000, 3500)
    check_window(C, full, 4999, 5000)
    before = dict(kernels.counters)
    assert torch.equal(C.decompress().cpu(), full)
    assert grew(before, "cla.decompress") == 1


# ---------------------------------------------------------------------------- tsmm
def check_tsmm(C, Xd, dtype, monkeypatch, step, what):
    n, D = C.shape
    es = 4 if dtype == torch.float32 else 8
    monkeypatch.setattr(kernels, "_CLA_TSMM_SCRATCH", step * D * es)
    blocks = -(-n // step)
    before = dict(kernels.counters)
    S = C.tsmm()
    assert grew(before, "cla.tsmm") == 1 and grew(before, "cla.decompress") == blocks, kernels.counters
    assert S.is_cuda and S.dtype == dtype
    tsmm_within(S, Xd, dtype, f"{what}, {blocks} block(s)")
    assert torch.equal(S, S.t())
    assert torch.equal(S, C.tsmm())
    return S


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["packed", "mixed"])
def test_tsmm_blocks(which, dtype, monkeypatch):
    n = 5000
    C, Xd = matrix(ddc_groups(n, [5] * 17, dtype, seed=17), n, dtype) if which == "packed" else mixed(n, dtype)
    check_tsmm(C, Xd, dtype, monkeypatch, 2000, which)             # 2000 + 2000 + 1000 rows
    check_tsmm(C, Xd, dtype, monkeypatch, 1 << 20, which)          # one block
    before = dict(kernels.counters)
    within = core.tsmm(C)
    assert grew(before, "cla.tsmm") == 1
    tsmm_within(within, Xd, dtype, "core.tsmm")


def test_tsmm_holds_no_dense_copy(monkeypatch):
    """n = 200000, D = 64, fp32: the dense matrix is 51.2 MB, the codes 6.4 MB.  With 4 MiB of
    scratch (13 blocks, the last of 3392 rows) the call allocates the window plus at most 4 MiB
    of split-K slab: the peak stays below 25.6 MB, half the dense matrix."""
    n, dtype = 200000, torch.float32
    C, Xd = matrix(ddc_groups(n, [5] * 32, dtype, seed=32), n, dtype)
    C.pack()                                                       # the codes are part of the matrix
    monkeypatch.setattr(kernels, "_CLA_TSMM_SCRATCH", 4 << 20)
    torch.cuda.synchronize()
    before = dict(kernels.counters)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    S = C.tsmm()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"tsmm of {n} x 64 fp32 with 4 MiB of scratch: peak {peak / 1e6:.1f} MB above the matrix")
    assert grew(before, "cla.decompress") == 13 and n - 12 * 16384 == 3392
    assert peak < 25.6e6, peak
    tsmm_within(S, Xd, dtype, "tsmm, 13 blocks")


# ---------------------------------------------------------------------------- right indexing
@pytest.mark.parametrize("dtype", DTYPES)
def test_rix_window(dtype):
    C, _ = mixed(5000, dtype)
    full = host_rows(C)
    before = dict(kernels.counters)
    got = core.rix(C, 11, 20, 2, 5)
    assert grew(before, "cla.decompress") == 1
    assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got.cpu(), full[10:20, 1:5])


def test_minibatch_loop_in_hbm(monkeypatch):
    from systemml_amd.api.executor import run
    from systemml_amd.conf import DMLConfig
    X, w = minibatch_inputs()
    try:
        ref = run(LOOP, inputs={"X": X, "w": w}, outputs=["s"], config=DMLConfig(gpu=False), out=lambda s: None)
        calls = spy_on_decompress(monkeypatch)
        before = dict(kernels.counters)
        got = run(LOOP, inputs={"X": X, "w": w}, outputs=["s", "X"],
                  config=DMLConfig(gpu=True, compressed_linalg="true"), out=lambda s: None)
        assert CMP.is_compressed(got["X"]) and torch.device(got["X"].device).type == "cuda"
        assert calls == [(1000 * i, 1000 * i + 1000) for i in range(5)], calls
        assert grew(before, "cla.decompress") == 5, kernels.counters
        np.testing.assert_allclose(float(got["s"]), float(ref["s"]), rtol=1e-10)
    finally:
        backend.configure(DMLConfig(gpu=False))


# ---------------------------------------------------------------------------- SYSML_CLA=0
def _child():
    """Run in a fresh process: window, tsmm and rix on a mixed matrix, then the counters."""
    backend.use_kernels = True
    kernels.load(required=True)
    for dtype in DTYPES:
        C, Xd = mixed(5000, dtype)
        full = host_rows(C)
        assert torch.equal(C.decompress(1000, 3500).cpu(), full[1000:3500])
        assert torch.equal(C.decompress().cpu(), full)
        assert torch.equal(core.rix(C, 11, 20, 2, 5).cpu(), full[10:20, 1:5])
        kernels._CLA_TSMM_SCRATCH = 2000 * 12 * (4 if dtype == torch.float32 else 8)
        S = core.tsmm(C)
        tsmm_within(S, Xd, dtype, "tsmm with the kernels off, 3 blocks")
        assert torch.equal(S, S.t()) and torch.equal(S, C.tsmm())
    print("COUNTERS", sorted(k for k in kernels.counters if k.startswith("cla.")))


def test_switch_off_in_a_fresh_process():
    env = dict(os.environ, SYSML_CLA="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_cla_tsmm_gpu as t; "
            "t._child()")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "COUNTERS []" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------- end to end
def test_linreg_ds_end_to_end():
    """LinearRegDS on compressed X in HBM against the dense host run.  1.2M cells: compress keeps
    it (three uint8 DDC groups and one UNC group); cond(t(X) X + reg I) = 126, and a perturbation
    of t(X) X at the fp64 tsmm bound (2.3e-11 |X|^T |X|) moves beta by at most 1.5e-10, so 2e-9
    absolute (beta's entries are 0.09 .. 1) is about 10x that."""
    from systemml_amd.api.executor import run
    from systemml_amd.api.mlcontext import SCRIPTS_DIR
    from systemml_amd.conf import DMLConfig
    rng = np.random.default_rng(1)
    n = 100000
    X = np.hstack([rng.integers(0, 5, (n, 6)), rng.random((n, 4)) < 0.3, rng.standard_normal((n, 2))]).astype(float)
    y = X @ np.linspace(-1, 1, 12)[:, None] + 0.01
    src = open(f"{SCRIPTS_DIR}/algorithms/LinearRegDS.dml").read()
    args = dict(X="X", Y="y", B="B", icpt=0, reg=1e-6)
    try:
        r1 = run(src, args=args, inputs={"X": X, "y": y}, outputs=["beta"], config=DMLConfig(gpu=False),
                 out=lambda s: None)
        before = dict(kernels.counters)
        r2 = run(src, args=args, inputs={"X": X, "y": y}, outputs=["beta", "X"],
                 config=DMLConfig(gpu=True, compressed_linalg="true"), out=lambda s: None)
        assert CMP.is_compressed(r2["X"]), type(r2["X"])
        b1, b2 = r1["beta"].cpu().double().numpy(), r2["beta"].cpu().double().numpy()
        print(f"LinearRegDS: max |beta_gpu - beta_host| = {np.abs(b2 - b1).max():.3e} (bound 2e-9)")
        assert np.abs(b2 - b1).max() <= 2e-9
        assert grew(before, "cla.tsmm") > 0, kernels.counters
    finally:
        backend.configure(DMLConfig(gpu=False))
