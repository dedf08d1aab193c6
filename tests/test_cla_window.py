"""Row windows of a compressed matrix on the host (ops/compress.py): decompress(r0, r1),
the blocked t(X) %*% X built on it, and right indexing that decompresses only its rows.

tsmm bound: with the fp64 host product of the decompressed matrix as the reference,
|got - ref| <= 2 n u (|X|^T |X|) elementwise, u = 2^-24 (fp32) or 2^-53 (fp64): the summation
bound gamma_n for any order of the n products of an entry, with a factor 2."""
import numpy as np
import pytest
import torch

from systemml_amd.api.executor import run
from systemml_amd.conf import DMLConfig
from systemml_amd.ops import compress as CMP
from systemml_amd.ops import core, kernels

from test_cla_gpu import ddc_groups, other_groups

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
DTYPES = [torch.float32, torch.float64]
LOOP = """
s = 0
for (i in 1:5) { Xb = X[((i-1)*1000+1):(i*1000), ]; s = s + sum(Xb %*% w) }
"""


def windows(n):
    return [(0, n)] + ([(1, n - 1)] if n > 2 else []) + [(n - 1, n)]


def tsmm_within(S, Xd, dtype, what):
    """Xd: the decompressed matrix in fp64 on the host."""
    n = Xd.shape[0]
    err = (S.detach().cpu().double() - Xd.t() @ Xd).abs()
    A = Xd.abs().t() @ Xd.abs()
    tol = 2 * n * U[dtype]
    worst = float((err / A.clamp_min(1e-300)).max())
    print(f"{what}: max |got - ref| / (|X|^T |X|) = {worst:.3e} (bound {tol:.3e})")
    assert S.shape == (Xd.shape[1], Xd.shape[1])
    assert bool((err <= tol * A).all()), (what, worst, tol)


def spy_on_decompress(monkeypatch):
    """Records the (r0, r1) of every CompressedMatrix.decompress call, r1 resolved."""
    calls = []
    inner = CMP.CompressedMatrix.decompress

    def spy(self, r0=0, r1=None):
        calls.append((r0, self.shape[0] if r1 is None else r1))
        return inner(self, r0, r1)
    monkeypatch.setattr(CMP.CompressedMatrix, "decompress", spy)
    return calls


def _data(n, seed=2):
    """Sparse flags (OLE), sorted runs (RLE), dense categories (DDC) and one column that does
    not compress (UNC)."""
    rng = np.random.default_rng(seed)
    flags = (rng.random((n, 3)) < 0.05) * rng.integers(1, 4, (n, 3))
    runs = np.sort(rng.integers(0, 6, (n, 2)), axis=0).astype(float)
    cat = rng.integers(1, 5, (n, 2)).astype(float)
    cont = rng.standard_normal((n, 1)) if n > 300 else np.arange(n, dtype=float).reshape(n, 1) / 7
    return torch.from_numpy(np.hstack([flags.astype(float), runs, cat, cont]))


def mixed(n, dtype):
    p0, p1, p2 = ddc_groups(n, [5, 40, 256], dtype, seed=21)
    unc, ole, rle, ddc16 = other_groups(n, dtype, seed=22, col0=6)
    return CMP.CompressedMatrix(n, 12, [p0, unc, p1, ole, rle, p2, ddc16], dtype, torch.device("cpu"))


@pytest.mark.parametrize("kinds", [("ddc",), ("ole",), ("rle",), None])
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_window_is_the_slice_of_the_full_matrix(n, kinds):
    X = _data(n)
    C = CMP.compress(X, force=True, kinds=kinds)
    assert CMP.is_compressed(C)
    if kinds is not None and n > 300:
        assert set(C.kinds()) == set(kinds) | {"unc"}, C.kinds()
    full = C.decompress()
    assert torch.equal(full, X)
    for r0, r1 in windows(n):
        w = C.decompress(r0, r1)
        assert w.shape == (r1 - r0, X.shape[1]) and torch.equal(w, full[r0:r1]), (r0, r1)
    assert C.decompress(n, n).shape == (0, X.shape[1])
    with pytest.raises(ValueError):
        C.decompress(0, n + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_of_every_group_kind(dtype):
    C = mixed(5000, dtype)
    assert C.kinds() == {"ddc": 4, "unc": 1, "ole": 1, "rle": 1}
    full = C.decompress()
    for r0, r1 in [(1000, 3500), (123, 4567), (4999, 5000)]:
        assert torch.equal(C.decompress(r0, r1), full[r0:r1]), (r0, r1)


def test_pack_tables_per_matrix_column():
    C = mixed(257, torch.float64)
    p = CMP._build_pack(C)
    assert [t.dtype for t in (p.mc_grp, p.mc_doff, p.mc_nc)] == [torch.int32] * 3
    assert p.mc_grp.tolist() == [0, 0, 1, 1, 2, 2] + [-1] * 6          # columns 6..11: the other groups
    for d in range(12):
        j = int(p.mc_grp[d])
        if j < 0:
            continue
        g = C.groups[p.index[j]]
        k = g.cols.tolist().index(d)
        assert int(p.mc_nc[d]) == g.cols.numel()
        o = int(p.mc_doff[d])
        assert torch.equal(p.dvals[o:o + g.dict.numel():g.cols.numel()], g.dict[:, k])
    q = p.with_dicts([g.with_dict(g.dict * 2) for g in C.groups])
    assert q.mc_grp is p.mc_grp and q.mc_doff is p.mc_doff and q.mc_nc is p.mc_nc


@pytest.mark.parametrize("dtype", DTYPES)
def test_tsmm_in_three_blocks(dtype, monkeypatch):
    n = 5000
    C = mixed(n, dtype)
    Xd = C.decompress().double()
    es = 4 if dtype == torch.float32 else 8
    monkeypatch.setattr(kernels, "_CLA_TSMM_SCRATCH", 2000 * 12 * es)      # blocks of 2000, 2000, 1000 rows
    seen = []
    inner = CMP.CompressedMatrix._window
    monkeypatch.setattr(CMP.CompressedMatrix, "_window",
                        lambda self, out, r0, r1, ordered=None: seen.append((r0, r1)) or inner(self, out, r0, r1, ordered))
    S = C.tsmm()
    assert seen == [(0, 2000), (2000, 4000), (4000, 5000)]
    assert S.dtype == dtype
    tsmm_within(S, Xd, dtype, "tsmm, 3 blocks")
    assert torch.equal(S, C.tsmm())
    monkeypatch.setattr(kernels, "_CLA_TSMM_SCRATCH", 1 << 30)
    tsmm_within(C.tsmm(), Xd, dtype, "tsmm, 1 block")


def test_core_tsmm_takes_the_blocked_path(monkeypatch):
    C = mixed(700, torch.float64)
    Xd = C.decompress()
    monkeypatch.setattr(kernels, "_CLA_TSMM_SCRATCH", 300 * 12 * 8)
    calls = spy_on_decompress(monkeypatch)
    S = core.tsmm(C)
    assert calls == []                                             # never the dense matrix
    tsmm_within(S, Xd, torch.float64, "core.tsmm")
    R = core.tsmm(C, left=False)                                   # X %*% t(X) keeps the full decompression
    assert calls == [(0, 700)]
    torch.testing.assert_close(R, Xd @ Xd.t())


def test_rix_of_a_compressed_matrix(monkeypatch):
    from systemml_amd.parser.errors import DMLRuntimeError
    C = mixed(700, torch.float64)
    Xd = C.decompress()
    calls = spy_on_decompress(monkeypatch)
    got = core.rix(C, 11, 20, 2, 5)
    assert calls == [(10, 20)]
    assert isinstance(got, torch.Tensor) and torch.equal(got, Xd[10:20, 1:5])
    assert torch.equal(core.rix(C, 700, 700, None, None), Xd[699:700])
    with pytest.raises(DMLRuntimeError):
        core.rix(C, 1, 701, 1, 12)


def minibatch_inputs():
    rng = np.random.default_rng(1)
    n = 80000
    X = np.hstack([rng.integers(0, 5, (n, 6)).astype(float), (rng.random((n, 4)) < 0.3).astype(float),
                   rng.standard_normal((n, 4))])                   # 1.12M cells: compress() keeps it
    return X, np.linspace(-1, 1, 14).reshape(-1, 1)


def test_minibatch_loop_decompresses_only_its_rows(monkeypatch):
    X, w = minibatch_inputs()
    ref = run(LOOP, inputs={"X": X, "w": w}, outputs=["s"], config=DMLConfig(gpu=False), out=lambda s: None)
    calls = spy_on_decompress(monkeypatch)
    got = run(LOOP, inputs={"X": X, "w": w}, outputs=["s", "X"],
              config=DMLConfig(gpu=False, compressed_linalg="true"), out=lambda s: None)
    assert CMP.is_compressed(got["X"])
    assert [c for c in calls if c[1] - c[0] <= 1000] == [(1000 * i, 1000 * i + 1000) for i in range(5)], calls
    assert all(r1 - r0 <= 1000 for r0, r1 in calls), calls
    np.testing.assert_allclose(float(got["s"]), float(ref["s"]), rtol=1e-10)
    assert abs(float(ref["s"]) - float((X[:5000] @ w).sum())) <= 1e-9 * np.abs(X[:5000] @ w).sum()
