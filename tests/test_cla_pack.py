"""The packed layout of the uint8 DDC groups (ops/compress.CLAPack, the operand of
ops/hip/cla.hip), built on host tensors: the pack is plain tensor code."""
import pytest
import torch

from systemml_amd.ops import compress as CMP


def _matrix(G, n=257, T=5, seed=0, dtype=torch.float64, extra=()):
    """G two-column uint8 DDC groups with T tuples each (+ extra groups), built directly."""
    gen = torch.Generator().manual_seed(seed)
    groups, col = [], 0
    for _ in range(G):
        codes = torch.randint(0, T, (n,), generator=gen).to(torch.uint8)
        codes[0], codes[1] = T - 1, 0
        cols = torch.tensor([col, col + 1])
        groups.append(CMP.ColGroup("ddc", cols, torch.randn(T, 2, generator=gen, dtype=dtype), n, codes=codes))
        col += 2
    for kind in extra:
        if kind == "unc":
            groups.append(CMP.ColGroup("unc", torch.tensor([col]), torch.randn(n, 1, generator=gen, dtype=dtype), n))
        elif kind == "ddc16":
            codes = torch.randint(0, 300, (n,), generator=gen).to(torch.int16)
            groups.append(CMP.ColGroup("ddc", torch.tensor([col]), torch.randn(300, 1, generator=gen, dtype=dtype), n,
                                       codes=codes))
        col += 1
    return CMP.CompressedMatrix(n, col, groups, dtype, torch.device("cpu"))


def _packed(C):
    C._pack = CMP._build_pack(C)
    return C._pack


@pytest.mark.parametrize("G", [1, 15, 16, 17])
def test_padding_and_offsets(G):
    C = _matrix(G)
    p = _packed(C)
    Gp = 16 * ((G + 15) // 16)
    assert (p.G, p.Gp) == (G, Gp) and p.codes.shape == (257, Gp) and p.codes.dtype == torch.uint8
    assert p.codes.is_contiguous() and p.valid
    assert not p.codes[:, G:].any()                                # padding columns hold code 0
    toff = p.toff.tolist()
    assert toff == p.toff_host and len(toff) == Gp
    assert toff[:G] == [5 * j for j in range(G)]                   # monotone, tuple 0 of each group
    assert p.T == 5 * G and toff[G - 1] + 5 == p.T
    assert toff[G:] == [p.T] * (Gp - G)                            # padding points at the extra row
    for j, g in enumerate(C.groups):
        assert g.codes.data_ptr() == p.codes[:, j].data_ptr()      # codes stored once
        assert torch.equal(p.codes[:, j], g.codes)


def test_flat_dictionaries():
    C = _matrix(3, extra=("unc",))
    p = _packed(C)
    assert p.index == [0, 1, 2] and p.C == 6
    for t in range(p.T):
        g, r = divmod(t, 5)
        o, nc, c0 = int(p.tup_off[t]), int(p.tup_nc[t]), int(p.tup_c0[t])
        assert torch.equal(p.dvals[o:o + nc], C.groups[g].dict[r])
        assert torch.equal(p.colidx[c0:c0 + nc].long(), C.groups[g].cols)
    for c in range(p.C):
        g, j = divmod(c, 2)
        assert int(p.col_out[c]) == int(C.groups[g].cols[j])
        assert (int(p.col_t0[c]), int(p.col_T[c]), int(p.col_nc[c])) == (5 * g, 5, 2)
        o = int(p.col_doff[c])
        assert torch.equal(p.dvals[o:o + 10:2], C.groups[g].dict[:, j])


@pytest.mark.parametrize("G", [1, 17])
def test_operators_unchanged_by_packing(G):
    C = _matrix(G, extra=("unc", "ddc16"))
    V = torch.randn(C.shape[1], 3, dtype=torch.float64)
    Y = torch.randn(C.shape[0], 2, dtype=torch.float64)
    before = (C.decompress(), C.matmul(V), C.tmatmul(Y), C.colsums(), C.rowsums(sq=True), C.nbytes())
    p = _packed(C)
    assert p.index == list(range(G))                               # the int16 DDC group is not packed
    after = (C.decompress(), C.matmul(V), C.tmatmul(Y), C.colsums(), C.rowsums(sq=True))
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert C.nbytes() == before[5] + C.shape[0] * (p.Gp - G)       # exactly the padding columns


def test_no_group_qualifies():
    C = _matrix(0, extra=("unc", "ddc16"))
    assert CMP._build_pack(C) is None
    assert C.pack() is None                                        # host matrices are never packed
    assert _matrix(3).pack() is None


def test_out_of_range_code_makes_pack_unusable():
    C = _matrix(3)
    C.groups[1].codes[7] = 5                                       # T_g = 5: codes are 0..4
    p = _packed(C)
    assert p is not None and not p.valid
    V = torch.randn(C.shape[1], 1, dtype=torch.float64)
    assert C._cla(1) is None and C.mmchain("XtXv", V) is None


def test_scale_shares_codes():
    C = _matrix(17)
    p = _packed(C)
    S = C.scale(2.0)
    q = S._pack
    assert q is not p and q.codes.data_ptr() == p.codes.data_ptr() and q.toff.data_ptr() == p.toff.data_ptr()
    assert torch.equal(q.dvals, 2.0 * p.dvals) and q.valid
    assert S.groups[3].codes.data_ptr() == p.codes[:, 3].data_ptr()
    assert torch.equal(S.decompress(), 2.0 * C.decompress())
    assert S.nbytes() == C.nbytes()


def test_host_mmchain_is_not_taken():
    """On the CPU a compressed X keeps today's path: the method declines, core composes."""
    from systemml_amd.ops import core
    C = _matrix(3)
    X = C.decompress()
    v = torch.randn(C.shape[1], 1, dtype=torch.float64)
    assert C.mmchain("XtXv", v) is None
    torch.testing.assert_close(core.mmchain("XtXv", C, v), X.t() @ (X @ v))
