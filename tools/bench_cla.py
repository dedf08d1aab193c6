"""Compressed linear algebra kernels (ops/hip/cla.hip) on directly built uint8 DDC groups:
X %*% v, t(X) %*% y and the XtXv chain, three ways on the same data --

  hip    the packed-DDC kernels (CompressedMatrix.matmul / tmatmul / mmchain);
  torch  the per-group torch operators on the same object (what SYSML_CLA=0 selects);
  dense  the dense row-streaming kernels (kernels.xv / xtg / mmchain) on the decompressed matrix.

Times are device-event times per call after warm-up; GB/s is the bytes of the packed code
matrix (n x Gp, read once by a product, once by the one-pass chain) over that time, for every
path, so the column compares the paths per byte of compressed data.  The LDS budget sweep
re-times the hip path with the budget of cla.hip set to 32 / 64 / 128 KiB.

    python tools/bench_cla.py [--rows 4000000] [--reps 20] [--out profiles/cla_kbench.txt]

--tsmm times instead the row-window decompression and the blocked t(X) %*% X built on it
(tsmm_rows below), with the sweep of the window's scratch budget:

    python tools/bench_cla.py --tsmm [--out profiles/cla_tsmm_kbench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from systemml_amd.ops import compress as CMP  # noqa: E402
from systemml_amd.ops import core, kernels  # noqa: E402
from systemml_amd.ops.backend import backend  # noqa: E402


def timed(f, reps, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def build(n, G, T, dtype, seed=0):
    """G two-column DDC groups of T tuples, built directly (no planner)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gs = []
    for j in range(G):
        codes = torch.randint(0, T, (n,), generator=gen, device="cuda").to(torch.uint8)
        d = torch.randn(T, 2, generator=gen, device="cuda", dtype=dtype)
        gs.append(CMP.ColGroup("ddc", torch.tensor([2 * j, 2 * j + 1], device="cuda"), d, n, codes=codes))
    return CMP.CompressedMatrix(n, 2 * G, gs, dtype, torch.device("cuda", torch.cuda.current_device()))


def ops(C, v, y):
    return (("X %*% v", lambda: C.matmul(v)), ("t(X) %*% y", lambda: C.tmatmul(y)),
            ("XtXv", lambda: core.mmchain("XtXv", C, v)))


def dense_ops(X, v, y):
    return (("X %*% v", lambda: kernels.xv(X, v)), ("t(X) %*% y", lambda: kernels.xtg(X, y)),
            ("XtXv", lambda: kernels.mmchain("XtXv", X, v)))


def tsmm_rows(a, say):
    """Full decompression and t(X) %*% X at the main shape (128 two-column groups, fp32):

      blocked  CompressedMatrix.tsmm: row windows of kernels._CLA_TSMM_SCRATCH bytes decompressed
               by cla.hip and multiplied by the MFMA tsmm, the dense matrix never allocated;
      parent   what core.tsmm did before: the per-group full decompression, then the dense tsmm
               (timed three times: their spread is the yardstick's noise);
      dense    the MFMA tsmm alone on an already decompressed matrix (the floor)."""
    dtype, G = torch.float32, 128
    C = build(a.rows, G, 64, dtype)
    C.pack()
    D = 2 * G
    dense_mb = a.rows * D * 4 / 2 ** 20
    reps = max(2, a.reps // 4)
    say(f"# rows {a.rows}, {G} two-column groups of 64 tuples, fp32: dense {dense_mb:.0f} MiB, "
        f"packed codes {a.rows * C.pack().Gp / 2 ** 20:.0f} MiB; {reps} timed calls after warm-up")
    default = kernels._CLA_TSMM_SCRATCH

    def per_group():
        kernels.CLA = False
        try:
            return C.decompress()
        finally:
            kernels.CLA = True

    th = timed(C.decompress, reps, warm=2)
    tt = timed(per_group, 2, warm=1)
    same = torch.equal(C.decompress(), per_group())
    say(f"{'op':>12s} {'hip ms':>9s} {'GB/s out':>9s} {'per-group ms':>13s} {'per-group/hip':>14s} {'equal bits':>10s}")
    say(f"{'decompress':>12s} {th:9.3f} {a.rows * D * 4 / th / 1e6:9.0f} {tt:13.3f} {tt / th:14.1f} {str(same):>10s}")

    tb = timed(C.tsmm, reps, warm=2)
    parent = [timed(lambda: kernels.try_tsmm(per_group(), True), 1, warm=1 if i == 0 else 0) for i in range(3)]
    X = C.decompress()
    td = timed(lambda: kernels.try_tsmm(X, True), reps, warm=2)
    ref = kernels.try_tsmm(X, True).double()
    diff = float(((C.tsmm().double() - ref).abs().max() / ref.abs().max()).item())
    del X, ref
    torch.cuda.empty_cache()
    say(f"{'op':>12s} {'blocked ms':>11s} {'parent ms (3 runs)':>27s} {'dense ms':>9s} {'parent/blocked':>14s} "
        f"{'max rel diff':>12s}")
    say(f"{'t(X) %*% X':>12s} {tb:11.3f} {' '.join(f'{t:8.3f}' for t in parent):>27s} {td:9.3f} "
        f"{min(parent) / tb:14.2f} {diff:12.2e}   (scratch {default >> 20} MiB)")
    say("# scratch sweep, blocked path (ms); peak MiB = allocated above the compressed matrix during the call")
    say(f"{'scratch MiB':>12s} {'blocks':>7s} {'ms':>9s} {'peak MiB':>9s}")
    one = a.rows * D * 4
    for scratch in [m << 20 for m in (32, 64, 128, 256, 512)] + [one]:
        kernels._CLA_TSMM_SCRATCH = scratch
        step = max(1, min(a.rows, scratch // (D * 4)))
        t = timed(C.tsmm, reps, warm=1)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        C.tsmm()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        label = "one block" if scratch == one else f"{scratch >> 20}"
        say(f"{label:>12s} {-(-a.rows // step):7d} {t:9.3f} {peak:9.0f}")
    kernels._CLA_TSMM_SCRATCH = default
    say(f"# default _CLA_TSMM_SCRATCH: {default >> 20} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tsmm", action="store_true",
                    help="the decompression and t(X) %%*%% X rows with the scratch sweep (profiles/cla_tsmm_kbench.txt)")
    ap.add_argument("--hip-only", action="store_true", help="tuning: skip the torch and dense columns")
    ap.add_argument("--bpc", type=int, default=0, help="tuning: workgroups per CU at most (0: built-in)")
    a = ap.parse_args()
    if a.bpc:
        kernels._CLA_BPC = a.bpc
    if not torch.cuda.is_available():
        raise SystemExit("bench_cla.py needs a GPU")
    L = kernels.load(required=True)
    backend.use_kernels = True
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    if a.tsmm:
        tsmm_rows(a, say)
        return save()
    dtype = torch.float32
    say(f"# rows {a.rows}, two-column groups of 64 tuples, fp32, {a.reps} timed calls after 3 warm-up calls")
    say(f"# LDS budget {L.sysml_cla_budget() // 1024} KiB, at most {kernels._CLA_BPC} workgroups per CU, "
        f"{L.sysml_cla_threads()} threads; GB/s = packed code bytes / time")
    say(f"{'groups':>6s} {'op':>11s} {'hip ms':>8s} {'GB/s':>7s} {'torch ms':>9s} {'GB/s':>7s} {'dense ms':>9s} "
        f"{'GB/s':>7s} {'torch/hip':>9s} {'max rel diff':>12s} {'counters':s}")
    for G in (128, 16, 512) + ((256,) if a.hip_only else ()):
        C = build(a.rows, G, 64, dtype)
        v = torch.randn(2 * G, 1, device="cuda", dtype=dtype)
        y = torch.randn(a.rows, 1, device="cuda", dtype=dtype)
        code_bytes = a.rows * C.pack().Gp
        X = None if a.hip_only else C.decompress()
        for (name, fh), (_, fd) in zip(ops(C, v, y), dense_ops(X, v, y)):
            before = dict(kernels.counters)
            kernels.CLA = True
            rh = fh()
            used = sorted(k for k, c in kernels.counters.items() if k.startswith("cla.") and c > before.get(k, 0))
            th = timed(fh, a.reps)
            if a.hip_only:
                say(f"{G:6d} {name:>11s} {th:8.3f} {code_bytes / th / 1e6:7.0f} {','.join(used)}")
                continue
            kernels.CLA = False
            rt = fh()
            tt = timed(fh, max(2, a.reps // 4), warm=1)
            kernels.CLA = True
            td = timed(fd, a.reps) if fd() is not None else float("nan")
            diff = float(((rh.double() - rt.double()).abs().max() / rt.double().abs().max()).item())
            say(f"{G:6d} {name:>11s} {th:8.3f} {code_bytes / th / 1e6:7.0f} {tt:9.3f} {code_bytes / tt / 1e6:7.0f} "
                f"{td:9.3f} {code_bytes / td / 1e6:7.0f} {tt / th:9.1f} {diff:12.2e} {','.join(used)}")
        del X
        if G in (128, 256):
            say(f"# LDS budget sweep, {G} groups, hip path (ms)")
            say(f"{'KiB':>6s} {'X %*% v':>9s} {'t(X) %*% y':>11s} {'XtXv':>9s} {'chain':>10s}")
            for kib in (32, 64, 128):
                L.sysml_cla_set_budget(kib * 1024)
                before = dict(kernels.counters)
                t3 = [timed(f, a.reps) for _, f in ops(C, v, y)]
                how = [k for k in ("cla.chain", "cla.chain2") if kernels.counters.get(k, 0) > before.get(k, 0)]
                say(f"{kib:6d} {t3[0]:9.3f} {t3[1]:11.3f} {t3[2]:9.3f} {','.join(how):>10s}")
            L.sysml_cla_set_budget(0)
        del C
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
