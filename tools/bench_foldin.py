"""Fold-in throughput (qmfx_wals_fold_in) beside the half-epoch that solves the same rows.

Generates C2's matrix on the device (1M users × 100K items, 50M signals, k = 64), fills the
item factors, downloads the user CSR and folds every user in as a foreign row: the same row
systems qmfx_wals_half(0) solves, with the plan built on the device and the rows, their plan
and their results going through the fold-in scratch.  Per precision it prints
  * fold_in kernel_ms: HIP events around the call's kernels (qmfx_solve_kernel_stats: planning,
    prologue, row solves, gather) and call_ms: the host clock around the whole call (the host's
    validation pass, the uploads and the copies of the result included);
  * half_ms: qmfx_kernel_stats_side class 2 (whole half) of the user half on the same data,
    measured in a fresh child process on the library named by --half-lib (default: QMFX_LIB
    or this tree's), so that the half of another build can stand beside this build's fold-in;
  * their ratio.
Prints one JSON line.

usage: bench_foldin.py [--half-lib PATH] [nusers=1000000] [nitems=100000] [nnz=50000000] [k=64]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA, LAM, REPS, SEED = 40.0, 0.05, 3, 2


def shape(argv):
    arg = [int(x) for x in argv] + [None] * 4
    return tuple(a if a is not None else d
                 for a, d in zip(arg, (1_000_000, 100_000, 50_000_000, 64)))


def generate(c, nu, ni, nnz):
    got = c.gen_synthetic(nu, ni, nnz, SEED)
    c.fill_uniform(1, 0.01, 2)
    return got


def half_main(argv):
    """Child: the user half's class-2 time per launch, per precision, on this process's library."""
    import ctypes

    import qmf_amd
    # a library built before the fold-in calls existed has none of them: the half needs none
    L = ctypes.CDLL(qmf_amd.LIB_PATH)
    for name in [n for n in qmf_amd._abi.SIGNATURES if "fold_in" in n and not hasattr(L, n)]:
        del qmf_amd._abi.SIGNATURES[name]
    nu, ni, nnz, k = shape(argv)
    out = {}
    for prec in (64, 32):
        with qmf_amd.Context(k, prec) as c:
            generate(c, nu, ni, nnz)
            c.wals_half(0, ALPHA, LAM)
            c.reset_stats()
            for _ in range(REPS):
                c.wals_half(0, ALPHA, LAM)
            st = c.kernel_stats_side(2, 0)
            out[str(prec)] = st["ms"] / st["launches"]
    print(json.dumps({"lib": qmf_amd.LIB_PATH, "half_ms": out}))


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--half-only":
        return half_main(argv[1:])
    half_lib = None
    if argv and argv[0] == "--half-lib":
        half_lib, argv = argv[1], argv[2:]
    import qmf_amd
    nu, ni, nnz, k = shape(argv)
    env = dict(os.environ)
    if half_lib:
        env["QMFX_LIB"] = os.path.abspath(half_lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--half-only"] +
                       [str(x) for x in (nu, ni, nnz, k)], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("the half measurement failed:\n" + r.stderr[-2000:])
    half = json.loads(r.stdout.splitlines()[-1])
    res = {}
    for prec in (64, 32):
        with qmf_amd.Context(k, prec) as c:
            got = generate(c, nu, ni, nnz)
            rp, col, val = c.download_csr(0)
            c.wals_fold_in(0, rp, col, val, ALPHA, LAM)
            c.reset_stats()
            t0 = time.perf_counter()
            for _ in range(REPS):
                F, losses, pivoted = c.wals_fold_in(0, rp, col, val, ALPHA, LAM)
            call_ms = (time.perf_counter() - t0) / REPS * 1e3
            st = c.solve_stats()
            kern_ms = st["ms"] / st["launches"]
            classes = c.fold_in_classes()
            own_half = c.wals_half(0, ALPHA, LAM)
            same = bool((c.factors(0) == F).all())
        h = half["half_ms"][str(prec)]
        res["f%d" % prec] = {"fold_in_kernel_ms": kern_ms, "fold_in_call_ms": call_ms, "half_ms": h,
                             "kernel_over_half": kern_ms / h, "rows_per_s": nu / (kern_ms * 1e-3),
                             "pivoted": pivoted, "classes": classes,
                             "rows_equal_own_half_bitwise": same,
                             "loss_sum_rel_diff": abs(losses.sum() - own_half) / abs(own_half)}
    print(json.dumps({"metric": "fold-in of C2's user side as foreign rows (kernel ms per call)",
                      "value": res["f32"]["fold_in_kernel_ms"], "unit": "ms",
                      "config": {"nusers": nu, "nitems": ni, "nnz": got, "nfactors": k,
                                 "alpha": ALPHA, "lambda": LAM, "reps": REPS},
                      "half_lib": half["lib"], "results": res}))


if __name__ == "__main__":
    main()
