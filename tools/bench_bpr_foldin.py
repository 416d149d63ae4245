"""BPR fold-in throughput (qmfx_bpr_fold_in) beside the training epoch on the same data.

Builds nrows new users of `per_row` distinct positives each over nitems items (strictly
ascending columns from seeded gaps), fills the item factors, and folds every row in with
nepochs passes and num_neg negatives.  The yardstick is qmfx_bpr_epoch at the same k, catalogue
and num_neg with those rows as the training users: a training step reads three rows and adds to
two atomically, a fold-in step reads two item rows and writes nothing shared.  Per precision it
prints
  * fold_in kernel_ms: HIP events around the call's kernels (qmfx_solve_kernel_stats: the
    start-value memset, the fold kernel, the gather) and call_ms: the host clock around the whole
    call (validation, uploads and result copies included), and steps per second from kernel_ms,
    steps = nepochs * num_neg * positives;
  * epoch_ms and its steps per second (steps = num_neg * positives), measured in a fresh child
    process on the library named by --epoch-lib (default: QMFX_LIB or this tree's), so that the
    epoch of another build can stand beside this build's fold-in;
  * the ratio of the two rates.
Prints one JSON line.

usage: bench_bpr_foldin.py [--epoch-lib PATH] [nrows=100000] [nitems=100000] [per_row=50]
                           [k=64] [num_neg=3] [nepochs=4]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR, DECAY, USER_LAMBDA, REPS, SEED = 0.05, 0.9, 0.025, 3, 2
DEFAULTS = (100_000, 100_000, 50, 64, 3, 4)


def shape(argv):
    arg = [int(x) for x in argv] + [None] * len(DEFAULTS)
    return tuple(a if a is not None else d for a, d in zip(arg, DEFAULTS))


def rows(nrows, nitems, per_row):
    """(rowptr, col): per_row strictly ascending items per row, from gaps in 1..nitems/per_row."""
    gaps = np.random.default_rng(SEED).integers(1, max(nitems // per_row, 1) + 1, (nrows, per_row))
    col = np.cumsum(gaps, axis=1) - 1
    assert col.max() < nitems
    return np.arange(nrows + 1, dtype=np.int64) * per_row, col.astype(np.int32).ravel()


def epoch_main(argv):
    """Child: the training epoch's kernel time, per precision, on this process's library."""
    import ctypes

    import qmf_amd
    # a library built before the BPR fold-in calls existed has none of them: the epoch needs none
    L = ctypes.CDLL(qmf_amd.LIB_PATH)
    for name in [n for n in qmf_amd._abi.SIGNATURES if "bpr_" in n and "fold_in" in n
                 and not hasattr(L, n)]:
        del qmf_amd._abi.SIGNATURES[name]
    nrows, ni, per_row, k, num_neg, _ = shape(argv)
    rp, col = rows(nrows, ni, per_row)
    users = np.repeat(np.arange(nrows, dtype=np.int64), per_row)
    out = {}
    for prec in (64, 32):
        with qmf_amd.Context(k, prec) as c:
            c.set_shape(nrows, ni)
            c.fill_uniform(0, 0.01, 1)
            c.fill_uniform(1, 0.01, 2)
            c.bpr_set_positives(users, col.astype(np.int64))
            c.bpr_epoch(1, num_neg, LR, 1.0, USER_LAMBDA, 0.0025, False)
            c.reset_stats()
            for r in range(REPS):
                c.bpr_epoch(2 + r, num_neg, LR, 1.0, USER_LAMBDA, 0.0025, False)
            st = c.solve_stats()
            out[str(prec)] = {"epoch_ms": st["ms"] / st["launches"], "plan": c.bpr_plan()}
    print(json.dumps({"lib": os.path.relpath(qmf_amd.LIB_PATH, ROOT), "epoch": out}))


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--epoch-only":
        return epoch_main(argv[1:])
    epoch_lib = None
    if argv and argv[0] == "--epoch-lib":
        epoch_lib, argv = argv[1], argv[2:]
    import qmf_amd
    nrows, ni, per_row, k, num_neg, nepochs = shape(argv)
    env = dict(os.environ)
    if epoch_lib:
        env["QMFX_LIB"] = os.path.abspath(epoch_lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--epoch-only"] +
                       [str(x) for x in (nrows, ni, per_row, k, num_neg, nepochs)], env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("the epoch measurement failed:\n" + r.stderr[-2000:])
    epoch = json.loads(r.stdout.splitlines()[-1])
    rp, col = rows(nrows, ni, per_row)
    npos = int(rp[-1])
    res = {}
    for prec in (64, 32):
        with qmf_amd.Context(k, prec) as c:
            c.set_shape(nrows, ni)
            c.fill_uniform(1, 0.01, 2)
            args = (rp, col, 7, nepochs, num_neg, LR, DECAY, USER_LAMBDA)
            first = c.bpr_fold_in(*args)
            c.reset_stats()
            t0 = time.perf_counter()
            for _ in range(REPS):
                F, losses = c.bpr_fold_in(*args)
            call_ms = (time.perf_counter() - t0) / REPS * 1e3
            st = c.solve_stats()
        kern_ms = st["ms"] / st["launches"]
        e = epoch["epoch"][str(prec)]
        fold_rate = nepochs * num_neg * npos / (kern_ms * 1e-3)
        epoch_rate = num_neg * npos / (e["epoch_ms"] * 1e-3)
        res["f%d" % prec] = {"fold_in_kernel_ms": kern_ms, "fold_in_call_ms": call_ms,
                             "fold_in_steps_per_s": fold_rate, "epoch_ms": e["epoch_ms"],
                             "epoch_steps_per_s": epoch_rate, "epoch_plan": e["plan"],
                             "fold_in_over_epoch": fold_rate / epoch_rate,
                             "calls_equal_bitwise": bool((F == first[0]).all() and
                                                         (losses == first[1]).all()),
                             "mean_last_pass_loss_per_step": float(losses.sum() / (num_neg * npos))}
    print(json.dumps({"metric": "BPR fold-in steps per second over the training epoch's (f32)",
                      "value": res["f32"]["fold_in_over_epoch"], "unit": "ratio",
                      "config": {"nrows": nrows, "nitems": ni, "per_row": per_row, "nfactors": k,
                                 "num_neg": num_neg, "nepochs": nepochs, "reps": REPS},
                      "epoch_lib": epoch["lib"], "results": res}))


if __name__ == "__main__":
    main()
