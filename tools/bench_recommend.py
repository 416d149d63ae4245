"""Device top-N recommendation throughput (qmfx_recommend) against the scoring-only floor.

Generates a shape on the device (default: C2's factor shape, 4096 users × 100K items, k = 64,
100 signals per user), then times
  * qmfx_recommend for every user, with all items eligible and with the users' signals left
    out: HIP events around the call's kernels (qmfx_solve_kernel_stats) and the host clock
    around the whole call (copies of the result included);
  * qmfx_eval_ranks for the same users and items with an empty label set: the same scores
    with nothing selected, i.e. the scoring-only floor (host clock around the call, which
    ends in a stream synchronise; its copies are empty).
Prints one JSON line: users/s, the times, their ratio to the floor, and the fp64 VALU
roofline of the scoring (one rounded multiply + one rounded add per factor: half the 78.6
TFLOP/s FMA peak).

usage: bench_recommend.py [precision=32] [nusers=4096] [nitems=100000] [k=64] [topn=10]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import qmf_amd  # noqa: E402


def main():
    arg = [int(x) for x in sys.argv[1:]] + [None] * 5
    prec, nu, ni, k, topn = (a if a is not None else d
                             for a, d in zip(arg, (32, 4096, 100_000, 64, 10)))
    reps = 5
    users = np.arange(nu, dtype=np.int64)
    with qmf_amd.Context(k, prec) as c:
        nnz = c.gen_synthetic(nu, ni, nu * 100, 7)
        c.fill_uniform(0, 0.5, 1)
        c.fill_uniform(1, 0.5, 2)
        c.eval_set_labels(users, np.zeros(nu + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))
        c.eval_ranks()
        t0 = time.perf_counter()
        for _ in range(reps):
            c.eval_ranks()
        eval_ms = (time.perf_counter() - t0) / reps * 1e3
        modes = {}
        for name, excl in (("all", 0), ("unseen_signals", 1)):
            c.recommend(users, topn, excl)
            c.reset_stats()
            t0 = time.perf_counter()
            for _ in range(reps):
                c.recommend(users, topn, excl)
            wall_ms = (time.perf_counter() - t0) / reps * 1e3
            st = c.solve_stats()
            kern_ms = st["ms"] / st["launches"]
            modes[name] = {"kernel_ms": kern_ms, "call_ms": wall_ms,
                           "users_per_s": nu / (kern_ms * 1e-3),
                           "kernel_over_eval": kern_ms / eval_ms}
    flops = 2.0 * nu * ni * k
    best = modes["unseen_signals"]
    out = {"metric": "top-N recommendations (users per second, kernels, signals left out)",
           "value": best["users_per_s"], "unit": "users/s",
           "config": {"nusers": nu, "nitems": ni, "nfactors": k, "topn": topn, "nnz": nnz,
                      "precision": "f%d storage, f64 scores" % prec},
           "eval_ranks_ms": eval_ms, "modes": modes,
           "roofline": {"bound": "fp64 valu", "achieved": flops / (best["kernel_ms"] * 1e-3) / 1e12,
                        "peak": 39.3, "unit": "TFLOP/s (mul+add, unfused)",
                        "frac": flops / (best["kernel_ms"] * 1e-3) / 1e12 / 39.3}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
