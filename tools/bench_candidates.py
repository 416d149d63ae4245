"""Device top-N within candidate sets (qmfx_recommend_candidates, qmfx_recommend_without) against
the dense qmfx_recommend call on the same context in the same process.

Generates bench_recommend.py's shape on the device (default: C2's factor shape, 4096 users ×
100K items, k = 64), then times, with all items eligible (exclude = 0):
  * per_user_1000   every user with its own list of `ncand` random candidates;
  * shared_1000     every user over one shared list of `ncand` random candidates;
  * one_user_all    one user over a shared list of every item (chunks must cover the GPU);
  * deny_1000       the dense scan with `ncand` items denied;
  * dense           plain qmfx_recommend for every user, and for the one user.
Per case: HIP events around the call's kernels (qmfx_solve_kernel_stats), the host clock around
the whole call (validation, uploads and result copies included), users/s on the kernel time,
and the fp64 VALU roofline of the scoring (one rounded multiply + one rounded add per factor:
half the 78.6 TFLOP/s FMA peak) on the work the call reports.  Prints one JSON line.

usage: bench_candidates.py [precision=32] [nusers=4096] [nitems=100000] [k=64] [topn=10] [ncand=1000]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import qmf_amd  # noqa: E402

PEAK = 39.3  # TFLOP/s, unfused mul + add


def timed(c, call, nusers, reps=5):
    call()
    c.reset_stats()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    st = c.solve_stats()
    kern_ms = st["ms"] / st["launches"]
    tflops = st["flops"] / st["launches"] / (kern_ms * 1e-3) / 1e12
    return {"kernel_ms": kern_ms, "call_ms": wall_ms, "users_per_s": nusers / (kern_ms * 1e-3),
            "roofline": {"bound": "fp64 valu", "achieved": tflops, "peak": PEAK,
                         "unit": "TFLOP/s (mul+add, unfused)", "frac": tflops / PEAK}}


def main():
    arg = [int(x) for x in sys.argv[1:]] + [None] * 6
    prec, nu, ni, k, topn, ncand = (a if a is not None else d
                                    for a, d in zip(arg, (32, 4096, 100_000, 64, 10, 1000)))
    rng = np.random.default_rng(0)
    users = np.arange(nu, dtype=np.int64)
    one = users[:1]
    # stratified random lists: one item from each of ncand equal cells of the catalogue, so a
    # list is strictly ascending as drawn
    cell = ni // ncand
    lists = np.arange(ncand, dtype=np.int64) * cell + rng.integers(0, cell, (nu, ncand))
    cand = lists.ravel()
    cptr = np.arange(nu + 1, dtype=np.int64) * ncand
    shared = lists[0].copy()
    everything = np.arange(ni, dtype=np.int64)
    with qmf_amd.Context(k, prec) as c:
        c.gen_synthetic(nu, ni, nu * 100, 7)
        c.fill_uniform(0, 0.5, 1)
        c.fill_uniform(1, 0.5, 2)
        cases = {
            "per_user_%d" % ncand: timed(c, lambda: c.recommend_candidates(users, topn, cand, cptr), nu),
            "shared_%d" % ncand: timed(c, lambda: c.recommend_candidates(users, topn, shared), nu),
            "one_user_all": timed(c, lambda: c.recommend_candidates(one, topn, everything), 1),
            "deny_%d" % ncand: timed(c, lambda: c.recommend_without(users, shared, topn), nu),
            "dense": timed(c, lambda: c.recommend(users, topn), nu),
            "dense_one_user": timed(c, lambda: c.recommend(one, topn), 1),
        }
    dense = cases["dense"]["kernel_ms"]
    out = {"metric": "top-N within %d candidates per user (users per second, kernels)" % ncand,
           "value": cases["per_user_%d" % ncand]["users_per_s"], "unit": "users/s",
           "config": {"nusers": nu, "nitems": ni, "nfactors": k, "topn": topn, "ncand": ncand,
                      "precision": "f%d storage, f64 scores" % prec},
           "cases": cases,
           "dense_over_per_user": dense / cases["per_user_%d" % ncand]["kernel_ms"],
           "dense_over_shared": dense / cases["shared_%d" % ncand]["kernel_ms"],
           "work_ratio": ni / ncand}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
