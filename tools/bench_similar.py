"""Device similar-rows throughput (qmfx_similar) beside qmfx_recommend on the same shape.

Fills a shape on the device (default: C2's item shape, 100K items, k = 64, with 4096 users),
then, in one process and alternating the three calls rep by rep, times
  * qmfx_recommend(QMFX_REC_ALL) for the 4096 users: the comparison point (the same scoring
    and selection with the queries taken from the other side);
  * qmfx_similar on the item side for 4096 query rows spread over the matrix, by dot product
    and by cosine, the query row left out.
Kernel time is HIP events around each call's kernels (qmfx_solve_kernel_stats; the cosine
call's includes its norms pass), call time the host clock around the whole call (copies of
the result included).  Prints one JSON line per precision: queries/s, the times, each metric's
kernel time over recommend's, and the fp64 VALU roofline of the scoring (one rounded multiply
+ one rounded add per factor: half the 78.6 TFLOP/s FMA peak).

usage: bench_similar.py [precision=0 (both)] [nq=4096] [nrows=100000] [k=64] [topn=10]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import qmf_amd  # noqa: E402


def bench(prec, nq, n, k, topn, reps=7):
    users = np.arange(nq, dtype=np.int64)
    rows = (np.arange(nq, dtype=np.int64) * (n // nq if n >= nq else 1)) % n
    calls = {
        "recommend_all": lambda c: c.recommend(users, topn, 0),
        "similar_dot": lambda c: c.similar(1, rows, topn, qmf_amd.QMFX_SIM_DOT, True),
        "similar_cosine": lambda c: c.similar(1, rows, topn, qmf_amd.QMFX_SIM_COSINE, True),
    }
    kern = {name: [] for name in calls}
    wall = {name: [] for name in calls}
    with qmf_amd.Context(k, prec) as c:
        c.set_shape(nq, n)
        c.fill_uniform(0, 0.5, 1)
        c.fill_uniform(1, 0.5, 2)
        for f in calls.values():   # warm up every kernel and grow the scratch
            f(c)
        for _ in range(reps):
            for name, f in calls.items():
                c.reset_stats()
                t0 = time.perf_counter()
                f(c)
                wall[name].append((time.perf_counter() - t0) * 1e3)
                st = c.solve_stats()
                assert st["launches"] == 1
                kern[name].append(st["ms"])
    modes = {}
    for name in calls:
        ms = float(np.median(kern[name]))
        modes[name] = {"kernel_ms": ms, "kernel_ms_min": min(kern[name]),
                       "kernel_ms_max": max(kern[name]), "call_ms": float(np.median(wall[name])),
                       "queries_per_s": nq / (ms * 1e-3)}
    base = modes["recommend_all"]["kernel_ms"]
    for name in ("similar_dot", "similar_cosine"):
        modes[name]["kernel_over_recommend"] = modes[name]["kernel_ms"] / base
    flops = 2.0 * nq * n * k
    best = modes["similar_cosine"]
    tf = flops / (best["kernel_ms"] * 1e-3) / 1e12
    return {"metric": "similar rows (queries per second, kernels, cosine, query left out)",
            "value": best["queries_per_s"], "unit": "queries/s",
            "config": {"nq": nq, "nrows": n, "nfactors": k, "topn": topn, "reps": reps,
                       "precision": "f%d storage, f64 scores" % prec},
            "modes": modes,
            "roofline": {"bound": "fp64 valu", "achieved": tf, "peak": 39.3,
                         "unit": "TFLOP/s (mul+add, unfused)", "frac": tf / 39.3}}


def main():
    arg = [int(x) for x in sys.argv[1:]] + [None] * 5
    prec, nq, n, k, topn = (a if a is not None else d
                            for a, d in zip(arg, (0, 4096, 100_000, 64, 10)))
    for p in ((32, 64) if prec == 0 else (prec,)):
        print(json.dumps(bench(p, nq, n, k, topn)), flush=True)


if __name__ == "__main__":
    main()
