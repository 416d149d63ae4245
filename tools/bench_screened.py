"""Screened top-N (qmfx_recommend_screened) beside the dense call (qmfx_recommend) on one shape.

Fills a shape on the device (default: C2's factor shape, 4096 users x 100K items, k = 64), then,
in one process and alternating the calls rep by rep, times qmfx_recommend(QMFX_REC_ALL) and
qmfx_recommend_screened for the same users: with sample and cap auto, and over a sweep of
`sample` (cap auto).  Device time is HIP events around each call's stages
(qmfx_solve_kernel_stats); the screened call's stages come from
qmfx_recommend_screen_stage_ms, its list lengths and exact-scan share from
qmfx_recommend_screen_stats.  The lists of every screened call are compared with the dense
call's.  Prints one JSON line per (precision, topn): median of `reps` with min..max, users/s,
the speed-up over the dense call, and the screen stage's TFLOP/s against the 157.3 TFLOP/s f32
MFMA peak.

usage: bench_screened.py [precision=0 (both)] [nusers=4096] [nitems=100000] [k=64]
                         [topn=0 (10 and 100)] [reps=7]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import qmf_amd  # noqa: E402

STAGES = ("sample", "prepare", "screen", "sort", "rerank", "exact")


def bench(prec, nu, ni, k, topn, reps):
    users = np.arange(nu, dtype=np.int64)
    s0 = int(np.ceil(np.sqrt(8.0 * topn * ni) / 64) * 64)
    sweep = sorted({min(ni, max(topn, int(s0 * f) // 64 * 64)) for f in (0.125, 0.25, 0.5, 1, 2)})
    calls = {"dense": lambda c: c.recommend(users, topn, 0),
             "screened_auto": lambda c: c.recommend_screened(users, topn, 0)}
    for s in sweep:
        calls["screened_S%d" % s] = lambda c, s=s: c.recommend_screened(users, topn, 0, False, s)
    kern = {n: [] for n in calls}
    wall = {n: [] for n in calls}
    stage = {n: [] for n in calls}
    stats = {}
    with qmf_amd.Context(k, prec) as c:
        c.set_shape(nu, ni)
        c.fill_uniform(0, 0.5, 1)
        c.fill_uniform(1, 0.5, 2)
        want = calls["dense"](c)
        for name, f in calls.items():   # warm up every kernel, grow the scratch, check the lists
            got = f(c)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
            stats[name] = c.screen_stats().tolist() if name != "dense" else None
        for _ in range(reps):
            for name, f in calls.items():
                c.reset_stats()
                t0 = time.perf_counter()
                f(c)
                wall[name].append((time.perf_counter() - t0) * 1e3)
                st = c.solve_stats()
                assert st["launches"] == 1
                kern[name].append(st["ms"])
                stage[name].append(c.screen_stage_ms())
    modes = {}
    for name in calls:
        ms = float(np.median(kern[name]))
        modes[name] = {"device_ms": ms, "device_ms_min": min(kern[name]),
                       "device_ms_max": max(kern[name]), "call_ms": float(np.median(wall[name])),
                       "users_per_s": nu / (ms * 1e-3)}
        if name != "dense":
            med = np.median(np.array(stage[name]), axis=0)
            modes[name]["stage_ms"] = dict(zip(STAGES, (float(x) for x in med)))
            modes[name]["stats"] = dict(zip(("screened", "exact", "kept", "longest"), stats[name]))
            modes[name]["speedup"] = modes["dense"]["device_ms"] / ms
            if med[2] > 0:
                modes[name]["screen_tflops"] = 2.0 * nu * ni * k / (med[2] * 1e-3) / 1e12
    best = modes["screened_auto"]
    return {"metric": "screened top-N (users per second, device time, all items eligible)",
            "value": best["users_per_s"], "unit": "users/s",
            "config": {"nusers": nu, "nitems": ni, "nfactors": k, "topn": topn, "reps": reps,
                       "precision": "f%d storage, f32 screen, f64 scores" % prec},
            "modes": modes,
            "roofline": {"bound": "f32 mfma (screen stage)", "peak": 157.3, "unit": "TFLOP/s",
                         "achieved": best.get("screen_tflops", 0.0),
                         "frac": best.get("screen_tflops", 0.0) / 157.3}}


def main():
    arg = [int(x) for x in sys.argv[1:]] + [None] * 6
    prec, nu, ni, k, topn, reps = (a if a is not None else d
                                   for a, d in zip(arg, (0, 4096, 100_000, 64, 0, 7)))
    for p in ((32, 64) if prec == 0 else (prec,)):
        for n in ((10, 100) if topn == 0 else (topn,)):
            print(json.dumps(bench(p, nu, ni, k, n, reps)), flush=True)


if __name__ == "__main__":
    main()
