"""Explanation throughput (qmfx_wals_explain) beside the fold-in of the same rows.

Generates C2's matrix on the device (1M users × 100K items, 50M signals, k = 64, fp64), fills
the item factors and explains, for the first 65,536 users, 10 seeded targets each with
topm = 5: one query per user, one kept Cholesky factor per query.  Beside it, in the same
process on the same build, qmfx_wals_fold_in of the same 65,536 rows (tools/bench_foldin.py's
call on bench_foldin's data): a fold-in row's time is the yardstick, both build the same k×k
system per row.  One warm-up call of each, then REPS calls alternating between the two; the
times are HIP events around each call's kernels (qmfx_solve_kernel_stats; YᵀY included in
both), reported as the mean with the per-call host-clock minimum and maximum beside it.
Prints one JSON line.

usage: bench_explain.py [nusers=1000000] [nitems=100000] [nnz=50000000] [k=64] [nq=65536]
                        [ntargets=10] [topm=5] [precision=64]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_foldin import ALPHA, LAM, generate  # noqa: E402

REPS = 5


def main():
    import qmf_amd
    arg = [int(x) for x in sys.argv[1:]] + [None] * 8
    nu, ni, nnz, k, nq, nt, topm, prec = (
        a if a is not None else d
        for a, d in zip(arg, (1_000_000, 100_000, 50_000_000, 64, 65536, 10, 5, 64)))
    nq = min(nq, nu)
    with qmf_amd.Context(k, prec) as c:
        got = generate(c, nu, ni, nnz)
        rows = np.arange(nq, dtype=np.int64)
        qptr = np.arange(nq + 1, dtype=np.int64) * nt
        targets = np.random.default_rng(5).integers(0, ni, nq * nt).astype(np.int64)
        rp, col, val = c.download_csr(0)
        rp, col, val = rp[:nq + 1], col[:rp[nq]], val[:rp[nq]]
        lengths = np.diff(rp)
        c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, topm)
        X = c.wals_fold_in(0, rp, col, val, ALPHA, LAM)[0]
        ms = {"explain": [], "fold_in": []}
        wall = {"explain": [], "fold_in": []}
        for _ in range(REPS):
            for name, call in (("explain", lambda: c.wals_explain(0, rows, qptr, targets, ALPHA,
                                                                  LAM, topm)),
                               ("fold_in", lambda: c.wals_fold_in(0, rp, col, val, ALPHA, LAM))):
                c.reset_stats()
                t0 = time.perf_counter()
                out = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                st = c.solve_stats()
                assert st["launches"] == 1
                ms[name].append(st["ms"])
                if name == "explain":
                    totals, flops = out[4], st["flops"]
        # the totals are the folded-in rows' scores of the targets
        score = np.einsum("qtk,qk->qt", c.factors(1)[targets.reshape(nq, nt)], X).ravel()
        err = float(np.max(np.abs(totals - score)) / np.max(np.abs(score)))
    ex, fi = float(np.mean(ms["explain"])), float(np.mean(ms["fold_in"]))
    res = {"explain_kernel_ms": ex, "explain_kernel_ms_all": ms["explain"],
           "explain_us_per_query": ex * 1e3 / nq, "explain_us_per_pair": ex * 1e3 / (nq * nt),
           "explain_call_ms_min_max": [min(wall["explain"]), max(wall["explain"])],
           "explain_gflops": flops / (ex * 1e6),
           "fold_in_kernel_ms": fi, "fold_in_kernel_ms_all": ms["fold_in"],
           "fold_in_us_per_row": fi * 1e3 / nq,
           "fold_in_call_ms_min_max": [min(wall["fold_in"]), max(wall["fold_in"])],
           "explain_query_over_fold_in_row": ex / fi,
           "signals_per_row_mean": float(lengths.mean()), "signals_per_row_max": int(lengths.max()),
           "totals_vs_fold_in_scores_rel": err}
    print(json.dumps({"metric": "explanations of 10 targets for C2 users (kernel µs per query)",
                      "value": res["explain_us_per_query"], "unit": "us",
                      "config": {"nusers": nu, "nitems": ni, "nnz": got, "nfactors": k,
                                 "precision": prec, "queries": nq, "targets_per_query": nt,
                                 "topm": topm, "alpha": ALPHA, "lambda": LAM, "reps": REPS},
                      "results": res}))


if __name__ == "__main__":
    main()
