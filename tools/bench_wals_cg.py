"""The conjugate-gradient half (qmfx_wals_half_cg) beside the exact half on the same data.

Per shape (C2: 1M × 100K, 50M signals, k = 64; C3: 10M × 1M, 500M signals, k = 128; both from
qmfx_gen_synthetic) and precision, one child process
  * times, per side, the exact half and the CG half at 1, 2, 3 and 5 steps in alternation
    (REPS rounds; the context's HIP events around the whole half: qmfx_kernel_stats_side class 2)
    and reports the median with min..max, and the CG half's flop/s by the model
    (steps + 1)·(2k² + 4nk) per row;
  * trains 10 epochs from the same start with each solver and reports the loss of the last item
    half divided by nusers·nitems (the reference's printed training loss).
Each child writes <out>/<config>_f<precision>.json; the parent prints one JSON line.

usage: bench_wals_cg.py [--out DIR] [--configs c2,c3] [--precisions 64,32]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": (1_000_000, 100_000, 50_000_000, 64, 2),
           "c3": (10_000_000, 1_000_000, 500_000_000, 128, 3)}
ALPHA, LAM, REPS, EPOCHS = 40.0, 0.05, 5, 10
STEPS = (1, 2, 3, 5)


def half(c, side, steps):
    if steps == 0:
        return c.wals_half(side, ALPHA, LAM)
    return c.wals_half_cg(side, ALPHA, LAM, steps)


def child(config, precision, out):
    import qmf_amd
    nu, ni, nnz, k, seed = CONFIGS[config]
    res = {"config": config, "precision": precision, "nusers": nu, "nitems": ni, "nfactors": k,
           "alpha": ALPHA, "lambda": LAM, "reps": REPS, "epochs": EPOCHS}
    with qmf_amd.Context(k, precision) as c:
        res["nnz"] = c.gen_synthetic(nu, ni, nnz, seed)

        def start():
            c.fill_uniform(1, 0.01, 2)
            c.fill_uniform(0, 0.0, 1)  # users start at zero, as the CLI's

        start()
        for side in (0, 1):  # warm-up: every kernel once
            half(c, side, 0)
            half(c, side, 1)
        times = {s: ([], []) for s in (0,) + STEPS}
        flops = {}
        for _ in range(REPS):
            for s in (0,) + STEPS:
                for side in (0, 1):
                    c.reset_stats()
                    half(c, side, s)
                    st = c.kernel_stats_side(2, side)
                    times[s][side].append(st["ms"])
                    flops[(s, side)] = st["flops"]
        res["half_ms"] = {}
        for s in (0,) + STEPS:
            name = "exact" if s == 0 else "cg%d" % s
            res["half_ms"][name] = {}
            for side in (0, 1):
                t = times[s][side]
                med = statistics.median(t)
                res["half_ms"][name]["users" if side == 0 else "items"] = {
                    "median": med, "min": min(t), "max": max(t),
                    "model_gflops": flops[(s, side)] / med * 1e-6}
        res["loss_after_%d_epochs" % EPOCHS] = {}
        for s in (0,) + STEPS:
            start()
            loss = 0.0
            for _ in range(EPOCHS):
                half(c, 0, s)
                loss = half(c, 1, s) / nu / ni
            res["loss_after_%d_epochs" % EPOCHS]["exact" if s == 0 else "cg%d" % s] = loss
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "%s_f%d.json" % (config, precision)), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wals_cg"))
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--precisions", default="64,32")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.out)
    results = []
    for config in a.configs.split(","):
        for prec in a.precisions.split(","):
            # one process per shape and precision
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", a.out, "--child",
                                config, prec], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("%s fp%s failed:\n%s" % (config, prec, r.stderr[-2000:]))
            results.append(json.loads(r.stdout.splitlines()[-1]))
    c3 = [r for r in results if r["config"] == "c3" and r["precision"] == 64]
    value = c3[0]["half_ms"]["cg3"]["items"]["median"] if c3 else None
    print(json.dumps({"metric": "CG half, 3 steps, C3 fp64 item side (ms)", "value": value,
                      "unit": "ms", "results": results}))


if __name__ == "__main__":
    main()
