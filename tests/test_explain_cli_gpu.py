"""--recommendation_explanations / --fold_in_explanations / --num_explanations of the `wals` CLI
on the MI355X, on tests/golden/tiny.txt (10 users, 12 items, 57 lines, two repeated pairs).

One run trains, writes the recommendations of the trained users and of the same lines folded
in again (--fold_in_dataset = the training file), and explains both files with 3 sources per
pair.  Every (user, item) pair of a recommendations file must appear in the explanations file,
in that order, with min(3, the user's lines) sources, each an item of the user's own lines, in
non-increasing order of contribution.  The contributions are compared with
test_explain.explain_reference on the saved item factors (α = 40, λ = 0.05, the CLI's defaults).

The bound is 1e-6 absolute, four significant digits of the 9 decimals the files carry.  The
item factor file rounds every factor by up to 5e-10, so the reference solves a slightly
different system, and the explanations file rounds a contribution by up to 5e-10 again; how far
the first moves a contribution depends on the conditioning of the users' systems on this
model.  Measured on the MI355X, max |file − reference|: 2.1e-8 (trained users) and 1.3e-8
(folded in) at fp64, 7.7e-8 and 4.5e-8 at fp32 (the device holds fp32 factors there; the file
prints them exactly enough): at most a thirteenth of the bound.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import load_tiny
from test_cli_gpu import BIN, read_factors, run, write_dataset, write_dist
from test_explain import explain_reference
from test_recommend_cli_gpu import read_recs

pytestmark = pytest.mark.gpu

K, EPOCHS, ALPHA, LAM, TOPN, TOPM = 8, 2, 40.0, 0.05, 4, 3
BOUND = 1e-6


def read_explanations(path):
    """[(user id, item id, source item id, contribution)] in file order."""
    out = []
    for line in open(path).read().splitlines():
        u, i, s, w = line.split(" ")
        assert len(w.split(".")[1]) == 9, line
        out.append((int(u), int(i), int(s), float(w)))
    return out


def check_explanations(tag, recs, expl, lines_of, iids, I):
    """recs: a recommendations file; expl: its explanations; lines_of: user id → (items, values)
    of the user's lines.  Returns the largest deviation from the reference."""
    ix = {int(x): n for n, x in enumerate(iids)}
    at, worst = 0, 0.0
    for u, i, _ in recs:
        items, values = lines_of[u]
        order = np.argsort([ix[x] for x in items], kind="stable")  # the engine's CSR order
        col = np.array([ix[items[e]] for e in order])
        val = np.array([values[e] for e in order])
        ref = explain_reference(np.array([0, len(col)]), col, val, I, 0, ix[i], ALPHA, LAM)[0]
        n = min(TOPM, len(col))
        got = expl[at:at + n]
        at += n
        assert len(got) == n and all(g[0] == u and g[1] == i for g in got), (tag, u, i, got)
        ws = [g[3] for g in got]
        assert all(a >= b for a, b in zip(ws, ws[1:])), (tag, u, i, ws)
        left = list(range(len(col)))
        for _, _, s, w in got:
            assert s in ix and ix[s] in col[left], (tag, u, i, s)
            e = min((e for e in left if col[e] == ix[s]), key=lambda e: abs(ref[e] - w))
            left.remove(e)
            worst = max(worst, abs(ref[e] - w))
        # nothing that was left out beats the last source listed
        if left and n:
            assert ref[left].max() <= ws[-1] + 2 * BOUND, (tag, u, i)
    assert at == len(expl), (tag, at, len(expl))
    return worst


@pytest.mark.parametrize("precision", [64, 32])
def test_cli_explains_the_pairs_of_both_recommendation_files(tmp_path, precision):
    u, i, v = load_tiny()
    data, dist = str(tmp_path / "train.txt"), str(tmp_path / "dist.dat")
    write_dataset(data, u, i, v)
    ni = len(np.unique(i))
    write_dist(dist, np.random.default_rng(K).uniform(-0.01, 0.01, (ni, K)))
    out = {x: str(tmp_path / (x + ".txt")) for x in ("U", "I", "R", "E", "FR", "FE")}
    run("wals", "--train_dataset=" + data, "--nfactors=%d" % K, "--nepochs=%d" % EPOCHS,
        "--distribution_file=" + dist, "--precision=%d" % precision,
        "--user_factors=" + out["U"], "--item_factors=" + out["I"],
        "--user_recommendations=" + out["R"], "--recommendation_explanations=" + out["E"],
        "--fold_in_dataset=" + data, "--fold_in_recommendations=" + out["FR"],
        "--fold_in_explanations=" + out["FE"], "--num_recommendations=%d" % TOPN,
        "--num_explanations=%d" % TOPM)
    iids, I = read_factors(out["I"])
    lines_of = {int(x): (i[u == x].tolist(), v[u == x].tolist()) for x in np.unique(u)}
    assert min(len(a) for a, _ in lines_of.values()) < TOPM < max(len(a) for a, _ in lines_of.values())
    for tag, r, e in (("trained", "R", "E"), ("folded", "FR", "FE")):
        recs = read_recs(out[r])
        assert len(recs) > 0
        worst = check_explanations(tag, recs, read_explanations(out[e]), lines_of, iids, I)
        print("EXPLAIN cli %s p=%d pairs=%d max |file - ref| = %.3g (bound %.1g)"
              % (tag, precision, len(recs), worst, BOUND))
        assert worst <= BOUND
    # for a folded-in user the contributions of a pair are its score, split up: with every
    # source listed they add up to the recommendation's score
    out2 = {x: str(tmp_path / (x + "2.txt")) for x in ("FR", "FE")}
    run("wals", "--train_dataset=" + data, "--nfactors=%d" % K, "--nepochs=%d" % EPOCHS,
        "--distribution_file=" + dist, "--precision=%d" % precision,
        "--fold_in_dataset=" + data, "--fold_in_recommendations=" + out2["FR"],
        "--fold_in_explanations=" + out2["FE"], "--num_recommendations=2",
        "--num_explanations=128", "--user_factors=" + out["U"], "--item_factors=" + out["I"])
    sums = {}
    for uu, ii, _, w in read_explanations(out2["FE"]):
        sums[(uu, ii)] = sums.get((uu, ii), 0.0) + w
    recs = read_recs(out2["FR"])
    assert len(recs) == len(sums)
    nmax = max(len(a) for a, _ in lines_of.values())
    tol = (1e-9 if precision == 64 else 1e-4) + (nmax + 1) * 5e-10  # the bar + the files' rounding
    for uu, ii, score in recs:
        assert abs(sums[(uu, ii)] - score) <= tol * max(1.0, abs(score)), (uu, ii, score)


@pytest.mark.parametrize("flags, message", [
    (("--recommendation_explanations=E",), "--recommendation_explanations needs --user_recommendations"),
    (("--fold_in_dataset=D", "--fold_in_explanations=E"),
     "--fold_in_explanations needs --fold_in_recommendations"),
    (("--user_recommendations=R", "--recommendation_explanations=E", "--num_explanations=0"),
     "--num_explanations must be in 1..128"),
    (("--user_recommendations=R", "--recommendation_explanations=E", "--num_explanations=129"),
     "--num_explanations must be in 1..128"),
])
def test_cli_flags_need_their_companions(tmp_path, flags, message):
    u, i, v = load_tiny()
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    flags = [f.replace("=D", "=" + data).replace("=E", "=" + str(tmp_path / "E"))
             .replace("=R", "=" + str(tmp_path / "R")) for f in flags]
    r = subprocess.run([os.path.join(BIN, "wals"), "--train_dataset=" + data, "--nfactors=8",
                        "--nepochs=1"] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
