"""--item_similarities / --user_similarities of the drop-in CLIs (`wals`, `bpr`) on the MI355X.

A similarity file ("<id> <neighbourId> <score>" per line, 9 decimals) is checked against the
factor files of the same run.  Those round every factor to 9 decimals, so a score recomputed
from them differs from the device's; the bounds below are derived, not tuned.  With file rows
â = a + δ, |δ_f| ≤ 5e-10 (the device's rows are a, b; hats are the file's values):

  dot     |a·b − â·b̂| ≤ ed(a, b) = 5e-10·(‖â‖₁ + ‖b̂‖₁) + k·2.5e-19, as
          test_recommend_cli_gpu derives it; the printed score is itself rounded by at most
          5e-10:  e_dot = ed + 5e-10.
  norm    |‖a‖ − ‖â‖| ≤ ‖δ‖₂ ≤ en = 5e-10·√k, for either row.
  cosine  c = d/(na·nb), ĉ = d̂/(n̂a·n̂b).  c − ĉ = ((d − d̂) + ĉ·(n̂a·n̂b − na·nb))/(na·nb) with
          |n̂a·n̂b − na·nb| ≤ en·(n̂a + n̂b) + en² and na·nb ≥ (n̂a − en)·(n̂b − en), so
          e_cos = (ed + |ĉ|·(en·(n̂a + n̂b) + en²)) / ((n̂a − en)·(n̂b − en)) + 5e-10.
          A row whose file norm is not above en could be a zero row on the device (cosine 0.0
          whatever the file says): with |c|, |ĉ| ≤ 1 (up to rounding) the bound is then 2.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import load_tiny, synth
from test_cli_gpu import BIN, read_factors, run, write_dataset
from test_recommend_cli_gpu import by_user, read_recs

pytestmark = pytest.mark.gpu


def file_scores_and_bounds(F, r, k, metric):
    """Row r's scores against every row, recomputed from the file factors F, and the bound of
    each one's distance from the printed score."""
    l1 = np.abs(F).sum(axis=1)
    ed = 5e-10 * (l1[r] + l1) + k * 2.5e-19
    d = F @ F[r]
    if metric == "dot":
        return d, ed + 5e-10
    en = 5e-10 * np.sqrt(k)
    nrm = np.sqrt((F * F).sum(axis=1))
    ok = (nrm > en) & (nrm[r] > en)
    den = np.where(ok, nrm[r] * nrm, 1.0)
    c = np.where(ok, d / den, 0.0)
    lo = np.where(ok, (nrm[r] - en) * (nrm - en), 1.0)
    e = (ed + np.abs(c) * (en * (nrm[r] + nrm) + en * en)) / lo + 5e-10
    return c, np.where(ok, e, 2.0)


def check_against_factors(path, ids, F, topn, k, metric, queries=None):
    """Queries in ascending index order (or the list's), each with min(topn, n − 1)
    contiguous lines in non-increasing score order, never itself, no neighbour twice; the
    printed scores match the file factors; no row left out beats the query's last line."""
    order, lists = by_user(read_recs(path))
    ix = {int(x): n for n, x in enumerate(ids)}
    n = len(ids)
    expect = [int(x) for x in (ids if queries is None else queries)] if n > 1 else []
    assert order == expect
    for qid in order:
        got = lists[qid]
        assert len(got) == min(topn, n - 1), qid
        ws = [w for _, w in got]
        assert all(a >= b for a, b in zip(ws, ws[1:])), qid
        nb = [ix[i] for i, _ in got]
        assert qid not in [i for i, _ in got] and len(set(nb)) == len(nb), qid
        s, e = file_scores_and_bounds(F, ix[qid], k, metric)
        for j, w in zip(nb, ws):
            assert abs(w - s[j]) <= e[j], (qid, int(ids[j]), w, s[j], e[j])
        rest = np.setdiff1d(np.arange(n), nb + [ix[qid]])
        if len(rest):
            assert np.all(s[rest] <= ws[-1] + e[rest] + e[nb[-1]]), qid


def cli_run(tmp_path, exe, u, i, v, k, *extra, tag="r"):
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    uf, itf, si, su = (str(tmp_path / (tag + x)) for x in ("U.txt", "I.txt", "SI.txt", "SU.txt"))
    train = ["--nepochs=2"] if exe == "wals" else \
        ["--nepochs=2", "--init_distribution_bound=0.1", "--seed=5"]
    log = run(exe, "--train_dataset=" + data, "--nfactors=%d" % k, *train,
              "--user_factors=" + uf, "--item_factors=" + itf, "--item_similarities=" + si,
              "--user_similarities=" + su, *extra)
    return log, read_factors(uf), read_factors(itf), si, su


@pytest.mark.parametrize("exe,case,metric,topn", [
    ("wals", "tiny", "cosine", 3),
    ("wals", "synth", "dot", 128),      # 120 items: fewer than asked for; 300 users: 128 each
    ("bpr", "synth", "cosine", 128),
    ("bpr", "small", "dot", 3),
])
def test_cli_similarities(tmp_path, exe, case, metric, topn):
    (u, i, v), k = {"tiny": (load_tiny(), 8), "small": (synth(60, 40, 300, seed=2), 8),
                    "synth": (synth(300, 120, 4000, seed=6), 16)}[case]
    log, (uids, U), (iids, I), si, su = cli_run(
        tmp_path, exe, u, i, v, k, "--num_similar=%d" % topn, "--similarity=" + metric)
    check_against_factors(si, iids, I, topn, k, metric)
    check_against_factors(su, uids, U, topn, k, metric)
    # the files are the dataset format: the project's reader takes every line
    r = subprocess.run([os.path.join(BIN, "qmf_tool"), "read-seq", si], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and int(r.stdout.split()[0]) == len(read_recs(si))


def test_wals_cli_similar_id_lists_and_defaults(tmp_path):
    """Id files: the list's order, an unknown id skipped with one warning; the defaults are
    cosine and 10 neighbours; QMF_TIMINGS adds the phase's line."""
    u, i, v = synth(300, 120, 4000, seed=6)
    k = 16
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    item_ids = sorted(set(i.tolist()))
    user_ids = sorted(set(u.tolist()))
    want_i = [item_ids[17], item_ids[3]]
    want_u = [user_ids[200], user_ids[0], user_ids[41]]
    fi, fu = str(tmp_path / "items.txt"), str(tmp_path / "users.txt")
    with open(fi, "w") as f:
        f.write("%d\n%d\n%d\n" % (want_i[0], max(item_ids) + 1000, want_i[1]))
    with open(fu, "w") as f:
        f.write("".join("%d\n" % x for x in want_u))
    uf, itf, si, su = (str(tmp_path / x) for x in ("U.txt", "I.txt", "SI.txt", "SU.txt"))
    env = dict(os.environ, QMF_TIMINGS="1")
    r = subprocess.run([os.path.join(BIN, "wals"), "--train_dataset=" + data, "--nfactors=%d" % k,
                        "--nepochs=2", "--user_factors=" + uf, "--item_factors=" + itf,
                        "--item_similarities=" + si, "--user_similarities=" + su,
                        "--similar_item_ids=" + fi, "--similar_user_ids=" + fu],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "1 requested item ids are not in the training data" in r.stderr
    assert "requested user ids" not in r.stderr
    assert "timing: similar" in r.stderr
    uids, U = read_factors(uf)
    iids, I = read_factors(itf)
    check_against_factors(si, iids, I, 10, k, "cosine", queries=want_i)
    check_against_factors(su, uids, U, 10, k, "cosine", queries=want_u)


@pytest.mark.parametrize("exe", ["wals", "bpr"])
def test_cli_without_the_flags_writes_no_similarities(tmp_path, exe):
    u, i, v = synth(60, 40, 300, seed=2)
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    before = set(os.listdir(tmp_path))
    run(exe, "--train_dataset=" + data, "--nfactors=8", "--nepochs=1",
        "--user_factors=" + str(tmp_path / "U"), "--item_factors=" + str(tmp_path / "I"),
        "--num_similar=5", "--similarity=dot")
    assert set(os.listdir(tmp_path)) - before == {"U", "I"}


@pytest.mark.parametrize("exe", ["wals", "bpr"])
@pytest.mark.parametrize("flag,message", [
    ("--num_similar=129", "--num_similar must be in 1..128"),
    ("--num_similar=0", "--num_similar must be in 1..128"),
    ("--similarity=euclid", "--similarity must be cosine or dot"),
])
def test_cli_rejects_bad_similarity_flags(tmp_path, exe, flag, message):
    u, i, v = load_tiny()
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    r = subprocess.run([os.path.join(BIN, exe), "--train_dataset=" + data, "--nfactors=8",
                        "--nepochs=1", "--item_similarities=" + str(tmp_path / "S"), flag],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in r.stderr
    assert not os.path.exists(tmp_path / "S")
