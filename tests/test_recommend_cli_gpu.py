"""--user_recommendations of the drop-in CLIs (`wals`, `bpr`) on the MI355X.

The recommendation file ("<userId> <itemId> <score>" per line, 9 decimals) is checked against
the factor files of the same run.  Those round every factor to 9 decimals, so a dot product
recomputed from them differs from the device's score; the bound below is derived, not tuned:
each factor is off by at most 5e-10, so |Σ u_f q_f − Σ û_f q̂_f| ≤ 5e-10·(‖u‖₁ + ‖q‖₁) + k·2.5e-19,
and the printed score is itself rounded by at most 5e-10:

    e(u, i) = 5e-10·(‖u‖₁ + ‖q_i‖₁ + 1) + k·2.5e-19

(the norms taken on the file values).  A bias read from the item file adds another 5e-10."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, load_tiny, synth
from test_cli_gpu import BIN, read_factors, run, write_dataset

pytestmark = pytest.mark.gpu


def read_recs(path):
    """[(user id, item id, score)] in file order."""
    out = []
    for line in open(path).read().splitlines():
        u, i, w = line.split(" ")
        assert len(w.split(".")[1]) == 9, line
        out.append((int(u), int(i), float(w)))
    return out


def by_user(recs):
    users, lists = [], {}
    for u, i, w in recs:
        if u not in lists:
            users.append(u)
            lists[u] = []
        assert users[-1] == u, "a user's lines are not contiguous"
        lists[u].append((i, w))
    return users, lists


def err(u, q, k):
    return 5e-10 * (np.abs(u).sum() + np.abs(q).sum() + 1.0) + k * 2.5e-19


def check_against_factors(recs, uids, U, iids, I, train, topn, k, bias=None, users=None):
    """Every user has min(topn, eligible) lines in non-increasing score order, none of them a
    training item (`train`: user id → set of item ids; None: nothing excluded); the printed
    scores match the file factors; no eligible item left out beats the user's last line."""
    order, lists = by_user(recs)
    uix = {int(x): n for n, x in enumerate(uids)}
    iix = {int(x): n for n, x in enumerate(iids)}
    eb = 5e-10 if bias is not None else 0.0
    expect = [int(x) for x in (uids if users is None else users)]
    expect = [u for u in expect
              if len(iids) - (len(train[u] & set(iix)) if train else 0) > 0]
    assert order == expect
    for u in order:
        seen = train[u] if train else set()
        got = lists[u]
        assert len(got) == min(topn, len(iids) - len(seen & set(iix))), u
        ws = [w for _, w in got]
        assert all(a >= b for a, b in zip(ws, ws[1:])), u
        assert len({i for i, _ in got}) == len(got)
        uf = U[uix[u]]
        dots = I @ uf + (bias if bias is not None else 0.0)
        es = np.array([err(uf, q, k) for q in I]) + eb
        for i, w in got:
            assert i not in seen, (u, i)
            assert abs(w - dots[iix[i]]) <= es[iix[i]], (u, i, w, dots[iix[i]])
        rest = [n for x, n in iix.items() if x not in seen and x not in {i for i, _ in got}]
        if rest and len(got) == topn:
            last_i, last_w = got[-1]
            rest = np.array(rest)
            assert np.all(dots[rest] <= last_w + es[rest] + es[iix[last_i]]), u


def wals_run(tmp_path, u, i, v, k, *extra, tag="r"):
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    uf, itf, rf = (str(tmp_path / (tag + x)) for x in ("U.txt", "I.txt", "R.txt"))
    log = run("wals", "--train_dataset=" + data, "--nfactors=%d" % k, "--nepochs=2",
              "--user_factors=" + uf, "--item_factors=" + itf, "--user_recommendations=" + rf,
              "--num_recommendations=5", *extra)
    return log, read_factors(uf), read_factors(itf), rf


def train_sets(u, i):
    t = {}
    for a, b in zip(u.tolist(), i.tolist()):
        t.setdefault(a, set()).add(b)
    return t


@pytest.mark.parametrize("case", ["tiny", "synth"])
def test_wals_cli_recommendations(tmp_path, case):
    (u, i, v), k = (load_tiny(), 8) if case == "tiny" else (synth(300, 120, 4000, seed=6), 16)
    log, (uids, U), (iids, I), rf = wals_run(tmp_path, u, i, v, k)
    recs = read_recs(rf)
    check_against_factors(recs, uids, U, iids, I, train_sets(u, i), 5, k)
    # the file is the dataset format: the project's reader takes every line
    r = subprocess.run([os.path.join(BIN, "qmf_tool"), "read-seq", rf], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and int(r.stdout.split()[0]) == len(recs)


def test_wals_cli_recommend_seen_and_user_list(tmp_path):
    u, i, v = synth(300, 120, 4000, seed=6)
    k = 16
    log, (uids, U), (iids, I), rf = wals_run(tmp_path, u, i, v, k, "--recommend_seen", tag="s")
    recs = read_recs(rf)
    check_against_factors(recs, uids, U, iids, I, None, 5, k)
    train = train_sets(u, i)
    assert any(it in train[uu] for uu, it, _ in recs), "no training item among 1,500 lines"
    # two known ids and one unknown, in file order
    known = [int(uids[17]), int(uids[3])]
    ufile = str(tmp_path / "users.txt")
    with open(ufile, "w") as f:
        f.write("%d\n%d\n%d\n" % (known[0], int(uids.max()) + 1000, known[1]))
    log, (uids, U), (iids, I), rf = wals_run(tmp_path, u, i, v, k, "--recommend_users=" + ufile,
                                             tag="l")
    recs = read_recs(rf)
    assert by_user(recs)[0] == known
    assert "1 requested user ids are not in the training data" in log
    check_against_factors(recs, uids, U, iids, I, train, 5, k, users=known)


def test_bpr_cli_recommendations_with_biases(tmp_path):
    u, i, v = synth(300, 120, 4000, seed=6)   # values 1..5: every pair is a positive
    k = 16
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    uf, itf, rf = (str(tmp_path / x) for x in ("U.txt", "I.txt", "R.txt"))
    run("bpr", "--train_dataset=" + data, "--nfactors=%d" % k, "--nepochs=2", "--use_biases",
        "--init_distribution_bound=0.1", "--seed=5", "--user_factors=" + uf,
        "--item_factors=" + itf, "--user_recommendations=" + rf, "--num_recommendations=5")
    uids, U = read_factors(uf)
    iids, b, I = read_factors(itf, biases=True)
    check_against_factors(read_recs(rf), uids, U, iids, I, train_sets(u, i), 5, k, bias=b)


@pytest.mark.parametrize("exe", ["wals", "bpr"])
def test_cli_without_the_flags_writes_no_recommendations(tmp_path, exe):
    u, i, v = synth(60, 40, 300, seed=2)
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    before = set(os.listdir(tmp_path))
    run(exe, "--train_dataset=" + data, "--nfactors=8", "--nepochs=1",
        "--user_factors=" + str(tmp_path / "U"), "--item_factors=" + str(tmp_path / "I"))
    assert set(os.listdir(tmp_path)) - before == {"U", "I"}


def test_cli_rejects_a_recommendation_count_out_of_range(tmp_path):
    u, i, v = load_tiny()
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    r = subprocess.run([os.path.join(BIN, "wals"), "--train_dataset=" + data, "--nfactors=8",
                        "--nepochs=1", "--user_recommendations=" + str(tmp_path / "R"),
                        "--num_recommendations=129"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--num_recommendations must be in 1..128" in r.stderr
