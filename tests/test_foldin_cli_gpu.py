"""--fold_in_dataset / --fold_in_user_factors / --fold_in_recommendations of the `wals` CLI on
the MI355X, on tests/golden/tiny.txt.

The fold-in file repeats three training users' lines under new ids (plus one line naming an
item the model does not know).  The expected rows come from the same fold-in through the C ABI
on a context trained the same way: the CLI's training is a fixed sequence of ABI calls
(qmfx_group_signals, the item factors of --distribution_file, a user half and an item half per
epoch), so the context holds the CLI's item factors bit for bit.  The file rounds every factor
to 9 decimals, so a row is held to the project's bar plus that rounding:

    |x_file − x_abi| ≤ bar·‖x_abi‖∞ + 5e-10,   bar = 1e-9 (fp64) or 1e-4 (fp32).

The recommendation file is checked against the factor files of the same run with the bound of
tests/test_recommend_cli_gpu.py (each factor off by at most 5e-10)."""
import numpy as np
import pytest

import qmf_amd
from helpers import load_tiny
from test_cli_gpu import read_factors, run, write_dataset, write_dist
from test_foldin import bars
from test_recommend_cli_gpu import by_user, err, read_recs

pytestmark = pytest.mark.gpu

K, EPOCHS, ALPHA, LAM, TOPN = 8, 2, 40.0, 0.05, 5
NEW_ID = 7_000_000_000_000   # past every id of the fixture
UNKNOWN_ITEM = 123_456_789


def fold_lines(u, i, v):
    """Three training users' lines under new ids, in shuffled line order."""
    uids = np.unique(u)
    picked = [int(uids[0]), int(uids[len(uids) // 2]), int(uids[-1])]
    fu, fi, fv = [], [], []
    for n, old in enumerate(picked):
        m = u == old
        fu += [NEW_ID + 10 * (len(picked) - n)] * int(m.sum())   # descending ids in the file
        fi += i[m].tolist()
        fv += v[m].tolist()
    order = np.random.default_rng(2).permutation(len(fu))
    return (np.array(fu, np.int64)[order], np.array(fi, np.int64)[order],
            np.array(fv, np.float64)[order])


def cli_fold_in(tmp_path, precision, *extra):
    u, i, v = load_tiny()
    fu, fi, fv = fold_lines(u, i, v)
    data, fold, dist = (str(tmp_path / x) for x in ("train.txt", "fold.txt", "dist.dat"))
    write_dataset(data, u, i, v)
    write_dataset(fold, fu, fi, fv)
    with open(fold, "a") as f:
        f.write("%d %d 1.0\n" % (fu[0], UNKNOWN_ITEM))
    ni = len(np.unique(i))
    write_dist(dist, np.random.default_rng(K).uniform(-0.01, 0.01, (ni, K)))
    init = np.array([float(x) for x in open(dist).read().split()]).reshape(ni, K)
    out = {x: str(tmp_path / (x + ".txt")) for x in ("U", "I", "FU", "FR")}
    log = run("wals", "--train_dataset=" + data, "--nfactors=%d" % K, "--nepochs=%d" % EPOCHS,
              "--distribution_file=" + dist, "--precision=%d" % precision,
              "--user_factors=" + out["U"], "--item_factors=" + out["I"],
              "--fold_in_dataset=" + fold, "--fold_in_user_factors=" + out["FU"],
              "--fold_in_recommendations=" + out["FR"], "--num_recommendations=%d" % TOPN, *extra)
    return log, (u, i, v), (fu, fi, fv), init, out


def abi_fold_in(train, fold, init, precision):
    """The same training and fold-in through the ABI: (new ids ascending, rows, item ids)."""
    u, i, v = train
    fu, fi, fv = fold
    with qmf_amd.Context(K, precision) as c:
        uids, iids = c.group_signals(u, i, v)
        c.set_factors(0, np.zeros((len(uids), K)))
        c.set_factors(1, init)
        for _ in range(EPOCHS):
            c.wals_half(0, ALPHA, LAM)
            c.wals_half(1, ALPHA, LAM)
        ids = np.unique(fu)
        col = np.searchsorted(iids, fi)
        order = np.lexsort((col, fu))   # by new id, then item idx
        rowptr = np.concatenate([[0], np.cumsum([np.sum(fu == x) for x in ids])])
        F, _, _ = c.wals_fold_in(0, rowptr, col[order], fv[order], ALPHA, LAM)
    return ids, F, iids


@pytest.mark.parametrize("precision", [64, 32])
def test_cli_fold_in_factors_and_recommendations(tmp_path, precision):
    log, train, fold, init, out = cli_fold_in(tmp_path, precision)
    assert "1 fold-in lines name items that are not in the training data; dropped" in log
    ids, F, iids = abi_fold_in(train, fold, init, precision)
    fids, FU = read_factors(out["FU"])
    assert np.array_equal(fids, ids) and FU.shape == F.shape == (3, K)
    bar = bars(precision)[0]
    excess = np.abs(FU - F) - (bar * np.max(np.abs(F), axis=1, keepdims=True) + 5e-10)
    print("FOLDIN cli p=%d max |x_file - x_abi| = %.3g, ‖x‖∞ ≥ %.3g"
          % (precision, np.abs(FU - F).max(), np.max(np.abs(F), axis=1).min()))
    assert excess.max() <= 0.0, excess.max()
    # the trained model's files are what they are without the fold-in flags' rows
    tuids, _ = read_factors(out["U"])
    assert np.array_equal(tuids, np.unique(train[0]))
    # recommendations: the new users ascending, no item of the user's own lines, scores of
    # the file factors, nothing eligible left out that beats the last line
    iid2, I = read_factors(out["I"])
    assert np.array_equal(iid2, iids)
    users, lists = by_user(read_recs(out["FR"]))
    assert users == ids.tolist()
    fu, fi, _ = fold
    for r, uid in enumerate(users):
        seen = set(fi[fu == uid].tolist())
        got = lists[uid]
        assert len(got) == min(TOPN, len(iids) - len(seen)), uid
        ws = [w for _, w in got]
        assert all(a >= b for a, b in zip(ws, ws[1:]))
        dots = I @ FU[r]
        es = np.array([err(FU[r], q, K) for q in I])
        pos = {int(x): n for n, x in enumerate(iids)}
        for it, w in got:
            assert it not in seen, (uid, it)
            assert abs(w - dots[pos[it]]) <= es[pos[it]], (uid, it, w, dots[pos[it]])
        rest = np.array([n for x, n in pos.items() if x not in seen and x not in {a for a, _ in got}],
                        np.int64)
        if len(rest) and len(got) == TOPN:
            assert np.all(dots[rest] <= got[-1][1] + es[rest] + es[pos[got[-1][0]]]), uid


def test_cli_fold_in_recommend_seen_and_timing(tmp_path, monkeypatch):
    monkeypatch.setenv("QMF_TIMINGS", "1")
    log, train, fold, init, out = cli_fold_in(tmp_path, 64, "--recommend_seen")
    assert "timing: fold_in " in log and " 3 users, " in log
    users, lists = by_user(read_recs(out["FR"]))
    fu, fi, _ = fold
    ni = len(np.unique(train[1]))
    assert all(len(lists[x]) == min(TOPN, ni) for x in users)
    assert any(it in set(fi[fu == x].tolist()) for x in users for it, _ in lists[x]), \
        "no item of a user's own lines among the recommendations"


def test_cli_fold_in_outputs_need_the_dataset(tmp_path):
    import os
    import subprocess
    from test_cli_gpu import BIN
    u, i, v = load_tiny()
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    r = subprocess.run([os.path.join(BIN, "wals"), "--train_dataset=" + data, "--nfactors=8",
                        "--nepochs=1", "--fold_in_user_factors=" + str(tmp_path / "FU")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "need --fold_in_dataset" in r.stderr
