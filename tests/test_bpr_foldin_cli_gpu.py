"""--fold_in_dataset / --fold_in_user_factors / --fold_in_recommendations / --fold_in_epochs of
the `bpr` CLI on the MI355X, on tests/golden/tiny.txt.

The fold-in file repeats three training users' positive lines under new ids, in shuffled line
order with one line doubled, plus one line naming an item the model does not know and one line
of value 0 on a known item.  The expected rows come from Context.bpr_fold_in with the run's
schedule and the sampling seed the engine logs, on the item factors of the run's --item_factors
file.  That file rounds every factor to 9 decimals, so the item rows the ABI call sees differ
from the CLI's by at most 5e-10 per element and (q_p - q_n) by at most 1e-9; a step moves p by
lr * eg * (q_p - q_n) with eg < 1, so after s steps the rows differ by at most s * lr * 1e-9,
times 1.5 for the second-order terms (eg's own change is below 0.25 * k * max|p| * 1e-9), plus
the 5e-10 of the written row itself:

    |x_file - x_abi| <= 5e-10 + 1.5e-9 * lr * epochs * num_neg * (the user's items)."""
import re

import numpy as np
import pytest

import qmf_amd
from helpers import load_tiny
from test_cli_gpu import read_factors, run, write_dataset
from test_recommend_cli_gpu import by_user, check_against_factors, read_recs

pytestmark = pytest.mark.gpu

K, EPOCHS, FOLD_EPOCHS, TOPN = 8, 3, 5, 4
LR, DECAY, USER_LAMBDA, NUM_NEG = 0.05, 0.9, 0.025, 3   # the CLI's defaults
NEW_ID = 7_000_000_000_000   # past every id of the fixture
UNKNOWN_ITEM = 123_456_789


def fold_lines():
    """(users, items, values) of the fold-in file and {new id: set of known positive item ids}."""
    u, i, v = load_tiny()
    pos = v >= 1.0
    known = set(i[pos].tolist())
    uids = np.unique(u[pos])
    picked = [int(uids[0]), int(uids[len(uids) // 2]), int(uids[-1])]
    fu, fi, fv, own = [], [], [], {}
    for n, old in enumerate(picked):
        m = (u == old) & pos
        new = NEW_ID + 10 * (len(picked) - n)   # descending ids in the file
        fu += [new] * int(m.sum())
        fi += i[m].tolist()
        fv += v[m].tolist()
        own[new] = set(i[m].tolist())
    fu.append(fu[0]), fi.append(fi[0]), fv.append(fv[0])        # a doubled line
    order = np.random.default_rng(2).permutation(len(fu))
    fu, fi, fv = (np.array(x)[order].tolist() for x in (fu, fi, fv))
    first = fu[0]
    fu.append(first), fi.append(UNKNOWN_ITEM), fv.append(1.0)   # dropped with the warning
    zero_item = sorted(known - own[first])[0]
    fu.append(first), fi.append(zero_item), fv.append(0.0)      # value < 1: dropped silently
    return (np.array(fu, np.int64), np.array(fi, np.int64), np.array(fv, np.float64)), own


def cli(tmp_path, tag, *extra, fold=True):
    u, i, v = load_tiny()
    data, foldf = str(tmp_path / "train.txt"), str(tmp_path / "fold.txt")
    write_dataset(data, u, i, v)
    write_dataset(foldf, *fold_lines()[0])
    out = {x: str(tmp_path / (tag + x + ".txt")) for x in ("U", "I", "FU", "FR")}
    flags = ["--train_dataset=" + data, "--nfactors=%d" % K, "--nepochs=%d" % EPOCHS, "--seed=5",
             "--user_factors=" + out["U"], "--item_factors=" + out["I"]]
    if fold:
        flags += ["--fold_in_dataset=" + foldf, "--fold_in_user_factors=" + out["FU"],
                  "--fold_in_recommendations=" + out["FR"], "--num_recommendations=%d" % TOPN]
    return run("bpr", *flags, *extra), out


def abi_rows(out, seed, epochs, own):
    """Context.bpr_fold_in on the run's item factor file: (new ids ascending, rows, steps)."""
    iids, I = read_factors(out["I"])
    idx = {int(x): n for n, x in enumerate(iids)}
    ids = sorted(own)
    cols = [np.sort([idx[x] for x in own[n]]) for n in ids]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    with qmf_amd.Context(K, 64) as c:
        c.set_shape(len(ids), len(iids))
        c.set_factors(1, I)
        F, _ = c.bpr_fold_in(rowptr, np.concatenate(cols), seed, epochs, NUM_NEG, LR, DECAY,
                             USER_LAMBDA)
    return np.array(ids), F, epochs * NUM_NEG * np.diff(rowptr)


@pytest.mark.parametrize("fold_epochs", [None, FOLD_EPOCHS])
def test_cli_fold_in_factors_and_recommendations(tmp_path, fold_epochs):
    extra = [] if fold_epochs is None else ["--fold_in_epochs=%d" % fold_epochs]
    log, out = cli(tmp_path, "a", *extra)
    epochs = fold_epochs or EPOCHS   # the default is --nepochs
    _, own = fold_lines()
    assert "1 fold-in lines name items that are not in the training data; dropped" in log
    m = re.search(r"fold-in: 3 users, (\d+) epochs, sampling seed (\d+)", log)
    assert m and int(m.group(1)) == epochs
    ids, F, steps = abi_rows(out, int(m.group(2)), epochs, own)
    fids, FU = read_factors(out["FU"])
    assert np.array_equal(fids, ids) and FU.shape == F.shape == (3, K)
    bound = 5e-10 + 1.5e-9 * LR * steps[:, None]
    print("BPR fold-in cli epochs=%d: max |x_file - x_abi| = %.3g (bound %.3g), max|x| %.3g"
          % (epochs, np.abs(FU - F).max(), bound.min(), np.abs(F).max()))
    assert np.all(np.abs(FU - F) <= bound)
    assert np.abs(F).max() > 1e-4   # the rows moved
    # recommendations: the new users ascending, rank order, none of the user's own items, the
    # value-0 item still eligible; scores of the written factors
    iids, I = read_factors(out["I"])
    recs = read_recs(out["FR"])
    assert by_user(recs)[0] == ids.tolist()
    check_against_factors(recs, fids, FU, iids, I, own, TOPN, K)


def test_cli_fold_in_recommend_seen_and_timing(tmp_path, monkeypatch):
    monkeypatch.setenv("QMF_TIMINGS", "1")
    log, out = cli(tmp_path, "s", "--recommend_seen")
    assert "timing: fold_in " in log and " 3 users" in log
    _, own = fold_lines()
    fids, FU = read_factors(out["FU"])
    iids, I = read_factors(out["I"])
    recs = read_recs(out["FR"])
    check_against_factors(recs, fids, FU, iids, I, None, TOPN, K)
    assert any(it in own[x] for x, it, _ in recs), "no own item among the recommendations"


def test_cli_trained_model_is_the_same_with_and_without_fold_in(tmp_path):
    _, with_fold = cli(tmp_path, "w")
    _, without = cli(tmp_path, "n", fold=False)
    for x in ("U", "I"):
        assert open(with_fold[x], "rb").read() == open(without[x], "rb").read()
