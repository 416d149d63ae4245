"""--recommend_exclude_items / --recommend_items / --recommend_candidates of the drop-in CLIs
(`wals`, `bpr`) on the MI355X, on a small trained model.

Each recommendation file is checked the way test_recommend_cli_gpu.py checks one: against the
factor files of the same run, with its derived bound for their 9 decimals
(check_against_factors), the catalogue being the items the flag leaves eligible: every user has
min(N, eligible) lines in rank order, none of them a training item, the printed scores are the
file factors' scores, and no eligible item left out beats a user's last line.  Ids the model
does not know are skipped with one warning carrying their count."""
import numpy as np
import pytest

from helpers import synth
from test_cli_gpu import read_factors, run, write_dataset
from test_explain_cli_gpu import read_explanations
from test_recommend_cli_gpu import by_user, check_against_factors, read_recs, train_sets

pytestmark = pytest.mark.gpu

K, TOPN = 8, 5
UNKNOWN = 10**6  # an id no line of the training data carries


def _train(tmp_path):
    u, i, v = synth(60, 40, 600, seed=2)
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    return u, i, v, data


def _run(exe, tmp_path, data, tag, *extra):
    uf, itf, rf = (str(tmp_path / (tag + x)) for x in ("U.txt", "I.txt", "R.txt"))
    model = ["--nfactors=%d" % K, "--nepochs=2", "--user_factors=" + uf, "--item_factors=" + itf,
             "--user_recommendations=" + rf, "--num_recommendations=%d" % TOPN]
    if exe == "bpr":
        model += ["--use_biases", "--init_distribution_bound=0.1", "--seed=5"]
    log = run(exe, "--train_dataset=" + data, *model, *extra)
    uids, U = read_factors(uf)
    if exe == "bpr":
        iids, b, I = read_factors(itf, biases=True)
    else:
        (iids, I), b = read_factors(itf), None
    return log, uids, U, iids, b, I, read_recs(rf)


def _write_ids(path, ids):
    with open(path, "w") as f:
        f.write("".join("%d\n" % x for x in ids))
    return str(path)


def _check(recs, uids, U, iids, b, I, train, keep, users=None):
    """check_against_factors with the catalogue cut down to the item ids in `keep`."""
    m = np.isin(iids, list(keep))
    check_against_factors(recs, uids, U, iids[m], I[m], train, TOPN, K,
                          bias=None if b is None else b[m], users=users)


@pytest.mark.parametrize("exe", ["wals", "bpr"])
def test_cli_item_scopes(tmp_path, exe):
    u, i, v, data = _train(tmp_path)
    train = train_sets(u, i)
    items = np.unique(i)
    rng = np.random.default_rng(3)
    some = rng.choice(items, 15, replace=False)
    # unsorted, with a repeat and two unknown ids
    listed = np.concatenate([some, some[:2], [UNKNOWN, UNKNOWN + 1]])
    users = [int(x) for x in np.unique(u)[[7, 2, 30]]]
    ifile = _write_ids(tmp_path / "items.txt", listed)
    ufile = _write_ids(tmp_path / "users.txt", users)

    log, uids, U, iids, b, I, recs = _run(exe, tmp_path, data, "d",
                                          "--recommend_exclude_items=" + ifile)
    assert log.count("2 requested item ids are not in the training data") == 1
    assert not {it for _, it, _ in recs} & set(some.tolist())
    _check(recs, uids, U, iids, b, I, train, set(items.tolist()) - set(some.tolist()))

    log, uids, U, iids, b, I, recs = _run(exe, tmp_path, data, "a", "--recommend_items=" + ifile)
    assert log.count("2 requested item ids are not in the training data") == 1
    assert {it for _, it, _ in recs} <= set(some.tolist())
    _check(recs, uids, U, iids, b, I, train, set(some.tolist()))

    # both combine with --recommend_users and --recommend_seen
    for flag, keep in (("--recommend_items=", set(some.tolist())),
                       ("--recommend_exclude_items=", set(items.tolist()) - set(some.tolist()))):
        log, uids, U, iids, b, I, recs = _run(exe, tmp_path, data, "u", flag + ifile,
                                              "--recommend_users=" + ufile, "--recommend_seen")
        assert by_user(recs)[0] == users
        _check(recs, uids, U, iids, b, I, None, keep, users=users)


@pytest.mark.parametrize("exe", ["wals", "bpr"])
def test_cli_per_user_candidates(tmp_path, exe):
    u, i, v, data = _train(tmp_path)
    train = train_sets(u, i)
    items, allusers = np.unique(i), np.unique(u)
    rng = np.random.default_rng(4)
    cands = {int(x): rng.choice(items, n, replace=False).tolist()
             for x, n in zip(rng.choice(allusers, 12, replace=False), rng.integers(1, 30, 12))}
    first = next(iter(cands))
    cands[first] = sorted(train[first])[:3]       # a user whose candidates are all seen
    lines = [(uu, it) for uu, l in cands.items() for it in l]
    lines += lines[:3]                            # repeated lines
    lines += [(UNKNOWN, int(items[0])), (first, UNKNOWN), (UNKNOWN, UNKNOWN)]
    order = rng.permutation(len(lines))
    cfile = str(tmp_path / "cands.txt")
    write_dataset(cfile, [lines[j][0] for j in order], [lines[j][1] for j in order],
                  np.ones(len(lines)))

    for seen_flag in ((), ("--recommend_seen",)):
        log, uids, U, iids, b, I, recs = _run(exe, tmp_path, data, "c",
                                              "--recommend_candidates=" + cfile, *seen_flag)
        assert log.count("3 candidate lines name a user or item id that is not in the training "
                         "data") == 1
        tr = None if seen_flag else train
        got_users, lists = by_user(recs)
        # the file's known users in ascending idx (the factor file's order), those with an
        # eligible candidate
        want_users = [int(x) for x in uids
                      if int(x) in cands and (set(cands[int(x)]) - (tr[int(x)] if tr else set()))]
        assert got_users == want_users
        assert (first in got_users) == bool(seen_flag)
        for uu in got_users:
            mine = [r for r in recs if r[0] == uu]
            _check(mine, uids, U, iids, b, I, tr, set(cands[uu]), users=[uu])


def test_cli_explains_the_pairs_of_a_scoped_file(tmp_path):
    u, i, v, data = _train(tmp_path)
    some = np.random.default_rng(3).choice(np.unique(i), 15, replace=False)
    ifile = _write_ids(tmp_path / "items.txt", some)
    ef = str(tmp_path / "E.txt")
    log, uids, U, iids, b, I, recs = _run("wals", tmp_path, data, "e", "--recommend_items=" + ifile,
                                          "--recommendation_explanations=" + ef,
                                          "--num_explanations=2")
    assert recs and {it for _, it, _ in recs} <= set(some.tolist())
    nlines = {int(x): int(np.sum(u == x)) for x in np.unique(u)}
    want = [(uu, it) for uu, it, _ in recs for _ in range(min(2, nlines[uu]))]
    assert [(e[0], e[1]) for e in read_explanations(ef)] == want
