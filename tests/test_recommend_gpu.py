"""Top-N recommendations on the device (qmfx_recommend, csrc/recommend.hip) against numpy.

Bar: exact.  The device scores are the reference's double scores bit for bit
(pyoracle.test_scores) and the order (score descending, then item index ascending) is total,
so every user's list is uniquely defined: items, scores (bit for bit) and counts must equal
the numpy reference (test_recommend.topn_reference), no tolerance.  Covers fp32 and fp64
contexts, k up to 256 (several LDS column stages), item biases, exact score ties inside a
tile and across chunks, ragged last tiles, users beyond one wave and one workgroup, repeated
and unsorted requests, seen lists from the WALS CSR (a duplicate pair, a user with 2,600 seen
items) and from the BPR positives, adversarial score orders (every item beats the threshold;
none does; all equal), chunks of several tiles, short lists, sharded contexts, user batches,
agreement with qmfx_eval_ranks, and the error returns.
"""
import functools

import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from test_recommend import topn_reference

pytestmark = pytest.mark.gpu

ALL, SIGNALS, POSITIVES = 0, 1, 2


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _factors(rng, nu, ni, k, prec, bias):
    U = rng.normal(0, 0.3, (nu, k))
    I = rng.normal(0, 0.3, (ni, k))
    I[7] = I[3]            # exact ties inside a tile ...
    I[11] = I[3]
    I[ni - 1] = I[3]       # ... and across chunks
    b = rng.normal(0, 0.5, ni) if bias else None
    if bias:
        b[7] = b[11] = b[ni - 1] = b[3]
    if prec == 32:  # the device stores fp32: the reference scores those same values
        U, I = _f32(U), _f32(I)
        b = _f32(b) if bias else None
    return U, I, b


def _pairs(rng, nu, ni, nnz, dense=None):
    """(user, item) pairs in which every user and every item occurs (so ids are indices after
    group_signals), with one duplicate pair; `dense` = (user, count) adds a heavy user."""
    u = np.concatenate([np.arange(nu), rng.integers(0, nu, ni), rng.integers(0, nu, nnz)])
    i = np.concatenate([rng.integers(0, ni, nu), np.arange(ni), rng.integers(0, ni, nnz)])
    if dense:
        du, dn = dense
        u = np.concatenate([u, np.full(dn, du)])
        i = np.concatenate([i, rng.choice(ni, dn, replace=False)])
    u = np.concatenate([u, u[:1]]).astype(np.int64)   # a duplicate pair
    i = np.concatenate([i, i[:1]]).astype(np.int64)
    return u, i


def _seen(u, i, users):
    return [np.unique(i[u == t]) for t in users]


def _request(rng, nu, n):
    """n distinct users in random order plus two repeated ones (one of them once more where
    the length would be a multiple of the 8 users of a wave)."""
    req = rng.choice(nu, n, replace=False)
    req = np.concatenate([req, req[[1, 0]]])
    if len(req) % 8 == 0:
        req = np.concatenate([req, req[:1]])
    return req.astype(np.int64)


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("items", "scores", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("prec,k,bias,ni,nreq,topn,excl", [
    (64, 16, False, 500, 40, 10, ALL),
    (32, 30, True, 777, 33, 7, SIGNALS),
    (64, 130, True, 300, 20, 128, SIGNALS),
    (32, 256, False, 1000, 17, 1, ALL),
    (64, 64, False, 5000, 70, 50, SIGNALS),
])
def test_recommend_matches_numpy(prec, k, bias, ni, nreq, topn, excl):
    rng = np.random.default_rng(k + ni)
    nu = 200
    U, I, b = _factors(rng, nu, ni, k, prec, bias)
    req = _request(rng, nu, nreq)
    assert len(req) % 8 != 0
    dense = (int(req[3]), 2600) if ni == 5000 else None
    pu, pi = _pairs(rng, nu, ni, 3000, dense)
    with qmf_amd.Context(k, prec) as c:
        if excl == SIGNALS:
            uids, iids = c.group_signals(pu, pi, np.ones(len(pu)))
            assert np.array_equal(uids, np.arange(nu)) and np.array_equal(iids, np.arange(ni))
        else:
            c.set_shape(nu, ni)
        c.set_factors(0, U)
        c.set_factors(1, I)
        if bias:
            c.bpr_set_biases(b)
        got = c.recommend(req, topn, excl, use_biases=bias)
    seen = _seen(pu, pi, req) if excl == SIGNALS else None
    if dense:
        assert len(seen[3]) >= 2600
    _assert_equal(got, topn_reference(po.test_scores(U, I, req, b), topn, seen))


@pytest.mark.parametrize("topn", [5, 128])
@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
def test_recommend_adversarial_score_order(order, topn):
    """score(u, i) = ±i or 0: every later item beats the threshold (the most prunes), none
    does after the first N, or the index alone orders the items."""
    k, ni, nu = 8, 4099, 9
    U = np.zeros((nu, k))
    U[:, 0] = 1.0
    I = np.zeros((ni, k))
    I[:, 0] = {"ascending": np.arange(ni), "descending": -np.arange(ni),
               "equal": np.zeros(ni)}[order]
    req = np.arange(nu, dtype=np.int64)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nu, ni)
        c.set_factors(0, U)
        c.set_factors(1, I)
        got = c.recommend(req, topn)
    _assert_equal(got, topn_reference(po.test_scores(U, I, req), topn))


@functools.lru_cache(maxsize=None)
def _many_users_case():
    """50 users requested 4,203 times over 8,000 items: 132 user groups leave 25 item chunks
    of 5 tiles, so a workgroup carries thresholds, seen-list cursors and prunes from tile to
    tile (with few groups every chunk is a single tile)."""
    rng = np.random.default_rng(77)
    nu, ni, k = 50, 8000, 8
    U = rng.normal(0, 0.3, (nu, k))
    I = rng.normal(0, 0.3, (ni, k))
    U[:10] = 0.0
    U[:10, 0] = 1.0
    I[:, 0] = np.arange(ni) / 64.0   # users 0..9 score ascending: every tile beats the last
    I[4000:4100] = I[100]            # ties across tiles and chunks
    pu, pi = _pairs(rng, nu, ni, 20000, dense=(4, 5000))
    req = np.concatenate([rng.integers(0, nu, 4200), [0, 4, 4]]).astype(np.int64)
    S = po.test_scores(U, I, np.arange(nu))
    for a in (U, I, pu, pi, req, S):
        a.setflags(write=False)
    return nu, ni, k, U, I, pu, pi, req, S


@pytest.mark.parametrize("topn,excl", [(128, SIGNALS), (3, SIGNALS), (100, ALL)])
def test_recommend_chunks_of_several_tiles(topn, excl):
    nu, ni, k, U, I, pu, pi, req, S = _many_users_case()
    with qmf_amd.Context(k, 64) as c:
        c.group_signals(pu, pi, np.ones(len(pu)))
        c.set_factors(0, U)
        c.set_factors(1, I)
        got = c.recommend(req, topn, excl)
    seen = _seen(pu, pi, range(nu)) if excl == SIGNALS else None
    ri, rs, rc = topn_reference(S, topn, seen)
    _assert_equal(got, (ri[req], rs[req], rc[req]))


def test_recommend_short_lists():
    """Fewer eligible items than N: the count says how many, the tail is -1 / 0.0."""
    rng = np.random.default_rng(5)
    nu, ni, k, topn = 4, 50, 12, 128
    U, I = rng.normal(0, 0.3, (nu, k)), rng.normal(0, 0.3, (ni, k))
    # user 0 has seen nothing, user 1 all but items 4, 17, 49, user 2 everything, user 3 item 0
    rows = [np.array([], np.int64), np.setdiff1d(np.arange(ni), [4, 17, 49]), np.arange(ni),
            np.array([0])]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col = np.concatenate(rows)
    req = np.arange(nu, dtype=np.int64)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nu, ni)
        c.upload_csr(0, rowptr, col, np.ones(len(col)))
        c.set_factors(0, U)
        c.set_factors(1, I)
        got_all = c.recommend(req, topn, ALL)
        got = c.recommend(req, topn, SIGNALS)
    S = po.test_scores(U, I, req)
    _assert_equal(got_all, topn_reference(S, topn))
    assert got_all[2].tolist() == [50] * 4
    assert np.all(got_all[0][:, 50:] == -1) and np.all(got_all[1][:, 50:] == 0.0)
    _assert_equal(got, topn_reference(S, topn, rows))
    assert got[2].tolist() == [50, 3, 0, 49]
    assert sorted(got[0][1, :3].tolist()) == [4, 17, 49]
    assert np.all(got[0][2] == -1) and np.all(got[1][2] == 0.0)


def test_recommend_bpr_positives_with_biases():
    rng = np.random.default_rng(64)
    nu, ni, k, topn = 90, 600, 64, 20
    U, I, b = _factors(rng, nu, ni, k, 64, True)
    pu, pi = _pairs(rng, nu, ni, 4000)
    req = _request(rng, nu, 25)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nu, ni)
        c.bpr_set_positives(pu, pi)
        c.set_factors(0, U)
        c.set_factors(1, I)
        c.bpr_set_biases(b)
        got = c.recommend(req, topn, POSITIVES, use_biases=True)
    _assert_equal(got, topn_reference(po.test_scores(U, I, req, b), topn, _seen(pu, pi, req)))


def test_recommend_on_sharded_contexts():
    """Three ranks without a communicator: each recommends its own users with their signals
    left out; together they give the unsharded answer bit for bit.  A user of another rank
    is an error there; exclude = all works on any rank (the factors are replicas)."""
    rng = np.random.default_rng(3)
    nu, ni, k, topn = 300, 400, 32, 12
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    pu, pi = _pairs(rng, nu, ni, 5000)

    def ctx():
        c = qmf_amd.Context(k, 64)
        c.group_signals(pu, pi, np.ones(len(pu)))
        c.set_factors(0, U)
        c.set_factors(1, I)
        return c

    everyone = np.arange(nu, dtype=np.int64)
    with ctx() as c:
        rowptr = c.download_csr(0)[0]
        whole = c.recommend(everyone, topn, SIGNALS)
        whole_all = c.recommend(everyone[::7], topn, ALL)
    _assert_equal(whole, topn_reference(po.test_scores(U, I, everyone), topn,
                                        _seen(pu, pi, everyone)))
    parts = []
    for rank in range(3):
        lo, hi = qmf_amd.partition_rows(rowptr, 3, rank)
        with ctx() as c:
            c.dist_init(rank, 3, None)
            parts.append(c.recommend(everyone[lo:hi], topn, SIGNALS))
            outside = (hi % nu) if rank < 2 else 0
            with pytest.raises(qmf_amd.QmfxError):
                c.recommend(np.array([outside]), topn, SIGNALS)
            _assert_equal(c.recommend(everyone[::7], topn, ALL), whole_all)
    _assert_equal([np.concatenate([p[j] for p in parts]) for j in range(3)], whole)


@pytest.mark.parametrize("batch_groups", ["1", "3"])
def test_recommend_user_batches_equal_one_launch(batch_groups, monkeypatch):
    """Users beyond one launch's grid run in batches of QMFX_EVAL_BATCH_GROUPS groups; batches
    of 1 and 3 groups on 150 users (5 groups, a ragged last one) give the same lists."""
    rng = np.random.default_rng(9)
    nu, ni, k, topn = 400, 900, 48, 20
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    pu, pi = _pairs(rng, nu, ni, 6000)
    req = rng.choice(nu, 150, replace=False).astype(np.int64)
    out = []
    for env in (None, batch_groups):
        if env:
            monkeypatch.setenv("QMFX_EVAL_BATCH_GROUPS", env)
        with qmf_amd.Context(k, 64) as c:
            c.group_signals(pu, pi, np.ones(len(pu)))
            c.set_factors(0, U)
            c.set_factors(1, I)
            out.append(c.recommend(req, topn, SIGNALS))
    _assert_equal(out[1], out[0])
    _assert_equal(out[0], topn_reference(po.test_scores(U, I, req), topn, _seen(pu, pi, req)))


def test_recommend_agrees_with_eval_ranks():
    """The item recommended at rank r has exactly r items scored above it (tie-free scores)."""
    rng = np.random.default_rng(21)
    nu, ni, k, topn = 60, 700, 24, 15
    U, I = rng.normal(0, 0.3, (nu, k)), rng.normal(0, 0.3, (ni, k))
    req = rng.choice(nu, 21, replace=False).astype(np.int64)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nu, ni)
        c.set_factors(0, U)
        c.set_factors(1, I)
        items, scores, counts = c.recommend(req, topn)
        assert counts.tolist() == [topn] * len(req)
        rowptr = np.arange(len(req) + 1, dtype=np.int64) * topn
        c.eval_set_labels(req, rowptr, items.ravel(), np.ones(items.size))
        ls, above, _ = c.eval_ranks()
    assert np.array_equal(ls, scores.ravel())
    assert np.array_equal(above.reshape(len(req), topn), np.tile(np.arange(topn), (len(req), 1)))


def test_recommend_errors_leave_the_context_usable():
    rng = np.random.default_rng(1)
    nu, ni, k = 20, 100, 8
    U, I = rng.normal(0, 0.3, (nu, k)), rng.normal(0, 0.3, (ni, k))
    req = np.arange(5, dtype=np.int64)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nu, ni)
        c.set_factors(0, U)
        c.set_factors(1, I)
        for args in [(req, 0), (req, 129), (np.array([nu]), 5), (req, 5, SIGNALS),
                     (req, 5, POSITIVES), (req, 5, ALL, True)]:
            with pytest.raises(qmf_amd.QmfxError) as e:
                c.recommend(*args)
            assert str(e.value).split(": ", 1)[1].strip(), args
            _assert_equal(c.recommend(req, 5), topn_reference(po.test_scores(U, I, req), 5))
        items, scores, counts = c.recommend(np.array([], np.int64), 5)
        assert items.shape == (0, 5) and scores.shape == (0, 5) and counts.shape == (0,)
