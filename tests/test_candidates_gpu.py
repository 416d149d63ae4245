"""Recommending within candidate sets on the device (qmfx_recommend_without,
qmfx_recommend_candidates, csrc/recommend.hip) against numpy.

Bar: exact, as in test_recommend_gpu.py.  The scores are qmfx_recommend's bit for bit and the
order is total, so items, scores and counts must equal test_recommend.topn_reference on
pyoracle.test_scores with, as the seen set, the complement of the user's list (a candidate
call) or the deny items (a deny call), united with the user's seen items.  No tolerance.

Covers both list forms (one shared list; per-user lists), list lengths around the tile (64),
the prune edge (192 / 193 entries in a list), topn and the chunk (512 candidates), ragged
lengths inside one wave and workgroup, repeated users with different lists, k at the LDS stage
edges, ties inside a tile and across chunks, signed zeros, adversarial score orders, the first
and last item, deny bits at word edges, seen lists (all seen, a heavy user, a duplicate pair),
sharded contexts, user batches, the error returns and the reported work."""
import ctypes

import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from test_candidates import CHUNK, candidate_seen, deny_seen
from test_recommend import topn_reference
from test_recommend_gpu import (ALL, POSITIVES, SIGNALS, _assert_equal, _f32, _factors, _pairs,
                                _request, _seen)

pytestmark = pytest.mark.gpu


def _lengths(topn):
    """Every list length at which the kernel takes another path."""
    return [0, 1, 63, 64, 65, topn - 1, topn, topn + 1, 192, 193, CHUNK - 1, CHUNK, CHUNK + 1,
            2 * CHUNK + 65]


def _subset(rng, ni, n):
    return np.sort(rng.choice(ni, n, replace=False)).astype(np.int64)


def _csr(lists):
    cptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    cand = np.concatenate(lists).astype(np.int64) if len(lists) else np.zeros(0, np.int64)
    return cand, cptr


def _context(k, prec, nu, ni, U, I, b=None, pairs=None, excl=ALL):
    c = qmf_amd.Context(k, prec)
    if excl == SIGNALS:
        uids, iids = c.group_signals(pairs[0], pairs[1], np.ones(len(pairs[0])))
        assert np.array_equal(uids, np.arange(nu)) and np.array_equal(iids, np.arange(ni))
    else:
        c.set_shape(nu, ni)
        if excl == POSITIVES:
            c.bpr_set_positives(pairs[0], pairs[1])
    c.set_factors(0, U)
    c.set_factors(1, I)
    if b is not None:
        c.bpr_set_biases(b)
    return c


@pytest.mark.parametrize("excl", [ALL, SIGNALS, POSITIVES])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("prec", [64, 32])
def test_identities_with_recommend(prec, bias, excl):
    """A shared list of every item and an empty deny list are qmfx_recommend; a deny list is
    the shared list of its complement."""
    rng = np.random.default_rng(prec + 2 * bias + 7 * excl)
    nu, ni, k, topn = 60, 1100, 20, 15
    U, I, b = _factors(rng, nu, ni, k, prec, bias)
    pairs = _pairs(rng, nu, ni, 3000)
    req = _request(rng, nu, 33)
    deny = rng.choice(ni, 400)  # with repeats, unsorted
    with _context(k, prec, nu, ni, U, I, b, pairs, excl) as c:
        want = c.recommend(req, topn, excl, use_biases=bias)
        everything = c.recommend_candidates(req, topn, np.arange(ni), None, excl, bias)
        nothing = c.recommend_without(req, np.zeros(0, np.int64), topn, excl, bias)
        without = c.recommend_without(req, deny, topn, excl, bias)
        within = c.recommend_candidates(req, topn, np.setdiff1d(np.arange(ni), deny), None, excl,
                                        bias)
    seen = _seen(pairs[0], pairs[1], req) if excl != ALL else None
    S = po.test_scores(U, I, req, b)
    _assert_equal(want, topn_reference(S, topn, seen))
    _assert_equal(everything, want)
    _assert_equal(nothing, want)
    _assert_equal(without, topn_reference(S, topn, deny_seen(deny, len(req), seen)))
    _assert_equal(within, without)


@pytest.mark.parametrize("prec,excl", [(64, ALL), (32, SIGNALS)])
def test_shared_list_lengths(prec, excl):
    rng = np.random.default_rng(11 + prec)
    nu, ni, k, topn = 40, 1500, 24, 20
    U, I, b = _factors(rng, nu, ni, k, prec, False)
    pairs = _pairs(rng, nu, ni, 4000)
    req = _request(rng, nu, 11)
    assert len(req) % 8 != 0
    seen = _seen(pairs[0], pairs[1], req) if excl != ALL else None
    S = po.test_scores(U, I, req)
    with _context(k, prec, nu, ni, U, I, None, pairs, excl) as c:
        for n in _lengths(topn):
            lst = _subset(rng, ni, n)
            got = c.recommend_candidates(req, topn, lst, None, excl)
            _assert_equal(got, topn_reference(S, topn, candidate_seen(ni, [lst] * len(req), seen)))
            if n == 0:
                assert got[2].tolist() == [0] * len(req) and np.all(got[0] == -1)


@pytest.mark.parametrize("prec,excl,bias", [(64, ALL, False), (32, SIGNALS, False),
                                            (64, POSITIVES, True)])
def test_per_user_ragged_list_lengths(prec, excl, bias):
    """45 requests (not a multiple of 8 or 32) of 30 users, so users repeat with different
    lists; the lengths of _lengths() in shuffled order, so one wave and one workgroup mix them."""
    rng = np.random.default_rng(5 + prec + excl)
    nu, ni, k, topn = 30, 1500, 24, 20
    U, I, b = _factors(rng, nu, ni, k, prec, bias)
    pairs = _pairs(rng, nu, ni, 4000)
    req = np.concatenate([rng.permutation(nu), rng.integers(0, nu, 15)]).astype(np.int64)
    assert len(req) == 45
    ln = _lengths(topn)
    ln = rng.permutation(ln + ln + ln + [7, 300, 700])
    assert len(ln) == len(req)
    lists = [_subset(rng, ni, n) for n in ln]
    cand, cptr = _csr(lists)
    with _context(k, prec, nu, ni, U, I, b, pairs, excl) as c:
        got = c.recommend_candidates(req, topn, cand, cptr, excl, bias)
    seen = _seen(pairs[0], pairs[1], req) if excl != ALL else None
    want = topn_reference(po.test_scores(U, I, req, b), topn, candidate_seen(ni, lists, seen))
    _assert_equal(got, want)
    assert np.array_equal(got[2], np.minimum(topn, want[2]))


@pytest.mark.parametrize("topn", [1, 128])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 130, 256])
def test_factor_counts_at_the_stage_edges(k, topn):
    rng = np.random.default_rng(k + topn)
    nu, ni = 20, 900
    prec = 32 if k % 2 else 64
    U, I, _ = _factors(rng, nu, ni, k, prec, False)
    req = _request(rng, nu, 9)
    shared = _subset(rng, ni, 700)
    lists = [_subset(rng, ni, n) for n in rng.integers(0, 800, len(req))]
    cand, cptr = _csr(lists)
    with _context(k, prec, nu, ni, U, I) as c:
        got_s = c.recommend_candidates(req, topn, shared)
        got_p = c.recommend_candidates(req, topn, cand, cptr)
    S = po.test_scores(U, I, req)
    _assert_equal(got_s, topn_reference(S, topn, candidate_seen(ni, [shared] * len(req))))
    _assert_equal(got_p, topn_reference(S, topn, candidate_seen(ni, lists)))


def test_ties_inside_a_tile_across_chunks_and_signed_zeros():
    """Duplicated item rows at list positions inside one gathered tile and in other chunks, and
    scores of -0.0 against +0.0 (bias -0.0 plus a product -0.0): the index decides."""
    rng = np.random.default_rng(8)
    nu, ni, k, topn = 12, 2000, 6, 40
    U = rng.normal(0, 0.3, (nu, k))
    I = rng.normal(0, 0.3, (ni, k))
    dup = [3, 7, 11, 40, 700, 1300, ni - 1]
    I[dup] = I[3]
    b = rng.normal(0, 0.5, ni)
    b[dup] = b[3]
    # users 0..3: every score is a zero; a -0.0 where bias and product are both -0.0
    U[:4] = 0.0
    U[:4, 0] = 1.0
    zero = np.arange(0, ni, 3)
    # (every factor of such an item is -0.0: one product of +0.0 would turn the sum into +0.0)
    Iz, bz = np.zeros((ni, k)), np.zeros(ni)
    Iz[zero] = -0.0
    bz[zero] = -0.0
    req = np.arange(nu, dtype=np.int64)
    lst = np.union1d(_subset(rng, ni, 1200), dup)
    lists = [np.union1d(_subset(rng, ni, n), dup) for n in rng.integers(600, 1400, nu)]
    cand, cptr = _csr(lists)
    for II, bb, users in ((I, b, req), (Iz, bz, req[:4])):
        with _context(k, 64, nu, ni, U, II, bb) as c:
            got_s = c.recommend_candidates(users, topn, lst, None, ALL, True)
            got_p = c.recommend_candidates(users, topn, cand, cptr[:len(users) + 1], ALL, True)
        S = po.test_scores(U, II, users, bb)
        if II is Iz:
            assert np.all(S == 0.0) and np.signbit(S[:, zero]).all() and not np.signbit(S[:, 1])[0]
        want = topn_reference(S, topn, candidate_seen(ni, [lst] * len(users)))
        _assert_equal(got_s, want)
        _assert_equal(got_p, topn_reference(S, topn, candidate_seen(ni, lists[:len(users)])))
    assert set(dup) <= set(lst)


@pytest.mark.parametrize("topn", [5, 128])
@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
def test_adversarial_score_order(order, topn):
    """Candidate scores ascending in list order (every tile beats the threshold), descending
    (none does after the first N), or all equal (the index alone orders)."""
    k, ni, nu = 8, 2000, 9
    rng = np.random.default_rng(topn)
    U = np.zeros((nu, k))
    U[:, 0] = 1.0
    I = np.zeros((ni, k))
    I[:, 0] = {"ascending": np.arange(ni), "descending": -np.arange(ni),
               "equal": np.zeros(ni)}[order]
    req = np.arange(nu, dtype=np.int64)
    lst = _subset(rng, ni, 1300)
    lists = [_subset(rng, ni, n) for n in (1300, 1025, 600, 193, 129, 128, 127, 64, 5)]
    cand, cptr = _csr(lists)
    with _context(k, 64, nu, ni, U, I) as c:
        got_s = c.recommend_candidates(req, topn, lst)
        got_p = c.recommend_candidates(req, topn, cand, cptr)
    S = po.test_scores(U, I, req)
    _assert_equal(got_s, topn_reference(S, topn, candidate_seen(ni, [lst] * nu)))
    _assert_equal(got_p, topn_reference(S, topn, candidate_seen(ni, lists)))


def test_index_edges_and_deny_words():
    """4,099 items: not a multiple of 64, several chunks of the dense scan.  Lists holding item 0
    and the last item; deny bits 63, 64 and the last item; denying everything; a deny list
    overlapping the seen lists."""
    rng = np.random.default_rng(4099)
    nu, ni, k, topn = 25, 4099, 10, 30
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    # items 0, 63, 64 and the last one rank first for everybody, so a wrong bit shows
    U[:, 0] = 1.0
    I[:, 0] = 0.0
    I[[0, 63, 64, ni - 1], 0] = 50.0
    pairs = _pairs(rng, nu, ni, 3000)
    req = _request(rng, nu, 10)
    seen = _seen(pairs[0], pairs[1], req)
    S = po.test_scores(U, I, req)
    ends = np.array([0, ni - 1])
    lists = [np.union1d(_subset(rng, ni, n), ends) for n in rng.integers(0, 900, len(req))]
    lists[0], lists[1] = ends[:1].copy(), ends[1:].copy()
    cand, cptr = _csr(lists)
    with _context(k, 64, nu, ni, U, I, None, pairs, SIGNALS) as c:
        for excl, sn in ((ALL, None), (SIGNALS, seen)):
            got = c.recommend_candidates(req, topn, cand, cptr, excl)
            _assert_equal(got, topn_reference(S, topn, candidate_seen(ni, lists, sn)))
            got = c.recommend_candidates(req, topn, ends, None, excl)
            _assert_equal(got, topn_reference(S, topn, candidate_seen(ni, [ends] * len(req), sn)))
            for deny in ([63], [64], [ni - 1], [63, 64, ni - 1], [0, 62, 65, ni - 2],
                         np.concatenate([seen[0][:5], seen[1], [64]])):
                got = c.recommend_without(req, deny, topn, excl)
                _assert_equal(got, topn_reference(S, topn, deny_seen(deny, len(req), sn)))
        got = c.recommend_without(req, np.arange(ni), topn, ALL)
        assert got[2].tolist() == [0] * len(req)
        assert np.all(got[0] == -1) and np.all(got[1] == 0.0)
        got = c.recommend_without(req, np.arange(1, ni), topn, ALL)
        assert got[2].tolist() == [1] * len(req) and np.all(got[0][:, 0] == 0)


def test_seen_lists():
    """A user whose whole list is seen, a heavy user with 2,600 seen items of which a few are
    candidates, and a duplicate training pair (the pair of _pairs)."""
    rng = np.random.default_rng(26)
    nu, ni, k, topn = 50, 5000, 12, 10
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    heavy = 4
    pu, pi = _pairs(rng, nu, ni, 2000, dense=(heavy, 2600))
    req = np.array([heavy, 9, 1, heavy, 17, int(pu[0]), 30, 2, 41], np.int64)
    seen = _seen(pu, pi, req)
    assert len(seen[0]) >= 2600
    lists = [_subset(rng, ni, n) for n in rng.integers(100, 900, len(req))]
    lists[0] = np.union1d(seen[0][::500], _subset(rng, ni, 40))   # a few of them are candidates
    lists[1] = seen[1].copy()                                    # everything is seen: count 0
    lists[3] = seen[0][5:1200]                                   # so is this, over three chunks
    lists[5] = np.union1d(lists[5], [int(pi[0])])                # the duplicated pair's item
    cand, cptr = _csr(lists)
    shared = np.union1d(seen[0][::300], _subset(rng, ni, 700))
    with _context(k, 64, nu, ni, U, I, None, (pu, pi), SIGNALS) as c:
        got = c.recommend_candidates(req, topn, cand, cptr, SIGNALS)
        got_s = c.recommend_candidates(req, topn, shared, None, SIGNALS)
    S = po.test_scores(U, I, req)
    _assert_equal(got, topn_reference(S, topn, candidate_seen(ni, lists, seen)))
    assert got[2][1] == 0 and got[2][3] == 0
    _assert_equal(got_s, topn_reference(S, topn, candidate_seen(ni, [shared] * len(req), seen)))


def test_on_sharded_contexts():
    """Three ranks without a communicator: own users work under SIGNALS, a foreign user fails,
    ALL works anywhere."""
    rng = np.random.default_rng(3)
    nu, ni, k, topn = 90, 400, 16, 12
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    pu, pi = _pairs(rng, nu, ni, 3000)
    everyone = np.arange(nu, dtype=np.int64)
    lists = [_subset(rng, ni, n) for n in rng.integers(0, 300, nu)]
    shared = _subset(rng, ni, 150)
    deny = _subset(rng, ni, 100)
    S = po.test_scores(U, I, everyone)
    seen = _seen(pu, pi, everyone)
    want_p = topn_reference(S, topn, candidate_seen(ni, lists, seen))
    want_s = topn_reference(S, topn, candidate_seen(ni, [shared] * nu, seen))
    want_d = topn_reference(S, topn, deny_seen(deny, nu, seen))
    want_all = topn_reference(S, topn, candidate_seen(ni, lists))
    with _context(k, 64, nu, ni, U, I, None, (pu, pi), SIGNALS) as c:
        rowptr = c.download_csr(0)[0]
    for rank in range(3):
        lo, hi = qmf_amd.partition_rows(rowptr, 3, rank)
        own = everyone[lo:hi]
        cand, cptr = _csr(lists[lo:hi])
        with _context(k, 64, nu, ni, U, I, None, (pu, pi), SIGNALS) as c:
            c.dist_init(rank, 3, None)
            _assert_equal(c.recommend_candidates(own, topn, cand, cptr, SIGNALS),
                          [w[lo:hi] for w in want_p])
            _assert_equal(c.recommend_candidates(own, topn, shared, None, SIGNALS),
                          [w[lo:hi] for w in want_s])
            _assert_equal(c.recommend_without(own, deny, topn, SIGNALS),
                          [w[lo:hi] for w in want_d])
            outside = np.array([(hi % nu) if rank < 2 else 0], np.int64)
            with pytest.raises(qmf_amd.QmfxError):
                c.recommend_candidates(outside, topn, shared, None, SIGNALS)
            with pytest.raises(qmf_amd.QmfxError):
                c.recommend_without(outside, deny, topn, SIGNALS)
            call, cptr_all = _csr(lists)
            _assert_equal(c.recommend_candidates(everyone, topn, call, cptr_all, ALL), want_all)


def test_user_batches_equal_one_launch(monkeypatch):
    """150 users in batches of one group of 32 (QMFX_EVAL_BATCH_GROUPS=1): the same lists."""
    rng = np.random.default_rng(9)
    nu, ni, k, topn = 400, 900, 16, 20
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    pu, pi = _pairs(rng, nu, ni, 6000)
    req = rng.choice(nu, 150, replace=False).astype(np.int64)
    lists = [_subset(rng, ni, n) for n in rng.integers(0, 800, len(req))]
    cand, cptr = _csr(lists)
    shared = _subset(rng, ni, 600)
    deny = _subset(rng, ni, 300)
    out = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("QMFX_EVAL_BATCH_GROUPS", env)
        with _context(k, 64, nu, ni, U, I, None, (pu, pi), SIGNALS) as c:
            out.append((c.recommend_candidates(req, topn, cand, cptr, SIGNALS),
                        c.recommend_candidates(req, topn, shared, None, SIGNALS),
                        c.recommend_without(req, deny, topn, SIGNALS)))
    S = po.test_scores(U, I, req)
    seen = _seen(pu, pi, req)
    want = (topn_reference(S, topn, candidate_seen(ni, lists, seen)),
            topn_reference(S, topn, candidate_seen(ni, [shared] * len(req), seen)),
            topn_reference(S, topn, deny_seen(deny, len(req), seen)))
    for j in range(3):
        _assert_equal(out[1][j], out[0][j])
        _assert_equal(out[0][j], want[j])


def test_errors_leave_the_context_usable():
    rng = np.random.default_rng(1)
    nu, ni, k, topn = 20, 100, 8, 5
    U, I = rng.normal(0, 0.3, (nu, k)), rng.normal(0, 0.3, (ni, k))
    req = np.arange(5, dtype=np.int64)
    lst = np.array([3, 9, 40, 99], np.int64)
    cand = np.concatenate([lst] * 5)
    cptr = np.arange(6, dtype=np.int64) * 4
    S = po.test_scores(U, I, req)
    want = topn_reference(S, topn, candidate_seen(ni, [lst] * 5))

    def raw_candidates(c, cptr, ncand, cand):
        P = ctypes.POINTER(ctypes.c_int64)
        out = c._topn_out(len(req), topn)
        return qmf_amd.lib().qmfx_recommend_candidates(
            c.h, len(req), req.ctypes.data_as(P), None if cptr is None else cptr.ctypes.data_as(P),
            ncand, cand.ctypes.data_as(P), topn, ALL, 0, out[0].ctypes.data_as(P),
            out[1].ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            out[2].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))

    def raw_without(c, ndeny, deny):
        P = ctypes.POINTER(ctypes.c_int64)
        out = c._topn_out(len(req), topn)
        return qmf_amd.lib().qmfx_recommend_without(
            c.h, len(req), req.ctypes.data_as(P), ndeny, deny.ctypes.data_as(P), topn, ALL, 0,
            out[0].ctypes.data_as(P), out[1].ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            out[2].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))

    with _context(k, 64, nu, ni, U, I) as c:
        def still_fine():
            _assert_equal(c.recommend_candidates(req, topn, cand, cptr), want)
            _assert_equal(c.recommend_candidates(req, topn, lst), want)

        bad_cptr0 = cptr.copy()
        bad_cptr0[0] = 1
        bad_decr = cptr.copy()
        bad_decr[2], bad_decr[3] = cptr[3], cptr[2]
        calls = [
            # everything qmfx_recommend rejects
            lambda: c.recommend_candidates(req, 0, lst),
            lambda: c.recommend_candidates(req, 129, lst),
            lambda: c.recommend_candidates(np.array([nu]), topn, lst),
            lambda: c.recommend_candidates(req, topn, lst, None, SIGNALS),
            lambda: c.recommend_candidates(req, topn, lst, None, POSITIVES),
            lambda: c.recommend_candidates(req, topn, lst, None, ALL, True),
            lambda: c.recommend_candidates(req, topn, lst, None, 3),
            lambda: c.recommend_without(req, lst, 0),
            lambda: c.recommend_without(np.array([-1]), lst, topn),
            lambda: c.recommend_without(req, lst, topn, SIGNALS),
            lambda: c.recommend_without(req, lst, topn, ALL, True),
            # an index out of range
            lambda: c.recommend_without(req, np.array([3, ni]), topn),
            lambda: c.recommend_without(req, np.array([-1, 3]), topn),
            lambda: c.recommend_candidates(req, topn, np.array([3, ni])),
            lambda: c.recommend_candidates(req, topn, np.array([-1, 3])),
            lambda: c.recommend_candidates(req, topn, np.concatenate([cand[:-1], [ni]]), cptr),
            # cptr
            lambda: c.recommend_candidates(req, topn, cand, bad_cptr0),
            lambda: c.recommend_candidates(req, topn, cand, bad_decr),
            # not strictly ascending: a repeat, a descent, and a descent inside one user's list
            lambda: c.recommend_candidates(req, topn, np.array([3, 9, 9, 40])),
            lambda: c.recommend_candidates(req, topn, np.array([3, 40, 9])),
            lambda: c.recommend_candidates(req, topn, np.concatenate([cand[:5], [9, 3], cand[7:]]),
                                           cptr),
        ]
        for n, call in enumerate(calls):
            with pytest.raises(qmf_amd.QmfxError) as e:
                call()
            assert "qmfx error -1" in str(e.value), n
            assert str(e.value).split(": ", 1)[1].strip(), n
            still_fine()
        # a descent across two users' lists is fine: each list is ascending on its own
        _assert_equal(c.recommend_candidates(req, topn, cand, cptr), want)
        # negative counts and 2^31 candidates (rejected before a list is read)
        assert raw_candidates(c, None, -1, lst) == -1
        assert raw_without(c, -1, lst) == -1
        assert raw_candidates(c, None, 2**31, lst) == -1
        huge = cptr.copy()
        huge[-1] = 2**31
        assert raw_candidates(c, huge, 0, cand) == -1
        assert qmf_amd.lib().qmfx_last_error().decode().strip()
        still_fine()
        # empty requests succeed; so do empty lists
        for got in (c.recommend_candidates(np.array([], np.int64), topn, lst),
                    c.recommend_candidates(np.array([], np.int64), topn, cand[:0],
                                           np.zeros(1, np.int64)),
                    c.recommend_without(np.array([], np.int64), lst, topn)):
            assert got[0].shape == (0, topn) and got[1].shape == (0, topn) and got[2].shape == (0,)
        got = c.recommend_candidates(req, topn, cand[:0], np.zeros(6, np.int64))
        assert got[2].tolist() == [0] * 5 and np.all(got[0] == -1) and np.all(got[1] == 0.0)
        _assert_equal(c.recommend_without(req, cand[:0], topn), topn_reference(S, topn))


def test_reported_work_is_the_lists():
    rng = np.random.default_rng(2)
    nu, ni, k, topn = 40, 2000, 24, 10
    U, I, _ = _factors(rng, nu, ni, k, 64, False)
    req = _request(rng, nu, 19)
    lists = [_subset(rng, ni, n) for n in rng.integers(0, 1200, len(req))]
    cand, cptr = _csr(lists)
    shared = _subset(rng, ni, 777)
    deny = _subset(rng, ni, 100)
    with _context(k, 64, nu, ni, U, I) as c:
        c.reset_stats()
        c.recommend_candidates(req, topn, cand, cptr)
        st = c.solve_stats()
        assert st["flops"] == 2.0 * k * len(cand) and st["launches"] == 1 and st["ms"] > 0
        c.reset_stats()
        c.recommend_candidates(req, topn, shared)
        assert c.solve_stats()["flops"] == 2.0 * k * len(req) * len(shared)
        c.reset_stats()
        c.recommend_without(req, deny, topn)
        assert c.solve_stats()["flops"] == 2.0 * k * len(req) * ni
