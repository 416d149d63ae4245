"""qmfx_recommend_screened on the device against qmfx_recommend on the same context.

Bar: equality.  Items, scores (compared as int64 views) and counts of the screened call are the
dense call's, whatever `sample` and `cap`; several cases also compare with numpy
(test_recommend.topn_reference), so the oracle is not only the library.

The rule that keeps the exact scan from hiding a broken screen: a case marked *screened* first
proves in numpy (test_screened.screen_bound_counts) that no conforming filter can emit more
than `cap` items for any user and that every sample holds topn eligible items, then asserts
that the call answered nobody by the exact scan (stats[1] == 0, stats[0] == nusers)."""
import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from test_recommend import topn_reference
from test_recommend_gpu import _assert_equal, _pairs, _seen
from test_screened import (TILE_ITEMS, TILE_USERS, sample_eligible, sample_items,
                           screen_bound_counts)

pytestmark = pytest.mark.gpu

ALL, SIGNALS, POSITIVES = 0, 1, 2


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _uniform(rng, nu, ni, k, prec, bias=False):
    U, I = rng.uniform(-0.5, 0.5, (nu, k)), rng.uniform(-0.5, 0.5, (ni, k))
    b = rng.uniform(-0.2, 0.2, ni) if bias else None
    if prec == 32:  # the device stores fp32: the references score those same values
        U, I, b = _f32(U), _f32(I), (_f32(b) if bias else None)
    return U, I, b


def _context(k, prec, U, I, b=None, signals=None, positives=None):
    c = qmf_amd.Context(k, prec)
    if signals is not None:
        uids, iids = c.group_signals(signals[0], signals[1], np.ones(len(signals[0])))
        assert np.array_equal(uids, np.arange(len(U))) and np.array_equal(iids, np.arange(len(I)))
    else:
        c.set_shape(len(U), len(I))
    if positives is not None:
        c.bpr_set_positives(*positives)
    c.set_factors(0, U)
    c.set_factors(1, I)
    if b is not None:
        c.bpr_set_biases(b)
    return c


def _same_bits(got, want):
    _assert_equal(got, want)
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), "score bits"


def _prove_screened(U, I, b, req, seen, topn, S, cap):
    bound = screen_bound_counts(U[req], I, b, seen, topn, S)
    assert bound.max() <= cap, (bound.max(), cap)
    assert sample_eligible(seen, len(I), S, len(req)).min() >= topn
    return bound


def _assert_screened(c, n):
    st = c.screen_stats()
    assert st[1] == 0 and st[0] == n, st
    assert 0 < st[3] <= st[2]
    return st


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("excl", [ALL, SIGNALS, POSITIVES])
@pytest.mark.parametrize("prec", [32, 64])
def test_screened_equals_dense_and_numpy(prec, excl, bias):
    """*Screened.*  70 requests (repeats, any order) × 3001 items, k = 20, 40 seen items per
    user under the two unseen modes: S = 256, cap = 512 (bound max ≈ 211)."""
    rng = np.random.default_rng(100 * prec + 10 * excl + bias)
    nu, ni, k, topn, S, cap = 90, 3001, 20, 10, 256, 512
    U, I, b = _uniform(rng, nu, ni, k, prec, bias)
    req = np.concatenate([rng.permutation(nu)[:68], [5, 5]]).astype(np.int64)
    pu, pi = _pairs(rng, nu, ni, 40 * nu - nu - ni)
    seen = _seen(pu, pi, req) if excl != ALL else None
    bound = _prove_screened(U, I, b, req, seen, topn, S, cap)
    with _context(k, prec, U, I, b, signals=(pu, pi) if excl == SIGNALS else None,
                  positives=(pu, pi) if excl == POSITIVES else None) as c:
        want = c.recommend(req, topn, excl, bias)
        got = c.recommend_screened(req, topn, excl, bias, S, cap)
        st = _assert_screened(c, len(req))
        assert st[3] <= bound.max() and st[2] <= bound.sum()
        _same_bits(got, want)
        # sample and cap never change the answer
        _same_bits(c.recommend_screened(req, topn, excl, bias, 2 * S, cap), want)
        _same_bits(c.recommend_screened(req, topn, excl, bias, S, ni), want)
        _same_bits(c.recommend_screened(req, topn, excl, bias), want)   # auto: small catalogue
        assert c.screen_stats()[0] == 0
    _assert_equal(got, topn_reference(po.test_scores(U, I, req, b), topn, seen))


def test_screened_long_lists():
    """*Screened.*  topn = 128 (lists of several re-rank chunks: bound max ≈ 917, cap 1536) and
    k = 130 at 33 × 1025 (topn = 7, S = 128, cap = 256)."""
    for seed, (nr, ni, k, topn, S, cap, prec) in enumerate([(70, 3001, 20, 128, 512, 1536, 64),
                                                            (33, 1025, 130, 7, 128, 256, 32)]):
        rng = np.random.default_rng(seed)
        U, I, _ = _uniform(rng, nr, ni, k, prec)
        req = rng.permutation(nr).astype(np.int64)
        _prove_screened(U, I, None, req, None, topn, S, cap)
        with _context(k, prec, U, I) as c:
            want = c.recommend(req, topn)
            _same_bits(c.recommend_screened(req, topn, sample=S, cap=cap), want)
            _assert_screened(c, nr)
        _assert_equal(want, topn_reference(po.test_scores(U, I, req), topn))


@pytest.mark.parametrize("k", [1, 3, 16, 17, 64, 65, 128, 130, 256])
def test_screened_tile_edges(k):
    """*Screened* wherever a sample of topn items exists.  User counts 1, tile − 1, tile,
    tile + 1 (repeated and unordered) × item counts tile − 1, tile, tile + 1, 2·tile + 1 × topn
    1, 10, 128, at every k stage boundary; cap = the catalogue, so no list can overflow.  Where
    topn exceeds the catalogue every sample is short and everyone takes the exact scan."""
    prec = 32 if k % 2 else 64
    rng = np.random.default_rng(k)
    nu = TILE_USERS + 1
    for ni in (TILE_ITEMS - 1, TILE_ITEMS, TILE_ITEMS + 1, 2 * TILE_ITEMS + 1):
        U, I, b = _uniform(rng, nu, ni, k, prec, bias=True)
        with _context(k, prec, U, I, b) as c:
            for n in (1, TILE_USERS - 1, TILE_USERS, TILE_USERS + 1):
                req = rng.integers(0, nu, n).astype(np.int64)
                for topn in (1, 10, 128):
                    want = c.recommend(req, topn, ALL, True)
                    if topn <= ni:
                        got = c.recommend_screened(req, topn, ALL, True, max(topn, 64), ni)
                        _assert_screened(c, n)
                    else:
                        got = c.recommend_screened(req, topn, ALL, True, 0, topn)
                        assert c.screen_stats().tolist()[:2] == [0, n]
                    _same_bits(got, want)
        if ni == 2 * TILE_ITEMS + 1:
            _assert_equal(want, topn_reference(po.test_scores(U, I, req, b), 128))


def test_forced_exact_scan():
    """cap = topn (nearly everyone overflows), a cap between the list lengths (some do), an
    all-zero user row (every item ties at L = 0 and passes), a user who has seen all but
    topn − 1 items of the sample (short sample) and one with 3 eligible items in the catalogue
    (short count, −1 / 0.0 tail)."""
    rng = np.random.default_rng(5)
    nu, ni, k, topn, S = 70, 3001, 20, 10, 256
    U, I, _ = _uniform(rng, nu, ni, k, 64)
    U[5] = 0.0
    smp = sample_items(ni, S)
    pu, pi = _pairs(rng, nu, ni, 2000)
    pu = np.concatenate([pu, np.full(S - topn + 1, 7), np.full(ni - 3, 9)])
    pi = np.concatenate([pi, smp[:S - topn + 1], np.arange(3, ni)])
    drop = (pu == 9) & (pi < 3) | (pu == 7) & np.isin(pi, smp[S - topn + 1:])
    pu, pi = pu[~drop], pi[~drop]
    # the items taken from users 7 and 9 stay in the data through other users
    pu = np.concatenate([pu, [0, 1, 2], np.zeros(topn - 1, np.int64)])
    pi = np.concatenate([pi, [0, 1, 2], smp[S - topn + 1:]])
    req = np.arange(nu, dtype=np.int64)
    seen = _seen(pu, pi, req)
    assert sample_eligible(seen, ni, S, nu)[7] == topn - 1 and ni - len(seen[9]) == 3
    with _context(k, 64, U, I, signals=(pu, pi)) as c:
        want = c.recommend(req, topn, SIGNALS)
        _same_bits(c.recommend_screened(req, topn, SIGNALS, False, S, 512), want)
        st = c.screen_stats()
        assert st[1] == 3 and st[0] == nu - 3, st          # users 5, 7 and 9
        _same_bits(c.recommend_screened(req, topn, SIGNALS, False, S, topn), want)
        assert c.screen_stats()[1] >= nu - 5
        mid = int(np.median(screen_bound_counts(U, I, None, seen, topn, S)))
        _same_bits(c.recommend_screened(req, topn, SIGNALS, False, S, mid), want)
        st = c.screen_stats()
        assert 3 < st[1] < nu and st[3] <= mid, st
        # the zero row alone, with nothing seen: ties broken by the item index
        z = c.recommend_screened(np.array([5]), topn, ALL, False, S, 512)
        assert c.screen_stats().tolist()[:2] == [0, 1]
        assert z[0].tolist() == [list(range(topn))]
    assert want[2][9] == 3 and want[0][9, 3:].tolist() == [-1] * 7
    _assert_equal(want, topn_reference(po.test_scores(U, I, req), topn, seen))


def _attack(U, I, b=None, prec=64, topn=10, S=256, cap=512, users=None):
    k = U.shape[1]
    req = np.arange(len(U), dtype=np.int64) if users is None else users
    with _context(k, prec, U, I, b) as c:
        want = c.recommend(req, topn, ALL, b is not None)
        _same_bits(c.recommend_screened(req, topn, ALL, b is not None, S, cap), want)
        st = c.screen_stats()
        _same_bits(c.recommend_screened(req, topn, ALL, b is not None, topn, len(I)), want)
    return want, st


def test_bound_attack_quantised_factors_and_signed_zeros():
    """Factors in multiples of 1/4: mass ties at the threshold, which the item index breaks;
    and rows of signed zeros (scores ±0.0 compare equal)."""
    rng = np.random.default_rng(11)
    U = np.round(rng.uniform(-0.5, 0.5, (40, 20)) * 4) / 4
    I = np.round(rng.uniform(-0.5, 0.5, (3001, 20)) * 4) / 4
    for prec in (32, 64):
        want, _ = _attack(U, I, prec=prec)
        _assert_equal(want, topn_reference(po.test_scores(U, I, np.arange(40)), 10))
    Z = np.where(rng.random((3001, 20)) < 0.5, -0.0, 0.0)
    Z[::7] = I[::7]
    Uz = U.copy()
    Uz[::3] = -0.0
    _attack(Uz, Z)


def test_bound_attack_rows_the_screen_cannot_tell_apart():
    """600 item rows equal up to perturbations of 1e-12, the best for every user: equal in
    f32, ordered only by the exact re-rank."""
    rng = np.random.default_rng(12)
    U = rng.uniform(0.1, 0.5, (30, 20))
    I = rng.uniform(-0.5, 0.5, (3001, 20))
    I[1000:1600] = 0.9 + 1e-12 * rng.standard_normal((600, 20))
    want, st = _attack(U, I, cap=1024)
    assert st[1] == 0 and st[3] >= 600, st
    assert np.all((want[0] >= 1000) & (want[0] < 1600))
    _assert_equal(want, topn_reference(po.test_scores(U, I, np.arange(30)), 10))


@pytest.mark.parametrize("scale", [1e-30, 1e25])
def test_bound_attack_f32_range(scale):
    """fp64 factors whose products underflow f32 (every a is 0 or subnormal: the absolute term
    of the slack must let everything through) or overflow it (a is not finite: passes)."""
    rng = np.random.default_rng(13)
    U, I, _ = _uniform(rng, 30, 3001, 20, 64)
    want, _ = _attack(U * scale, I * scale)
    _assert_equal(want, topn_reference(po.test_scores(U * scale, I * scale, np.arange(30)), 10))
    # one side only: the other keeps ordinary magnitudes
    _attack(U * scale, I)


def test_bound_attack_best_items_and_large_biases():
    """The best items outside the sample, at index 0 and at the last index; biases much larger
    than the dot products."""
    rng = np.random.default_rng(14)
    ni = 3001
    U = rng.uniform(0.05, 0.5, (30, 20))
    I = rng.uniform(-0.5, 0.5, (ni, 20))
    smp = sample_items(ni, 256)
    assert 0 in smp and 1 not in smp and ni - 1 not in smp
    for best in ([1, 2, 3], [0], [ni - 1], [0, 1, ni - 1]):
        J = I.copy()
        J[best] = 5.0
        want, st = _attack(U, J)
        assert st[1] == 0, st
        assert sorted(want[0][0, :len(best)].tolist()) == best
    b = rng.uniform(-1e6, 1e6, ni)
    for prec in (32, 64):
        bb = _f32(b) if prec == 32 else b
        UU, II = (_f32(U), _f32(I)) if prec == 32 else (U, I)
        want, _ = _attack(UU, II, bb, prec=prec)
        _assert_equal(want, topn_reference(po.test_scores(UU, II, np.arange(30), bb), 10))


def test_errors_leave_the_context_usable_and_state_untouched():
    rng = np.random.default_rng(15)
    nu, ni, k, topn, S, cap = 60, 2000, 24, 8, 128, 400
    U, I, _ = _uniform(rng, nu, ni, k, 64)
    pu, pi = _pairs(rng, nu, ni, 3000)
    req = rng.permutation(nu)[:40].astype(np.int64)
    with _context(k, 64, U, I, signals=(pu, pi)) as c:
        want = c.recommend(req, topn, SIGNALS)
        csr = c.download_csr(0)
        bad = [dict(topn=0), dict(topn=129), dict(users=np.array([nu])), dict(users=np.array([-1])),
               dict(exclude=POSITIVES), dict(exclude=3), dict(use_biases=True),
               dict(sample=topn - 1), dict(sample=ni + 1), dict(sample=-1), dict(cap=topn - 1),
               dict(cap=-1)]
        for kw in bad:
            args = dict(users=req, topn=topn, exclude=SIGNALS, use_biases=False, sample=S, cap=cap)
            args.update(kw)
            with pytest.raises(qmf_amd.QmfxError) as e:
                c.recommend_screened(**args)
            assert str(e.value).split(": ", 1)[1].strip(), kw
            _same_bits(c.recommend_screened(req, topn, SIGNALS, False, S, cap), want)
        empty = c.recommend_screened(np.array([], np.int64), topn, SIGNALS, False, S, cap)
        assert empty[0].shape == (0, topn) and empty[2].shape == (0,)
        # a large request, then a small one on the same scratch
        everyone = np.arange(nu, dtype=np.int64)
        _same_bits(c.recommend_screened(everyone, 100, SIGNALS, False, 512, ni),
                   c.recommend(everyone, 100, SIGNALS))
        _same_bits(c.recommend_screened(req[:3], 2, SIGNALS, False, 64, 100),
                   c.recommend(req[:3], 2, SIGNALS))
        # nothing the context holds has moved
        assert np.array_equal(c.factors(0), U) and np.array_equal(c.factors(1), I)
        for a, w in zip(c.download_csr(0), csr):
            assert np.array_equal(a, w)
        _same_bits(c.recommend(req, topn, SIGNALS), want)
        # accounted like the dense call: 2k flop per (user, item scanned)
        c.reset_stats()
        c.recommend_screened(req, topn, SIGNALS, False, S, cap)
        st = c.solve_stats()
        assert st["launches"] == 1 and st["flops"] == 2.0 * k * len(req) * ni and st["ms"] > 0


def test_screened_on_sharded_contexts():
    """The own-rows rule of QMFX_REC_UNSEEN_SIGNALS: a rank answers its own users, rejects
    another rank's, and the ranks together give the unsharded lists."""
    rng = np.random.default_rng(16)
    nu, ni, k, topn, S, cap = 150, 1500, 16, 6, 128, 1500
    U, I, _ = _uniform(rng, nu, ni, k, 64)
    pu, pi = _pairs(rng, nu, ni, 4000)
    everyone = np.arange(nu, dtype=np.int64)
    with _context(k, 64, U, I, signals=(pu, pi)) as c:
        rowptr = c.download_csr(0)[0]
        whole = c.recommend(everyone, topn, SIGNALS)
    parts = []
    for rank in range(3):
        lo, hi = qmf_amd.partition_rows(rowptr, 3, rank)
        with _context(k, 64, U, I, signals=(pu, pi)) as c:
            c.dist_init(rank, 3, None)
            parts.append(c.recommend_screened(everyone[lo:hi], topn, SIGNALS, False, S, cap))
            assert c.screen_stats()[0] > 0
            outside = (hi % nu) if rank < 2 else 0
            with pytest.raises(qmf_amd.QmfxError):
                c.recommend_screened(np.array([outside]), topn, SIGNALS, False, S, cap)
            _same_bits(c.recommend_screened(everyone[::7], topn, ALL, False, S, cap),
                       c.recommend(everyone[::7], topn, ALL))
    _same_bits([np.concatenate([p[j] for p in parts]) for j in range(3)], whole)
