"""The three BPR kernels (qmf_amd/csrc/bpr.hip) beyond k = 64 and one wave.

1. bpr_apply_kernel / bpr_epoch_kernel on one wave at E = ceil(kp/64) = 2, 3, 4 against the
   oracle's BPREngine::update (BPREngine.cpp:178-220) over the restated (u, p, n) sequence;
   users at the 64-positive staging boundary, a user who holds every item (the 4096-attempt
   cap then returns a positive, possibly p itself), epochs shorter than the prefetch depth.
2. bpr_eval_kernel at every NT = kp/16 against the oracle's loss sum (BPREngine.cpp:246-274).
3. The multi-wave epoch linearised (lr = 2⁻³⁰, one side zero): the other side's rows are then
   ½·lr·Σ over exactly the epoch's triplets, whatever the interleaving of the waves, so a
   skipped or repeated positive or a lost update shows at first order.
   tests/test_oracle.py::test_bpr_linearised_epoch_anchor pins the tolerance on the CPU.
4. The multi-wave epoch at a real learning rate: with item_lambda = bias_lambda = 0 every
   step adds ±lr·e·p_u to two item rows and ±lr·e to two biases, so the item factors' column
   sums and Σ bias are invariant unless an update is lost.
5. A NaN in a user row: the step is skipped, the call reports "gradients too big".
"""
import functools

import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from helpers import (bpr_linear_item, bpr_linear_user, bpr_wave_case, bpr_wave_triplets,
                     triplets)

pytestmark = pytest.mark.gpu
LR = 0.05
LAM = (1.0, 0.025, 0.0025)  # bias, user, item
TOL = {64: 1e-12, 32: 1e-5}
UNIT = {64: 2.0 ** -53, 32: 2.0 ** -24}


def rounded(a, precision):
    """The values the device holds after set_factors / bpr_set_biases."""
    return a.astype(np.float32).astype(np.float64) if precision == 32 else a


def check_state(got, want, tol, what):
    """Factors relative to max|U|, |I|; biases relative to max(|b|, 1): the bounds of
    test_bpr_epoch_single_wave_exact."""
    (gU, gI, gb), (U, I, b) = got, want
    scale = max(np.abs(U).max(), np.abs(I).max())
    eu, ei = np.max(np.abs(gU - U)) / scale, np.max(np.abs(gI - I)) / scale
    eb = np.max(np.abs(gb - b)) / max(np.abs(b).max(), 1)
    print(what, "err U %.3g I %.3g bias %.3g (tol %.3g)" % (eu, ei, eb, tol))
    assert eu <= tol, what
    assert ei <= tol, what
    assert eb <= tol, what


def state(c):
    return c.factors(0), c.factors(1), c.bpr_biases()


def init_state(nu, ni, k, precision, seed):
    rng = np.random.default_rng(seed)
    return tuple(rounded(rng.normal(0, 0.1, s), precision) for s in ((nu, k), (ni, k), ni))


def load(c, U0, I0, b0):
    c.set_factors(0, U0)
    c.set_factors(1, I0)
    c.bpr_set_biases(b0)


# ---- 1. exact serial semantics at every E

@functools.lru_cache(maxsize=None)
def apply_triplets():
    rng = np.random.default_rng(1)
    nu, ni, n = 60, 80, 3000
    trip = np.stack([rng.integers(0, nu, n), rng.integers(0, ni, n), rng.integers(0, ni, n)], 1)
    same = rng.random(n) < 0.05
    trip[same, 2] = trip[same, 1]
    trip.setflags(write=False)
    return nu, ni, trip


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [80, 100, 128, 130, 200, 256])
def test_bpr_apply_exact_wide_rows(k, precision):
    """bpr_apply_kernel at E = 2 (k = 80, 100, 128), 3 (130) and 4 (200, 256), biases on, 5% of
    the triplets with p == n (q_n's step then starts from the new q_p).  Bounds as at k = 64
    (test_c4_bpr_update_sequence_k64): 1e-12 / 1e-5 of max|·|."""
    nu, ni, trip = apply_triplets()
    assert 100 < np.sum(trip[:, 1] == trip[:, 2]) < 250
    U, I, b = init_state(nu, ni, k, precision, k)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        load(c, U, I, b)
        c.bpr_apply(trip, LR, *LAM, True)
        got = state(c)
    po.bpr_update_seq(U, I, b, trip, LR, *LAM, True)
    check_state(got, (U, I, b), TOL[precision], "apply k=%d" % k)


@functools.lru_cache(maxsize=None)
def positives(case):
    """"boundary": 20 users × 300 items; users 0..5 hold exactly 1, 63, 64, 65, 128 and 129
    items (≤ 64 are staged in registers, longer lists are scanned from memory), the others a
    few.  "all_items": 20 users × 40 items; user 0 holds every item, so each of their draws
    ends at the attempt cap with a positive.  Data order is shuffled."""
    rng = np.random.default_rng(11)
    if case == "boundary":
        nu, ni, counts, extra = 20, 300, (1, 63, 64, 65, 128, 129), 150
    else:
        nu, ni, counts, extra = 20, 40, (40,), 60
    users = [np.full(cnt, u) for u, cnt in enumerate(counts)]
    items = [rng.permutation(ni)[:cnt] for cnt in counts]
    users.append(rng.integers(len(counts), nu, extra))
    items.append(rng.integers(0, ni, extra))
    keys = rng.permutation(np.unique(np.concatenate(users) * ni + np.concatenate(items)))
    users, items = (keys // ni).astype(np.int64), (keys % ni).astype(np.int64)
    assert tuple(np.bincount(users)[:len(counts)]) == counts
    return nu, ni, users, items


@functools.lru_cache(maxsize=None)
def epoch_triplets(case, seed, num_neg, shuffle):
    _, ni, users, items = positives(case)
    trip = triplets(users, items, ni, seed, num_neg, shuffle)
    trip.setflags(write=False)
    return trip


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("num_neg", [1, 4, 5, 9])
@pytest.mark.parametrize("k", [100, 130, 256])
@pytest.mark.parametrize("case", ["boundary", "all_items"])
def test_bpr_epoch_single_wave_exact_wide_rows(case, k, num_neg, precision, monkeypatch):
    """bpr_epoch_kernel on one wave at E = 2, 3, 4; num_neg = one partial group of four, one
    group, a group + 1, two groups + 1; identity order, then shuffled."""
    monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    nu, ni, users, items = positives(case)
    U, I, b = init_state(nu, ni, k, precision, k + num_neg)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        load(c, U, I, b)
        c.bpr_set_positives(users, items)
        for seed, shuffle in ((7, False), (8, True)):
            c.bpr_epoch(seed, num_neg, LR, *LAM, True, shuffle=shuffle)
            assert c.bpr_plan()[0] == 1
            trip = epoch_triplets(case, seed, num_neg, shuffle)
            if case == "all_items":  # the cap returned a positive
                assert np.all(np.isin(trip[trip[:, 0] == 0, 2], items[users == 0]))
            po.bpr_update_seq(U, I, b, trip, LR, *LAM, True)
            check_state(state(c), (U, I, b), TOL[precision],
                        "%s k=%d neg=%d shuffle=%d" % (case, k, num_neg, shuffle))


def test_bpr_all_items_case_draws_the_positive_itself():
    """The all-items case reaches p == n (the capped draw returns p): the epoch must then
    continue q_n from the new q_p, as BPREngine::update does in place."""
    hit = {nn: sum(int(np.sum(t[:, 1] == t[:, 2]))
                   for t in (epoch_triplets("all_items", 7, nn, False),
                             epoch_triplets("all_items", 8, nn, True)))
           for nn in (4, 5, 9)}
    print("p == n triplets per num_neg:", hit)
    assert all(v > 0 for v in hit.values()), hit


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [16, 130])
@pytest.mark.parametrize("npos", [1, 2, 3, 5])
def test_bpr_epoch_shorter_than_prefetch(npos, k, precision, monkeypatch):
    """Fewer positives than the 3-stage prefetch looks ahead: the slots past the end wrap to
    valid, unused positives."""
    monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    nu, ni, num_neg = 20, 30, 3
    rng = np.random.default_rng(npos)
    keys = rng.permutation(nu * ni)[:npos]
    users, items = (keys // ni).astype(np.int64), (keys % ni).astype(np.int64)
    U, I, b = init_state(nu, ni, k, precision, 100 + npos)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        load(c, U, I, b)
        c.bpr_set_positives(users, items)
        for seed in (5, 6):
            c.bpr_epoch(seed, num_neg, LR, *LAM, True, shuffle=True)
            assert c.bpr_plan()[0] == 1
            trip = triplets(users, items, ni, seed, num_neg, True)
            assert len(trip) == npos * num_neg
            po.bpr_update_seq(U, I, b, trip, LR, *LAM, True)
            check_state(state(c), (U, I, b), TOL[precision], "npos=%d k=%d" % (npos, k))


# ---- 2. the loss kernel

EVAL_NU, EVAL_NI = 200, 300
EVAL_N = (1, 15, 17, 16384 + 5, 40000)  # one pass of the grid covers 16384 triplets


@functools.lru_cache(maxsize=None)
def eval_triplets(seed=2):
    rng = np.random.default_rng(seed)
    n = EVAL_N[-1]
    trip = np.stack([rng.integers(0, EVAL_NU, n), rng.integers(0, EVAL_NI, n),
                     rng.integers(0, EVAL_NI, n)], 1)
    trip.setflags(write=False)
    return trip


def eval_cases():
    out = []
    for nt in range(1, 17):
        for ub in ((True, False) if nt in (1, 4, 8, 16) else (nt % 2 == 1,)):
            out.append((16 * nt, ub))
    return out + [(30, True), (100, False), (130, True)]


def score_magnitude(U, I, b, trip, use_biases):
    """Σ_f |p_u,f (q_p,f − q_n,f)| + |b_p| + |b_n| per triplet."""
    mag = np.abs(U[trip[:, 0]] * (I[trip[:, 1]] - I[trip[:, 2]])).sum(1)
    if use_biases:
        mag += np.abs(b[trip[:, 1]]) + np.abs(b[trip[:, 2]])
    return mag


def loss_tol(precision, want, k, mag):
    """fp64: only the summation order differs, 1e-12 of the sum.  fp32: the loss is
    1-Lipschitz in x̂, and x̂'s rounding error is at most (k+2)·2⁻²⁴ times the triplet's
    score magnitude, so the sums differ by at most n times the largest such error."""
    return 1e-12 * abs(want) if precision == 64 else len(mag) * (k + 2) * 2.0 ** -24 * mag.max()


def check_loss(c, slot, U, I, b, trip, use_biases, precision, what):
    k = U.shape[1]
    mag = score_magnitude(U, I, b, trip, use_biases)
    for n in sorted({min(n, len(trip)) for n in EVAL_N}):
        got = c.bpr_eval(slot, trip[:n], use_biases)
        want = po.bpr_loss_sum(U, I, b, trip[:n], use_biases)
        tol = loss_tol(precision, want, k, mag[:n])
        print(what, "n=%d loss %.12g err %.3g tol %.3g" % (n, want, abs(got - want), tol))
        assert abs(got - want) <= tol, (what, n)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k,use_biases", eval_cases())
def test_bpr_eval_matches_oracle(k, use_biases, precision):
    """Every NT = kp/16 = 1..16 and padded k = 30, 100, 130; n = 1, 15, 17 (ragged groups of
    16 lanes) and 16389, 40000 (second and third pass of the grid-stride loop)."""
    rng = np.random.default_rng(k)
    U, I, b = (rounded(rng.normal(0, 0.3, s), precision)
               for s in ((EVAL_NU, k), (EVAL_NI, k), EVAL_NI))
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(EVAL_NU, EVAL_NI)
        load(c, U, I, b)
        check_loss(c, k % 2, U, I, b, eval_triplets(), use_biases, precision, "k=%d" % k)


@pytest.mark.parametrize("precision", [64, 32])
def test_bpr_eval_large_scores(precision):
    """N(0, 1) factors at k = 128: |x̂| reaches tens, the terms are large or below 1e-10."""
    k = 128
    rng = np.random.default_rng(128)
    U, I, b = (rounded(rng.normal(0, 1.0, s), precision)
               for s in ((EVAL_NU, k), (EVAL_NI, k), EVAL_NI))
    trip = eval_triplets()
    x = np.einsum("tf,tf->t", U[trip[:, 0]], I[trip[:, 1]] - I[trip[:, 2]])
    assert np.abs(x).max() > 30 and np.log1p(np.exp(-x)).min() < 1e-10
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(EVAL_NU, EVAL_NI)
        load(c, U, I, b)
        check_loss(c, 0, U, I, b, trip, True, precision, "N(0,1) k=128")


@pytest.mark.parametrize("precision", [64, 32])
def test_bpr_eval_ignores_padding_after_fill_uniform(precision):
    """k = 30 is stored with kp = 32: after qmfx_fill_uniform on both sides the two padding
    columns must contribute nothing to the loss."""
    k = 30
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(EVAL_NU, EVAL_NI)
        c.fill_uniform(0, 0.5, 1)
        c.fill_uniform(1, 0.5, 2)
        U, I = c.factors(0), c.factors(1)
        assert U.shape == (EVAL_NU, k) and np.abs(U).max() > 0.4 and np.abs(I).max() > 0.4
        check_loss(c, 0, U, I, np.zeros(EVAL_NI), eval_triplets(), False, precision,
                   "fill_uniform k=30")


@pytest.mark.parametrize("precision", [64, 32])
def test_bpr_eval_slot_reuploads_a_different_array(precision):
    """The per-slot upload cache is keyed by host address and length: two arrays of the same
    length, evaluated in turn in one slot, each give their own loss."""
    k, n = 48, 1000
    rng = np.random.default_rng(48)
    U, I, b = (rounded(rng.normal(0, 0.3, s), precision)
               for s in ((EVAL_NU, k), (EVAL_NI, k), EVAL_NI))
    ta = np.ascontiguousarray(eval_triplets()[:n])
    tb = np.ascontiguousarray(eval_triplets(3)[:n])
    assert ta.ctypes.data != tb.ctypes.data and not np.array_equal(ta, tb)
    la, lb = (po.bpr_loss_sum(U, I, b, t, True) for t in (ta, tb))
    assert abs(la - lb) > 1e-3 * la
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(EVAL_NU, EVAL_NI)
        load(c, U, I, b)
        for t, want in ((ta, la), (tb, lb), (ta, la), (ta, la)):
            tol = loss_tol(precision, want, k, score_magnitude(U, I, b, t, True))
            assert abs(c.bpr_eval(0, t, True) - want) <= tol


# ---- 3. multi-wave epoch, linearised

WAVE_LR = 2.0 ** -30


def wave_tol(precision, touches):
    """fp64: 1e-6, 20× above the second-order term and 10⁴ below one missing triplet
    (test_oracle.py::test_bpr_linearised_epoch_anchor).  fp32: every step rounds the running
    row once and its change once, 4·c_max·2⁻²⁴ for the c_max steps that touch one row."""
    return 1e-6 if precision == 64 else max(1e-6, 4 * touches.max() * 2.0 ** -24)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [16, 100])
@pytest.mark.parametrize("atomic_env", [None, "1"])
def test_bpr_multiwave_user_rows_linearised(atomic_env, k, precision, monkeypatch):
    """From U0 = 0 the user rows become ½·lr·Σ (I0[p] − I0[n]) over exactly the epoch's
    triplets: every positive visited once by some wave, every draw as restated, and no
    concurrent change of a user row lost (atomic add; the plan picks it at this shape)."""
    if atomic_env is None:
        monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    else:
        monkeypatch.setenv("QMFX_BPR_ATOMIC_USER", atomic_env)
    nu, ni, users, items = bpr_wave_case()
    I0 = rounded(np.random.default_rng(k).normal(0, 0.1, (ni, k)), precision)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        c.bpr_set_positives(users, items)
        for shuffle in (False, True):
            load(c, np.zeros((nu, k)), I0, np.zeros(ni))
            c.bpr_epoch(32 if shuffle else 31, 5, WAVE_LR, 0.0, 0.0, 0.0, True, shuffle=shuffle)
            waves, atomic = c.bpr_plan()
            assert waves > 1 and atomic == 1, (waves, atomic)
            trip = bpr_wave_triplets(shuffle)
            want = bpr_linear_user(trip, I0, WAVE_LR, nu)
            tol = wave_tol(precision, np.bincount(trip[:, 0], minlength=nu))
            err = np.max(np.abs(c.factors(0) - want)) / np.abs(want).max()
            print("waves %d shuffle %d err U %.3g tol %.3g" % (waves, shuffle, err, tol))
            assert err <= tol, shuffle


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [16, 100])
def test_bpr_multiwave_item_rows_linearised(k, precision, monkeypatch):
    """From I0 = 0, bias0 = 0 the item rows become ½·lr·(Σ_{p=i} U0[u] − Σ_{n=i} U0[u]) and the
    biases ½·lr·(#{p=i} − #{n=i}): no concurrent change of an item row or bias lost."""
    monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    nu, ni, users, items = bpr_wave_case()
    U0 = rounded(np.random.default_rng(k + 1).normal(0, 0.1, (nu, k)), precision)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        c.bpr_set_positives(users, items)
        for shuffle in (False, True):
            load(c, U0, np.zeros((ni, k)), np.zeros(ni))
            c.bpr_epoch(32 if shuffle else 31, 5, WAVE_LR, 0.0, 0.0, 0.0, True, shuffle=shuffle)
            assert c.bpr_plan()[0] > 1
            trip = bpr_wave_triplets(shuffle)
            wI, wb = bpr_linear_item(trip, U0, WAVE_LR, ni)
            tol = wave_tol(precision, np.bincount(trip[:, 1], minlength=ni)
                           + np.bincount(trip[:, 2], minlength=ni))
            ei = np.max(np.abs(c.factors(1) - wI)) / np.abs(wI).max()
            eb = np.max(np.abs(c.bpr_biases() - wb)) / np.abs(wb).max()
            print("shuffle %d err I %.3g bias %.3g tol %.3g" % (shuffle, ei, eb, tol))
            assert ei <= tol, shuffle
            assert eb <= tol, shuffle


# ---- 4. multi-wave epoch at a real learning rate

@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [16, 100])
def test_bpr_multiwave_conserves_item_sums(k, precision, monkeypatch):
    """Two epochs at lr = 0.05 with item_lambda = bias_lambda = 0.  Each of the ntrip steps
    rounds two item rows (and two biases) once as a running value and once as a change:
    |Δ column sum|, |Δ Σ bias| ≤ 4·ntrip·u·max|I|, u the unit roundoff.  The bound must stay
    below a tenth of a typical lost update, lr·¼·median|U0|; fp32 (u = 2⁻²⁴) meets that only
    with few triplets, so it runs the first 50 positives (still one per wave and more)."""
    monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    num_neg, epochs = 5, 2
    nu, ni, users, items = bpr_wave_case(4000 if precision == 64 else 50)
    U0, I0, b0 = init_state(nu, ni, k, precision, k + 2)
    ntrip = epochs * len(users) * num_neg
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        load(c, U0, I0, b0)
        c.bpr_set_positives(users, items)
        for e in range(epochs):
            c.bpr_epoch(41 + e, num_neg, LR, 0.0, 0.025, 0.0, True, shuffle=e > 0)
            assert c.bpr_plan()[0] > 1
        I1, b1 = c.factors(1), c.bpr_biases()
    assert np.abs(I1 - I0).max() > 1e-3  # the epochs did move the rows
    bound = 4 * ntrip * UNIT[precision] * max(np.abs(I0).max(), np.abs(I1).max())
    assert bound < 0.1 * LR * 0.25 * np.median(np.abs(U0)), bound
    dcol = np.max(np.abs(I1.sum(0) - I0.sum(0)))
    dbias = abs(b1.sum() - b0.sum())
    print("ntrip %d Δcolsum %.3g ΔΣbias %.3g bound %.3g" % (ntrip, dcol, dbias, bound))
    assert dcol <= bound
    assert dbias <= bound


# ---- 5. non-finite gradient

@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [16, 130])
def test_bpr_nonfinite_gradient_reported_and_skipped(k, precision, monkeypatch):
    """A NaN in user 3's row makes that user's derivative non-finite: the device skips those
    steps, applies all others and reports "gradients too big" (the reference CHECK-aborts)."""
    monkeypatch.delenv("QMFX_BPR_ATOMIC_USER", raising=False)
    nu, ni, n, bad = 20, 30, 400, 3
    rng = np.random.default_rng(k)
    trip = np.stack([rng.integers(0, nu, n), rng.integers(0, ni, n), rng.integers(0, ni, n)], 1)
    assert 0 < np.sum(trip[:, 0] == bad) < n
    U, I, b = init_state(nu, ni, k, precision, k + 3)
    Ubad = U.copy()
    Ubad[bad, k // 2] = np.nan
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        load(c, Ubad, I, b)
        with pytest.raises(qmf_amd.QmfxError, match="gradients too big"):
            c.bpr_apply(trip, LR, *LAM, True)
        gU, gI, gb = state(c)
        po.bpr_update_seq(U, I, b, trip[trip[:, 0] != bad], LR, *LAM, True)
        keep = np.arange(nu) != bad
        check_state((gU[keep], gI, gb), (U[keep], I, b), TOL[precision], "NaN k=%d" % k)
        keys = np.unique(trip[:, 0] * ni + trip[:, 1])
        c.bpr_set_positives(keys // ni, keys % ni)
        load(c, Ubad, I, b)
        with pytest.raises(qmf_amd.QmfxError, match="gradients too big"):
            c.bpr_epoch(9, 3, LR, *LAM, True, shuffle=True)
