"""The test-set evaluation kernels (qmfx_eval_ranks, csrc/eval.hip) at their own edges, and
what a context keeps over a qmfx_set_shape.

Reference: helpers.eval_scores / eval_reference, plain numpy fp64 (bias or 0, then one rounded
multiply and one rounded add per factor, in factor order; anchored on pyoracle.test_scores by
tests/test_eval.py::test_vectorised_eval_reference_equals_oracle).  An fp32 context's inputs
are rounded to fp32 first, so both sides score the same values.  Bars, the project's own:
label scores bit for bit, `above` exactly equal and as long as the positive labels, Σ score²
within 1e-12 relative (only the summation order differs).

  A  ntest 1, 7, 8, 9, 31, 32, 33, 63, 64, 65 (ni = 200, k = 8): the `t >= ntest` break inside
     a wave, a last group of one user, pptr at a group edge.  0..6 labels per user; from
     ntest = 7 on one user has no labels and one only non-positive ones, and the last user
     always has a positive.  ntest = 1 cannot hold those three at once: it runs the single
     user three times (with positives, without labels, with non-positive labels only).
  B  ni 1, 2, 63, 64, 65, 127, 128, 129 (ntest = 33, k = 8): less than a tile, tile edges, a
     ragged last tile; one user's positives are all ni items, so its counts are the strictly
     higher scores among the positives themselves.
  C  k 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256 (ni = 130, ntest = 9): the
     unrolled full LDS stage mixed with the runtime tail; biases on for every second k.
  D  50 users in 4100 test slots over 5000 items: 129 groups (the last of 4 users, one partial
     wave) leave 27 chunks of 3 tiles, the last chunk of 8 items (asserted from
     helpers.eval_chunks, so a retune of the grid cannot quietly make the chunks single
     tiles again).  With item biases, 100 identical item rows in other chunks than their
     original, ten users whose scores ascend with the item index, a zero user row whose
     positives score 0.0 and -0.0, and one item labelled twice for a user.
  E  one group whose running count of positives reaches 2047, 2048 and 2049 (EV_CAP = 2048 LDS
     counters) inside its user 20; user 21 has 5 more positives except at 2047.  Once over
     2100 items (one group gives 33 chunks of a single tile each: no shape with 2100 items
     has fewer) and once as group 64 of case D's shape, where 27 workgroups of 3 tiles flush
     their LDS counters into, and add past the cap directly to, the same global slots.
  F  no test users at all; five test users without a label.
  Reshape: (200, 400) -> (150, 300) with every index below the new counts, so the parent
     library's stale buffers are larger than needed and nothing is read or written out of
     bounds whichever library runs: eval_ranks, bpr_epoch and bpr_biases fail until labels,
     positives and biases are set again, fresh ones give the new shape's reference, and the
     same shape again keeps the labels.

Measured on an MI355X: the 79 cases here together with the 8 of test_eval_gpu.py take 1.5 s
(the slowest, the first one, 0.25 s; cases D and E 0.06 s each); largest Σ score² relative
error 5.6e-16 beside the 1e-12 bar.  All pass on the unmodified kernels (no kernel bug found).

Single-line mutants of the library, each run once (new cases failing of 79; cases of the
three older tests of test_eval_gpu.py failing too, of 8):
  __ballot(valid && s > sp[j]) without `valid` .................. 69 new, 5 old
  s >= sp[j] .................................................... 73 new, 5 old
  acc[g] = b0 set once before the tile loop ..................... 5 new (D and E over several
      tiles: nothing else has a second tile), 0 old
  mul_add_rn contracted to a fused multiply-add ................. 40 new, 2 old (the fp64
      contexts only: the product of two fp32 values is exact in fp64, so fusing changes no bit)
  the host's Σ score² over the chunks stops at nch - 1 .......... 75 new, 5 old
  the parent commit's host units (no reshape fix) ............... the 2 reshape-drops tests
      ("DID NOT RAISE"), 0 old
"""
import functools

import numpy as np
import pytest

import qmf_amd
from helpers import eval_chunks, eval_reference, eval_scores

pytestmark = pytest.mark.gpu

VALUES = (-1.0, 0.0, 0.5, 1.0, 2.0, 4.0)   # label values: > 0 is a positive
EV_CAP = 2048                                # LDS counters of a workgroup (eval.hip)


def _rounded(a, prec):
    """The values a context of this precision holds."""
    a = np.asarray(a, np.float64)
    return a.astype(np.float32).astype(np.float64) if prec == 32 else a


def _factors(rng, nu, ni, k, prec, bias):
    U = _rounded(rng.normal(0, 0.3, (nu, k)), prec)
    I = rng.normal(0, 0.3, (ni, k))
    if ni >= 12:
        I[7] = I[3]     # exact ties: identical item rows score identically
        I[11] = I[3]
    b = _rounded(rng.normal(0, 0.5, ni), prec) if bias else None
    return U, _rounded(I, prec), b


def _labels(rng, ntest, ni, planted=None):
    """A label CSR over the test slots: a planted slot's (items, values), otherwise 0..6
    distinct items (every fifth slot starts with the tied items 3, 7, 11) with values drawn
    from VALUES."""
    planted = planted or {}
    rowptr, items, values = [0], [], []
    for t in range(ntest):
        if t in planted:
            it, v = planted[t]
        else:
            m = min(int(rng.integers(0, 7)), ni)
            it = np.sort(rng.choice(ni, m, replace=False))
            if t % 5 == 0 and ni >= 12 and m >= 3:
                it = np.concatenate([[3, 7, 11], np.setdiff1d(it, [3, 7, 11])[:m - 3]])
            v = rng.choice(VALUES, len(it))
        items.extend(np.asarray(it).tolist())
        values.extend(np.asarray(v, np.float64).tolist())
        rowptr.append(len(items))
    return np.array(rowptr, np.int64), np.array(items, np.int64), np.array(values, np.float64)


def _device(prec, k, U, I, b, users, labels, ctx=None):
    """eval_ranks of the label set on a fresh context (or on `ctx`, shape and factors set)."""
    if ctx is not None:
        ctx.eval_set_labels(users, *labels)
        return ctx.eval_ranks(use_biases=b is not None)
    with qmf_amd.Context(k, prec) as c:
        c.set_shape(len(U), len(I))
        c.set_factors(0, U)
        c.set_factors(1, I)
        if b is not None:
            c.bpr_set_biases(b)
        return _device(prec, k, U, I, b, users, labels, c)


def _assert_equal(got, ref, values):
    ls, above, sq = got
    rls, rabove, rsq = ref
    err = float(np.max(np.abs(sq - rsq) / np.maximum(np.abs(rsq), 1e-300), initial=0.0))
    print("sq rel err %.3g" % err)
    assert len(above) == len(rabove) == int(np.count_nonzero(values > 0))
    assert np.array_equal(ls, rls)                         # bit-exact label scores
    assert np.array_equal(above, rabove), np.nonzero(above != rabove)[0][:10]   # exact counts
    assert sq.shape == rsq.shape and np.all(np.abs(sq - rsq) <= 1e-12 * np.abs(rsq))


def _check(prec, k, U, I, b, users, labels, S=None, rows=None):
    """Device against reference; S[rows[t]] are slot t's scores when the caller shares them."""
    if S is None:
        S, rows = eval_scores(U, I, users, b), np.arange(len(users))
    ref = eval_reference(S, rows, *labels)
    got = _device(prec, k, U, I, b, users, labels)
    _assert_equal(got, ref, labels[2])
    return got, ref


# ---- A: user-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("ntest", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65])
def test_eval_user_count_edges(ntest, prec):
    rng = np.random.default_rng(1000 + ntest)
    nu, ni, k = 80, 200, 8
    U, I, _ = _factors(rng, nu, ni, k, prec, False)
    users = rng.choice(nu, ntest, replace=False)
    some = (np.array([3, 7, 50, 199]), np.array([1.0, 2.0, -1.0, 0.5]))
    none = (np.array([], np.int64), np.array([]))
    nonpos = (np.array([0, 7, 64]), np.array([-1.0, 0.0, -1.0]))
    if ntest == 1:
        plans = [{0: some}, {0: none}, {0: nonpos}]
    else:
        plans = [{0: none, ntest // 2: nonpos, ntest - 1: some}]
    for planted in plans:
        labels = _labels(rng, ntest, ni, planted)
        assert np.max(np.diff(labels[0])) <= 6
        _check(prec, k, U, I, None, users, labels)


# ---- B: item-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("ni", [1, 2, 63, 64, 65, 127, 128, 129])
def test_eval_item_count_edges(ni, prec):
    rng = np.random.default_rng(2000 + ni)
    nu, k, ntest, dense = 40, 8, 33, 5
    U, I, _ = _factors(rng, nu, ni, k, prec, False)
    users = rng.choice(nu, ntest, replace=False)
    labels = _labels(rng, ntest, ni, {dense: (np.arange(ni), np.ones(ni)),
                                      ntest - 1: (np.array([ni - 1]), np.array([1.0]))})
    (ls, above, _), _ = _check(prec, k, U, I, None, users, labels)
    # every item of the dense user is a positive: its counts are ranks among the positives
    rowptr, _, values = labels
    p0 = int(np.count_nonzero(values[:rowptr[dense]] > 0))
    ps = ls[rowptr[dense]:rowptr[dense + 1]]
    assert above[p0:p0 + ni].tolist() == [int(np.count_nonzero(ps > s)) for s in ps]


# ---- C: factor-count edges -------------------------------------------------------------------
KS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("k", KS)
def test_eval_factor_count_edges(k, prec):
    rng = np.random.default_rng(3000 + k)
    nu, ni, ntest = 20, 130, 9
    U, I, b = _factors(rng, nu, ni, k, prec, bias=KS.index(k) % 2 == 0)
    users = rng.choice(nu, ntest, replace=False)
    labels = _labels(rng, ntest, ni, {ntest - 1: (np.array([0, 64, 129]), np.array([1.0, 2.0, 1.0]))})
    _check(prec, k, U, I, b, users, labels)


# ---- D: several tiles per chunk --------------------------------------------------------------
D_NU, D_NI, D_K, D_NTEST = 50, 5000, 8, 4100
D_ZERO = 10                          # the zero user row
D_POS0 = np.arange(1000, 1100)       # items that score 0.0 for it (chunk 5)
D_NEG0 = np.arange(3000, 3100)       # items that score -0.0 for it (chunk 15)
D_ZERO_SLOTS = (777, D_NTEST - 3)    # the second one in the last, partial wave
D_TWICE_SLOT = 300


@functools.lru_cache(maxsize=None)
def _tiles_case(prec):
    """Case D's factors, biases, test slots and the 50 users' scores.  Read-only, shared."""
    rng = np.random.default_rng(77)
    U = rng.normal(0, 0.3, (D_NU, D_K))
    I = rng.normal(0, 0.3, (D_NI, D_K))
    U[:10] = 0.0
    U[:10, 0] = 1.0
    I[:, 0] = np.arange(D_NI) / 64.0      # users 0..9: score = i/64 + bias_i, ascending
    b = rng.uniform(-1.0, 1.0, D_NI) / 256.0   # |bias| < half the step 1/64
    # the zero row is all -0.0: its products are -0.0 with the non-negative rows of D_NEG0, so
    # a bias of -0.0 stays -0.0 there, and a bias of 0.0 stays 0.0 whatever the products' signs
    U[D_ZERO] = -0.0
    I[D_NEG0, 1:] = np.abs(I[D_NEG0, 1:])
    b[D_POS0], b[D_NEG0] = 0.0, -0.0
    I[4000:4100], b[4000:4100] = I[100], b[100]   # ties across tiles and chunks
    U, I, b = _rounded(U, prec), _rounded(I, prec), _rounded(b, prec)
    users = np.concatenate([rng.permutation(D_NU), rng.integers(0, D_NU, D_NTEST - D_NU)])
    users[list(D_ZERO_SLOTS)] = D_ZERO
    S = eval_scores(U, I, np.arange(D_NU), b)
    for a in (U, I, b, users, S):
        a.setflags(write=False)
    return U, I, b, users, S


def _tiles_labels(rng, extra=None):
    ties = (np.array([100, 4000, 4031, 4032, 4099, 2500]), np.array([1.0, 2.0, 1.0, 0.5, 4.0, -1.0]))
    zero = (np.array([1000, 1050, 3000, 3050, 2000]), np.ones(5))
    planted = {t: ties for t in range(0, D_NTEST, 41)}
    planted.update({t: zero for t in D_ZERO_SLOTS})
    planted[D_TWICE_SLOT] = (np.array([17, 4990, 4990]), np.array([1.0, 2.0, 1.0]))
    planted[D_NTEST - 1] = (np.array([4992, 4999]), np.array([1.0, 1.0]))   # the last chunk's items
    planted.update(extra or {})
    return _labels(rng, D_NTEST, D_NI, planted)


def test_eval_tiles_case_grid():
    """The arithmetic cases D and E rest on, from the restatement of eval_chunks."""
    assert -(-D_NTEST // 32) == 129 and D_NTEST - 128 * 32 == 4    # last group: one partial wave
    n, chunk = eval_chunks(D_NTEST, D_NI)
    assert (n, chunk) == (27, 3 * 64) and D_NI - 26 * chunk == 8
    assert 4096 // 129 == 31                                       # divided into 31 first
    assert 100 // chunk != 4000 // chunk != 4099 // chunk          # the tied block's chunks
    assert eval_chunks(32, 2100) == (33, 64)                       # case E alone: single tiles


@pytest.mark.parametrize("prec", [64, 32])
def test_eval_chunks_of_several_tiles(prec):
    U, I, b, users, S = _tiles_case(prec)
    assert eval_chunks(len(users), len(I)) == (27, 192)
    assert set(users.tolist()) == set(range(D_NU))
    z = S[D_ZERO]
    assert np.all(z[D_POS0] == 0.0) and not np.any(np.signbit(z[D_POS0]))
    assert np.all(z[D_NEG0] == 0.0) and np.all(np.signbit(z[D_NEG0]))
    asc = np.delete(S[3], np.arange(4000, 4100))
    assert np.all(np.diff(asc) > 0)
    labels = _tiles_labels(np.random.default_rng(78))
    (_, above, _), _ = _check(prec, D_K, U, I, b, users, labels, S, users)
    # 0.0 and -0.0 compare as equal: above a zero score are exactly the positive scores
    rowptr, _, values = labels
    for t in D_ZERO_SLOTS:
        p0 = int(np.count_nonzero(values[:rowptr[t]] > 0))
        assert above[p0:p0 + 4].tolist() == [int(np.count_nonzero(z > 0.0))] * 4


# ---- E: the LDS counter cap ------------------------------------------------------------------
def _cap_group(rng, ni, reach):
    """32 users' labels: users 0..19 two positives each, user 20 as many as bring the group's
    running count to `reach`, user 21 five more (none when reach < EV_CAP), users 22..31 two
    non-positive labels each."""
    out = []
    for g in range(32):
        m = 2 if g < 20 else reach - 40 if g == 20 else 5 if g == 21 and reach >= EV_CAP else 0
        it = np.sort(rng.choice(ni, m, replace=False)) if m else np.array([5, 9])
        out.append((it, np.ones(m) if m else np.array([-1.0, 0.0])))
    return out


@pytest.mark.parametrize("reach", [EV_CAP - 1, EV_CAP, EV_CAP + 1])
def test_eval_counter_cap_single_tile_chunks(reach):
    rng = np.random.default_rng(5000 + reach)
    nu, ni, k = 32, 2100, 8
    U, I, b = _factors(rng, nu, ni, k, 64, True)
    users = rng.permutation(nu)
    labels = _labels(rng, 32, ni, dict(enumerate(_cap_group(rng, ni, reach))))
    rowptr, _, values = labels
    assert int(np.count_nonzero(values[:rowptr[21]] > 0)) == reach
    _check(64, k, U, I, b, users, labels)


@pytest.mark.parametrize("reach", [EV_CAP - 1, EV_CAP, EV_CAP + 1])
def test_eval_counter_cap_several_tiles(reach):
    """The same group as group 64 of case D: each of its 27 workgroups holds the counters of
    the first 2048 positives over 3 tiles, flushes them into the global slots the other 26
    add to, and adds the later positives' counts to their slots directly."""
    U, I, b, users, S = _tiles_case(64)
    rng = np.random.default_rng(6000 + reach)
    t0 = 64 * 32
    group = {t0 + g: lab for g, lab in enumerate(_cap_group(rng, D_NI, reach))}
    labels = _tiles_labels(rng, group)
    rowptr, _, values = labels
    pos_before = lambda t: int(np.count_nonzero(values[:rowptr[t]] > 0))
    assert pos_before(t0 + 21) - pos_before(t0) == reach
    _check(64, D_K, U, I, b, users, labels, S, users)


# ---- F: empty inputs -------------------------------------------------------------------------
def test_eval_no_test_users():
    rng = np.random.default_rng(7)
    U, I, _ = _factors(rng, 6, 70, 8, 64, False)
    none = np.array([], np.int64)
    got = _device(64, 8, U, I, None, none, (np.zeros(1, np.int64), none, np.array([])))
    assert [a.shape for a in got] == [(0,)] * 3


@pytest.mark.parametrize("prec", [64, 32])
def test_eval_test_users_without_labels(prec):
    rng = np.random.default_rng(8)
    U, I, b = _factors(rng, 6, 70, 8, prec, True)
    users = np.array([5, 0, 3, 3, 1])
    labels = (np.zeros(6, np.int64), np.array([], np.int64), np.array([]))
    (ls, above, _), _ = _check(prec, 8, U, I, b, users, labels)
    assert ls.shape == above.shape == (0,)


# ---- what a context keeps over set_shape -----------------------------------------------------
# Every reshape shrinks, and every index is below the new counts: see the module docstring.
OLD, NEW = (200, 400), (150, 300)


def _shape_case(prec=64):
    rng = np.random.default_rng(9)
    k, ntest = 8, 40
    U, I, b = _factors(rng, *OLD, k, prec, True)
    users = rng.choice(NEW[0], ntest, replace=False)
    labels = _labels(rng, ntest, NEW[1])
    return k, U, I, b, users, labels


def _load(c, U, I, b=None):
    c.set_shape(len(U), len(I))
    c.set_factors(0, U)
    c.set_factors(1, I)
    if b is not None:
        c.bpr_set_biases(b)


def test_reshape_drops_the_eval_labels():
    k, U, I, b, users, labels = _shape_case()
    with qmf_amd.Context(k, 64) as c:
        _load(c, U, I, b)
        c.eval_set_labels(users, *labels)
        c.eval_ranks(use_biases=True)
        _load(c, U[:NEW[0]], I[:NEW[1]])
        with pytest.raises(qmf_amd.QmfxError, match="no test labels"):
            c.eval_ranks()


def test_reshape_drops_the_bpr_positives_and_biases():
    k, U, I, b, users, labels = _shape_case()
    rng = np.random.default_rng(10)
    pu, pi = rng.integers(0, NEW[0], 500), rng.integers(0, NEW[1], 500)
    b_new = rng.normal(0, 0.5, NEW[1])
    with qmf_amd.Context(k, 64) as c:
        _load(c, U, I, b)
        c.bpr_set_positives(pu, pi)
        assert np.array_equal(c.bpr_biases(), b)
        _load(c, U[:NEW[0]], I[:NEW[1]])
        with pytest.raises(qmf_amd.QmfxError, match="no biases"):
            c.bpr_biases()
        with pytest.raises(qmf_amd.QmfxError, match="no positives"):
            c.bpr_epoch(1, 1, 0.05, 1.0, 0.025, 0.0025, True)
        c.bpr_set_biases(b_new)
        got = c.bpr_biases()
        assert got.shape == (NEW[1],) and np.array_equal(got, b_new)


@pytest.mark.parametrize("prec", [64, 32])
def test_fresh_labels_after_reshape_match_the_new_shape(prec):
    k, U, I, b, users, labels = _shape_case(prec)
    Un, In, bn = U[:NEW[0]] * 0.5, I[:NEW[1]][::-1].copy(), b[:NEW[1]][::-1].copy()
    with qmf_amd.Context(k, prec) as c:
        _load(c, U, I, b)
        c.eval_set_labels(users, *labels)
        c.eval_ranks(use_biases=True)
        _load(c, Un, In, bn)
        got = _device(prec, k, Un, In, bn, users, labels, c)
    ref = eval_reference(eval_scores(Un, In, users, bn), np.arange(len(users)), *labels)
    _assert_equal(got, ref, labels[2])


def test_same_shape_again_keeps_the_labels():
    k, U, I, b, users, labels = _shape_case()
    with qmf_amd.Context(k, 64) as c:
        _load(c, U, I, b)
        c.eval_set_labels(users, *labels)
        before = c.eval_ranks(use_biases=True)
        c.set_shape(*OLD)
        after = c.eval_ranks(use_biases=True)
        assert np.array_equal(c.bpr_biases(), b)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    _assert_equal(after, eval_reference(eval_scores(U, I, users, b), np.arange(len(users)),
                                        *labels), labels[2])
