"""qmfx_bpr_fold_in / qmfx_bpr_recommend_fold_in (qmf_amd/csrc/bpr_foldin.hip) on the MI355X
against the numpy reference of tests/bpr_foldin_ref.py (the restated draws, the oracle's user
line on frozen items; anchored on the CPU by tests/test_bpr_foldin.py).

Bounds: the project's single-wave BPR bounds (tests/test_bpr_kernels_gpu.py), 1e-12 (fp64) and
1e-5 (fp32); factors relative to max|.| of the reference rows and the item factors, losses
relative to max(loss, 1).

Shapes: "edges": 300 items, rows of exactly 0, 1, 63, 64, 65, 128 and 129 positives (the edges
of the 64-lane staging) and a dozen short rows; "all_items": 40 items, one row holding all of
them (every draw capped, some equal to the step's own positive).  k = 10, 64, 100, 130, 256 is
E = 1, 1, 2, 3, 4 with and without padding columns."""
import numpy as np
import pytest

import qmf_amd
from qmf_amd._abi import P_f64, P_i32, P_i64, _p
from bpr_foldin_ref import (DECAY, LR, SEED, USER_LAMBDA, batch, batch_draws, batch_reference,
                            fold_in_reference, model, start)

pytestmark = pytest.mark.gpu
TOL = {64: 1e-12, 32: 1e-5}
BAD_GRADIENTS = "gradients too big, try decreasing the learning rate (--init_learning_rate)"

# (batch, k, num_neg, nepochs, use_biases): every k (every E) on both batches' axes, every
# num_neg of {1, 4, 5, 9}, nepochs 1 and 3, biases on and off; each at both precisions
CASES = [("edges", 10, 1, 1, False), ("edges", 64, 4, 3, True), ("edges", 100, 5, 3, False),
         ("edges", 130, 9, 1, True), ("edges", 256, 4, 3, True),
         ("all_items", 10, 5, 3, True), ("all_items", 64, 9, 1, False),
         ("all_items", 130, 4, 3, False), ("all_items", 256, 1, 3, True)]


def context(name, k, precision, biases=True):
    """A context with the shape, the item factors and (with `biases`) the item biases only."""
    ni = batch(name)[0]
    I, b = model(name, k, precision)
    c = qmf_amd.Context(k, precision)
    c.set_shape(3, ni)
    c.set_factors(1, I)
    if biases:
        c.bpr_set_biases(b)
    return c


def fold(c, name, num_neg, nepochs, use_biases, init=None):
    _, rowptr, col = batch(name)
    return c.bpr_fold_in(rowptr, col, SEED[name], nepochs, num_neg, LR, DECAY, USER_LAMBDA,
                         use_biases, init)


def check(got, want, I, precision, what, rows=None):
    (F, losses), (P, lref) = got, want[:2]
    rows = slice(None) if rows is None else rows
    scale = max(np.abs(P).max(), np.abs(I).max())
    ef = np.max(np.abs(F - P)[rows]) / scale
    el = np.max((np.abs(losses - lref) / np.maximum(lref, 1.0))[rows])
    print("%s p=%d: factors %.3g losses %.3g (tol %.3g)" % (what, precision, ef, el, TOL[precision]))
    assert ef <= TOL[precision], what
    assert el <= TOL[precision], what


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name,k,num_neg,nepochs,use_biases", CASES)
def test_fold_in_matches_the_reference(name, k, num_neg, nepochs, use_biases, precision):
    want = batch_reference(name, k, num_neg, nepochs, precision, use_biases)
    assert not want[2].any()
    with context(name, k, precision, biases=use_biases) as c:
        got = fold(c, name, num_neg, nepochs, use_biases)
        again = fold(c, name, num_neg, nepochs, use_biases)
    check(got, want, model(name, k, precision)[0], precision,
          "%s k=%d neg=%d ep=%d b=%d" % (name, k, num_neg, nepochs, use_biases))
    # two identical calls: identical bits
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    if name == "edges":  # the row without positives: its start value, loss 0.0
        assert np.all(got[0][0] == 0.0) and got[1][0] == 0.0


@pytest.mark.parametrize("precision", [64, 32])
def test_fold_in_from_given_start_rows(precision):
    name, k, num_neg, nepochs = "edges", 100, 4, 3
    want = batch_reference(name, k, num_neg, nepochs, precision, True, with_init=True)
    init = start(name, k, precision)
    with context(name, k, precision) as c:
        got = fold(c, name, num_neg, nepochs, True, init=init)
    check(got, want, model(name, k, precision)[0], precision, "init k=%d" % k)
    assert np.array_equal(got[0][0], init[0]) and got[1][0] == 0.0  # the empty row


@pytest.mark.parametrize("precision", [64, 32])
def test_more_rows_than_the_grid(precision, monkeypatch):
    """The launch capped at 3 workgroups: 19 rows reach them by striding; every row matches the
    reference and the uncapped launch bit for bit."""
    name, k, num_neg, nepochs = "edges", 64, 4, 3
    want = batch_reference(name, k, num_neg, nepochs, precision, True)
    with context(name, k, precision) as c:
        full = fold(c, name, num_neg, nepochs, True)
        monkeypatch.setenv("QMFX_BPR_FOLD_GRID", "3")
        got = fold(c, name, num_neg, nepochs, True)
    assert len(batch(name)[1]) - 1 > 3
    check(got, want, model(name, k, precision)[0], precision, "grid 3")
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])


@pytest.mark.parametrize("precision", [64, 32])
def test_the_model_is_left_untouched(precision):
    """factors(0), factors(1), the biases and the positives-dependent launch plan of the last
    epoch are bit-identical before and after both calls."""
    name, k = "edges", 64
    ni, rowptr, col = batch(name)
    I, b = model(name, k, precision)
    rng = np.random.default_rng(2)
    nu = 40
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(nu, ni)
        c.set_factors(0, rng.normal(0, 0.1, (nu, k)))
        c.set_factors(1, I)
        c.bpr_set_biases(b)
        c.bpr_set_positives(rng.integers(0, nu, 500), rng.integers(0, ni, 500))
        c.bpr_epoch(7, 3, LR, 1.0, USER_LAMBDA, 0.0025, True)
        before = (c.factors(0), c.factors(1), c.bpr_biases(), c.bpr_plan())
        fold(c, name, 4, 3, True)
        c.bpr_recommend_fold_in(rowptr, col, SEED[name], 3, 4, LR, DECAY, USER_LAMBDA, 5, True)
        after = (c.factors(0), c.factors(1), c.bpr_biases(), c.bpr_plan())
        # and the positives still drive an epoch
        c.bpr_epoch(8, 3, LR, 1.0, USER_LAMBDA, 0.0025, True)
    for x, y in zip(before[:3], after[:3]):
        assert np.array_equal(x, y)
    assert before[3] == after[3] and before[3][0] >= 1


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("use_biases", [False, True])
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_fold_in_is_recommend_on_the_folded_rows(exclude_seen, use_biases, precision):
    name, k, num_neg, nepochs, topn = "edges", 100, 4, 3, 10
    ni, rowptr, col = batch(name)
    n = len(rowptr) - 1
    I, b = model(name, k, precision)
    with context(name, k, precision) as c:
        F, _ = fold(c, name, num_neg, nepochs, use_biases)
        items, scores, counts, F2 = c.bpr_recommend_fold_in(
            rowptr, col, SEED[name], nepochs, num_neg, LR, DECAY, USER_LAMBDA, topn, use_biases,
            exclude_seen=exclude_seen)
    assert np.array_equal(F, F2)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(n, ni)
        c.set_factors(0, F)
        c.set_factors(1, I)
        c.bpr_set_biases(b)
        c.bpr_set_positives(np.repeat(np.arange(n), np.diff(rowptr)), col.astype(np.int64))
        want = c.recommend(np.arange(n), topn, exclude=2 if exclude_seen else 0,
                           use_biases=use_biases)
    assert np.array_equal(items, want[0])
    assert np.array_equal(scores, want[1])
    assert np.array_equal(counts, want[2])
    assert counts.min() == topn
    if exclude_seen:
        for r in range(n):
            assert not set(items[r].tolist()) & set(col[rowptr[r]:rowptr[r + 1]].tolist())


def raw_fold(c, rowptr, col, seed, nepochs, num_neg, use_biases, nrows=None):
    """qmfx_bpr_fold_in through ctypes: (rc, factors, losses), the outputs kept on failure."""
    rp = np.ascontiguousarray(rowptr, np.int64)
    cl = np.ascontiguousarray(col, np.int32)
    n = len(rp) - 1 if nrows is None else nrows
    F = np.full((max(min(n, len(rp) - 1), 0), c.k), -7.0)
    losses = np.full(len(F), -7.0)
    rc = qmf_amd.lib().qmfx_bpr_fold_in(c.h, n, _p(rp, P_i64), _p(cl, P_i32), None, seed, nepochs,
                                        num_neg, LR, DECAY, USER_LAMBDA, int(use_biases),
                                        _p(F, P_f64), _p(losses, P_f64))
    return rc, F, losses


@pytest.mark.parametrize("precision", [64, 32])
def test_a_nan_item_row_flags_the_call_and_spares_the_other_rows(precision):
    name, k, num_neg, nepochs = "edges", 64, 4, 3
    ni, rowptr, col = batch(name)
    I, b = model(name, k, precision)
    In = I.copy()
    nan_item = int(col[rowptr[3]])  # a positive of the 64-item row
    In[nan_item, 5] = np.nan
    P, lref, flagged = fold_in_reference(rowptr, col, In, b, batch_draws(name, nepochs, num_neg),
                                         nepochs, LR, DECAY, USER_LAMBDA, True,
                                         precision=precision)
    assert flagged[3] and 3 <= (~flagged).sum() < len(flagged)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(3, ni)
        c.set_factors(1, In)
        c.bpr_set_biases(b)
        rc, F, losses = raw_fold(c, rowptr, col, SEED[name], nepochs, num_neg, True)
        assert rc == -4 and qmf_amd.lib().qmfx_last_error().decode() == BAD_GRADIENTS
        with pytest.raises(qmf_amd.QmfxError, match="gradients too big"):
            fold(c, name, num_neg, nepochs, True)
    clean = np.nonzero(~flagged)[0]
    check((F, losses), (P, lref), I, precision, "nan item, clean rows", rows=clean)


def test_validation_failures_launch_nothing():
    name, k = "edges", 10
    ni, rowptr, col = batch(name)
    I, b = model(name, k, 64)
    L = qmf_amd.lib()
    good = dict(seed=1, nepochs=2, num_neg=3, use_biases=False)

    def fails(c, what, rp=rowptr, cl=col, nrows=None, **kw):
        a = dict(good, **kw)
        before = c.solve_stats()["launches"]
        rc, _, _ = raw_fold(c, rp, cl, a["seed"], a["nepochs"], a["num_neg"], a["use_biases"],
                            nrows=nrows)
        assert rc == -1, (what, rc)
        assert L.qmfx_last_error(), what
        assert c.solve_stats()["launches"] == before, what

    with qmf_amd.Context(k, 64) as c:
        c.set_shape(3, ni)
        fails(c, "no item factors")
        c.set_factors(1, I)
        fails(c, "use_biases without biases", use_biases=True)
        bad = rowptr.copy()
        bad[0] = 1
        fails(c, "rowptr[0] != 0", rp=bad)
        bad = rowptr.copy()
        bad[4] = bad[3] - 1
        fails(c, "rowptr decreasing", rp=bad)
        for v in (-1, ni):
            bad = col.copy()
            bad[10] = v
            fails(c, "column out of range", cl=bad)
        fails(c, "repeated column", rp=np.array([0, 3]), cl=np.array([2, 5, 5]))
        fails(c, "descending columns", rp=np.array([0, 3]), cl=np.array([2, 9, 5]))
        fails(c, "nepochs < 1", nepochs=0)
        fails(c, "num_neg < 1", num_neg=0)
        fails(c, "nrows >= 2^31", rp=np.array([0, 0]), cl=np.zeros(1), nrows=1 << 31)
        fails(c, "rowptr[nrows] >= 2^31", rp=np.array([0, 1 << 31]), cl=np.zeros(1))
        for topn in (0, 129):
            before = c.solve_stats()["launches"]
            with pytest.raises(qmf_amd.QmfxError, match="error -1"):
                c.bpr_recommend_fold_in(rowptr, col, 1, 2, 3, LR, DECAY, USER_LAMBDA, topn)
            assert c.solve_stats()["launches"] == before
        # no rows: succeeds and touches nothing
        before = c.solve_stats()["launches"]
        F, losses = c.bpr_fold_in(np.array([0]), np.zeros(0, np.int32), 1, 2, 3, LR, DECAY,
                                  USER_LAMBDA)
        assert F.shape == (0, k) and losses.shape == (0,)
        out = c.bpr_recommend_fold_in(np.array([0]), np.zeros(0, np.int32), 1, 2, 3, LR, DECAY,
                                      USER_LAMBDA, 5)
        assert out[0].shape == (0, 5)
        assert c.solve_stats()["launches"] == before
        # nfactors > 256 cannot be reached: qmfx_create refuses such a context


@pytest.mark.parametrize("precision,k", [(64, 10), (32, 100)])
def test_solve_stats_count_the_stated_work(precision, k):
    name, num_neg, nepochs, topn = "edges", 4, 3, 7
    ni, rowptr, col = batch(name)
    n = len(rowptr) - 1
    kp, esz = -(-k // 16) * 16, precision // 8
    steps = nepochs * num_neg * int(rowptr[-1])
    with context(name, k, precision) as c:
        c.reset_stats()
        fold(c, name, num_neg, nepochs, True)
        s = c.solve_stats()
        assert s["launches"] == 1 and s["ms"] > 0
        assert s["flops"] == steps * 6.0 * k and s["bytes"] == steps * 2.0 * kp * esz
        c.reset_stats()
        c.bpr_recommend_fold_in(rowptr, col, SEED[name], nepochs, num_neg, LR, DECAY, USER_LAMBDA,
                                topn, True)
        s = c.solve_stats()
        assert s["launches"] == 1
        assert s["flops"] == steps * 6.0 * k + 2.0 * n * ni * k
        assert s["bytes"] == steps * 2.0 * kp * esz + float((n + 31) // 32) * ni * k * esz
