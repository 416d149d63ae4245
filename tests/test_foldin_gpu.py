"""Fold-in on the MI355X (qmfx_wals_fold_in, qmfx_recommend_fold_in; csrc/api_foldin.cpp,
csrc/foldin.hip) against numpy.

The case is test_foldin.foldin_case: one new row of every length in test_foldin.LENGTHS (every
whitened bucket edge, a row past the largest bucket, a row with repeated columns) against a
fixed side of 300 rows with seeded factors, α = 40, λ = 0.05.  Every row is compared with
numpy's fp64 solve of the system formed from the fixed side's factors as the device holds them
(qmfx_get_factors), normalised as tests/test_wals_rows_gpu.py does:

  factors  ‖x_dev − x_ref‖∞ / ‖x_ref‖∞ ≤ 1e-9 (fp64) or 1e-4 (fp32);
  loss     |loss_dev − loss_ref| ≤ tol·S_r, tol 1e-9 / 1e-4;
  a row without signals is exactly 0.

The device-built plan (qmfx_fold_in_classes, qmfx_fold_in_order) must equal
test_foldin.plan_reference with the tiling's largest whitened bucket (WB_MAX of
tests/test_wals_rows_gpu.py), and must hold rows in every whitened bucket the tiling has and
in the direct bucket, so that no case passes on one route alone.  The recommendations are
exact: items, scores (bit for bit) and counts equal test_recommend.topn_reference on the
returned factors and the item factors.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from helpers import ROOT, ladder_reference
from test_foldin import (ALPHA, LAM, LENGTHS, NFIXED, bars, classes_of, foldin_case,
                         plan_reference, row_errors)
from test_recommend import topn_reference
from test_wals_rows_gpu import WB_MAX

pytestmark = pytest.mark.gpu

NROWS = len(LENGTHS)


def max_ntn(k, precision, whiten=True):
    return WB_MAX[precision].get((k + 15) // 16, 0) if whiten else 0


def check_rows(tag, F, losses, rowptr, col, val, Y, precision, alpha=ALPHA, lam=LAM):
    xerr, lerr, X, loss = row_errors(F, losses, rowptr, col, val, Y, alpha, lam)
    xbar, lbar = bars(precision)
    print("FOLDIN %s p=%d rows=%d xerr=%.3g (bar %.1g) lerr=%.3g (bar %.1g)"
          % (tag, precision, len(xerr), xerr.max(), xbar, lerr.max(), lbar))
    n = np.diff(rowptr)
    bad = np.flatnonzero(xerr > xbar)
    assert len(bad) == 0, [(int(r), int(n[r]), xerr[r]) for r in bad[:8]]
    bad = np.flatnonzero(lerr > lbar)
    assert len(bad) == 0, [(int(r), int(n[r]), lerr[r]) for r in bad[:8]]
    empty = np.flatnonzero(n == 0)
    assert np.all(F[empty] == 0.0) and np.all(losses[empty] == 0.0)
    return X, loss


def check_plan(c, rowptr, mx):
    """The device's plan equals the numpy restatement; returns the classes."""
    order, wb = plan_reference(rowptr, mx)
    nrows = len(rowptr) - 1
    got = c.fold_in_classes()
    want = classes_of(wb, nrows)
    assert got["whitened"] == want[:8] and got["direct"] == want[8], (got, want)
    assert got["heavy"] == 0 and got["segments"] == 0
    assert np.array_equal(c.fold_in_order(nrows), order)
    return got


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [8, 64, 128, 144])
def test_every_bucket_edge_matches_numpy(k, precision):
    rowptr, col, val, Y0 = foldin_case(k, precision)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(NROWS, NFIXED)
        c.set_factors(1, Y0)
        Y = c.factors(1)
        F, losses, pivoted = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        mx = max_ntn(k, precision)
        got = check_plan(c, rowptr, mx)
    assert np.array_equal(Y, Y0)
    assert pivoted == 0  # SPD systems: the pivoted re-solve must not have repaired a kernel
    # every whitened bucket the tiling has, and the direct bucket, hold rows
    assert all(got["whitened"][b] > 0 for b in range(mx)), got
    assert all(got["whitened"][b] == 0 for b in range(mx, 8)), got
    assert got["direct"] > 0, got
    check_rows("edges k=%d" % k, F, losses, rowptr, col, val, Y, precision)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [64, 128])
def test_agrees_with_a_half_and_leaves_it_untouched(k, precision):
    """The same rows as the context's own side 0: the fold-in equals what qmfx_wals_half(0)
    wrote, its plan has the side's bucket counts, and everything the context reports about the
    half is bit for bit what it was."""
    rowptr, col, val, Y0 = foldin_case(k, precision)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(NROWS, NFIXED)
        c.upload_csr(0, rowptr, col, val)
        c.set_factors(1, Y0)
        total = c.wals_half(0, ALPHA, LAM)
        before = (c.factors(0), c.factors(1), c.row_losses(0), c.failed_rows(), c.row_classes(0))
        F, losses, pivoted = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        after = (c.factors(0), c.factors(1), c.row_losses(0), c.failed_rows(), c.row_classes(0))
        plan = c.fold_in_classes()
        # the next half is not disturbed either
        total2 = c.wals_half(0, ALPHA, LAM)
        again = c.factors(0)
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4] == plan
    assert total2 == total and np.array_equal(again, before[0])
    X, rl = before[0], before[2]
    xbar, lbar = bars(precision)
    full = np.diff(rowptr) > 0
    xerr = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    S = ladder_reference(rowptr, col, val, before[1], ALPHA, LAM)[3]  # the size of a loss's terms
    lerr = np.abs(losses - rl) / np.where(S > 0, S, 1.0)
    print("FOLDIN half k=%d p=%d xerr=%.3g lerr=%.3g" % (k, precision, xerr.max(), lerr.max()))
    assert xerr.max() <= xbar and lerr.max() <= lbar
    assert np.all(F[~full] == 0.0) and pivoted == 0
    assert abs(total - losses.sum()) <= lbar * np.abs(S).sum()


@pytest.mark.parametrize("precision", [64, 32])
def test_no_csr_on_the_context(precision):
    """Shape and item factors only: no CSR, no user factors, a user count unrelated to the
    number of new rows; folding in twice gives the same bits (scratch is reused)."""
    k = 64
    rowptr, col, val, Y0 = foldin_case(k, precision, seed=11)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(3, NFIXED)
        c.set_factors(1, Y0)
        F, losses, _ = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        # a shorter batch next (the scratch keeps its size), then the first one again
        F3, l3, _ = c.wals_fold_in(0, rowptr[:4], col[:rowptr[3]], val[:rowptr[3]], ALPHA, LAM)
        F2, l2, _ = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        Y = c.factors(1)
    check_rows("no-csr", F, losses, rowptr, col, val, Y, precision)
    assert np.array_equal(F, F2) and np.array_equal(losses, l2)
    assert np.array_equal(F3, F[:3]) and np.array_equal(l3, losses[:3])


def test_item_side_fold_in():
    """side = 1: new items against the user factors."""
    k, precision = 64, 64
    rowptr, col, val, Y0 = foldin_case(k, precision, seed=13)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(NFIXED, 5)
        c.set_factors(0, Y0)
        F, losses, _ = c.wals_fold_in(1, rowptr, col, val, ALPHA, LAM)
        with pytest.raises(qmf_amd.QmfxError, match="no factors on the fixed side"):
            c.wals_fold_in(0, rowptr[:2], col[:0], val[:0], ALPHA, LAM)
    check_rows("items", F, losses, rowptr, col, val, Y0, precision)


CHILD = """
import json, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import qmf_amd
from test_foldin import ALPHA, LAM, NFIXED, foldin_case, row_errors
out = []
for precision in (64, 32):
    rowptr, col, val, Y0 = foldin_case(64, precision)
    with qmf_amd.Context(64, precision) as c:
        c.set_shape(1, NFIXED)
        c.set_factors(1, Y0)
        F, losses, pivoted = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        cls, order = c.fold_in_classes(), c.fold_in_order(len(rowptr) - 1)
        Y = c.factors(1)
    xerr, lerr, _, _ = row_errors(F, losses, rowptr, col, val, Y)
    out.append(dict(precision=precision, classes=cls, order=order.tolist(), pivoted=pivoted,
                    xerr=float(xerr.max()), lerr=float(lerr.max())))
print(json.dumps(out))
"""


def test_direct_only_with_whitening_off():
    """QMFX_NO_WHITEN=1 (read when a context is created) in a fresh process: the plan holds
    only the direct bucket, in build_buckets' heaviest-first order, and the rows still match."""
    code = CHILD % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, QMFX_NO_WHITEN="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.splitlines()[-1])
    rowptr = foldin_case(64, 64)[0]
    order, _ = plan_reference(rowptr, 0)
    for o in res:
        print("FOLDIN no-whiten", o["precision"], o["xerr"], o["lerr"])
        assert o["classes"]["whitened"] == [0] * 8 and o["classes"]["direct"] == NROWS
        assert o["order"] == order.tolist() and o["pivoted"] == 0
        xbar, lbar = bars(o["precision"])
        assert o["xerr"] <= xbar and o["lerr"] <= lbar


@pytest.mark.parametrize("precision", [64, 32])
def test_multi_wave_rows_k256(precision):
    """k = 256 at n = 1 (whitened) and n = 200 (past every whitened bucket: the multi-wave
    direct kernel)."""
    k = 256
    rowptr, col, val, Y0 = foldin_case(k, precision, lengths=(1, 200))
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(2, NFIXED)
        c.set_factors(1, Y0)
        F, losses, pivoted = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        got = check_plan(c, rowptr, max_ntn(k, precision))
        Y = c.factors(1)
    assert got["direct"] >= 1 and pivoted == 0   # n = 200 is past every whitened bucket
    check_rows("k256", F, losses, rowptr, col, val, Y, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_pivoted_row(precision):
    """One weight with 1 + αv < 0 makes a row's system indefinite: the Cholesky kernels flag
    it and the pivoted fp64 re-solve answers, as in a half."""
    k = 16
    rng = np.random.default_rng(5)
    Y0 = rng.uniform(-0.5, 0.5, (NFIXED, k))
    lens = np.array([5, 20, 3])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(NFIXED, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.uniform(0.5, 5.0, int(rowptr[-1]))
    val[rowptr[1] + 2] = -30.0  # 1 + 40·(−30) < 0 on row 1
    if precision == 32:
        Y0 = Y0.astype(np.float32).astype(np.float64)
        val = val.astype(np.float32).astype(np.float64)
    # on the CPU: row 1 is indefinite and well conditioned
    sl = slice(int(rowptr[1]), int(rowptr[2]))
    Yr = Y0[col[sl]]
    A = Y0.T @ Y0 + (Yr.T * (ALPHA * val[sl])) @ Yr + LAM * np.eye(k)
    ev = np.linalg.eigvalsh(A)
    assert ev[0] < 0 and np.abs(ev).max() / np.abs(ev).min() < 1e8, ev
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(3, NFIXED)
        c.set_factors(1, Y0)
        F, losses, pivoted = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        Y = c.factors(1)
    assert pivoted >= 1
    check_rows("pivoted", F, losses, rowptr, col, val, Y, precision)


def test_singular_row_fails_like_a_half():
    """An all-zero fixed side with λ = 0: every system is exactly singular (-6)."""
    with qmf_amd.Context(16, 64) as c:
        c.set_shape(2, 10)
        c.set_factors(1, np.zeros((10, 16)))
        with pytest.raises(qmf_amd.QmfxError, match="qmfx error -6"):
            c.wals_fold_in(0, [0, 2], [1, 3], [1.0, 2.0], ALPHA, 0.0)
        # the context still folds in
        c.set_factors(1, np.random.default_rng(0).uniform(-1, 1, (10, 16)))
        F, _, _ = c.wals_fold_in(0, [0, 2], [1, 3], [1.0, 2.0], ALPHA, LAM)
        assert np.all(np.isfinite(F)) and np.any(F != 0)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("topn", [1, 10, 128])
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_fold_in_is_exact(exclude_seen, topn, precision):
    k = 64
    rowptr, col, val, Y0 = foldin_case(k, precision, seed=17)
    # one more row that has seen all but 3 items
    rng = np.random.default_rng(3)
    most = np.sort(rng.choice(NFIXED, NFIXED - 3, replace=False)).astype(np.int32)
    rowptr = np.concatenate([rowptr, [rowptr[-1] + len(most)]])
    col = np.concatenate([col, most])
    val = np.concatenate([val, np.ones(len(most))])
    n = len(rowptr) - 1
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(1, NFIXED)
        c.set_factors(1, Y0)
        items, scores, counts, F = c.recommend_fold_in(rowptr, col, val, ALPHA, LAM, topn,
                                                       exclude_seen)
        Y = c.factors(1)
        F2, losses, _ = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
    assert np.array_equal(F, F2)  # the rows recommended from are the rows fold-in returns
    check_rows("recommend", F, losses, rowptr, col, val, Y, precision)
    seen = [np.unique(col[rowptr[r]:rowptr[r + 1]]) for r in range(n)] if exclude_seen else None
    want = topn_reference(po.test_scores(F, Y, np.arange(n), None), topn, seen)
    for g, w, name in zip((items, scores, counts), want, ("items", "scores", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name
    if exclude_seen:
        assert counts[-1] == min(topn, 3)
        assert np.all(items[-1, counts[-1]:] == -1) and np.all(scores[-1, counts[-1]:] == 0.0)
        assert counts[LENGTHS.index(300)] == min(topn, NFIXED - len(seen[LENGTHS.index(300)]))
    else:
        assert np.all(counts == min(topn, NFIXED))


def test_errors_launch_nothing_and_leave_the_context_working():
    k = 16
    rng = np.random.default_rng(1)
    Y0 = rng.uniform(-0.1, 0.1, (NFIXED, k))
    rp, col, val = np.array([0, 2, 5]), np.array([1, 7, 0, 3, 9]), np.ones(5)
    E = qmf_amd.QmfxError
    with qmf_amd.Context(k, 64) as c:
        with pytest.raises(E, match="error -1: no factors on the fixed side"):
            c.wals_fold_in(0, rp, col, val, ALPHA, LAM)          # no shape at all
        c.set_shape(4, NFIXED)
        with pytest.raises(E, match="error -1: no factors on the fixed side"):
            c.wals_fold_in(0, rp, col, val, ALPHA, LAM)
        with pytest.raises(E, match="error -1: no fold-in planned yet"):
            c.fold_in_classes()
        c.set_factors(1, Y0)
        launches = c.solve_stats()["launches"]
        for side in (-1, 2):
            with pytest.raises(E, match="error -1: side must be 0 or 1"):
                c.wals_fold_in(side, rp, col, val, ALPHA, LAM)
        with pytest.raises(E, match=r"error -1: rowptr\[0\] must be 0"):
            c.wals_fold_in(0, rp + 1, np.zeros(6, np.int32), np.ones(6), ALPHA, LAM)
        with pytest.raises(E, match="error -1: rowptr not monotone"):
            c.wals_fold_in(0, [0, 3, 2, 5], col, val, ALPHA, LAM)
        for bad in (-1, NFIXED):
            with pytest.raises(E, match="error -1: column index out of range"):
                c.wals_fold_in(0, rp, [1, 7, 0, bad, 9], val, ALPHA, LAM)
            with pytest.raises(E, match="error -1: column index out of range"):
                c.recommend_fold_in(rp, [1, 7, 0, bad, 9], val, ALPHA, LAM, 5)
        # new items need the user factors, which this context does not have
        with pytest.raises(E, match="error -1: no factors on the fixed side"):
            c.wals_fold_in(1, rp, col, val, ALPHA, LAM)
        for topn in (0, 129):
            with pytest.raises(E, match="error -1: topn must be in 1..128"):
                c.recommend_fold_in(rp, col, val, ALPHA, LAM, topn)
        with pytest.raises(E, match="error -1: exclude_seen needs the column indices ascending"):
            c.recommend_fold_in(rp, [7, 1, 0, 3, 9], val, ALPHA, LAM, 5, True)   # row 0 descends
        with pytest.raises(E, match="error -1: .*2\\^31"):
            qmf_amd._abi._check(qmf_amd.lib().qmfx_wals_fold_in(
                c.h, 0, 1 << 31, None, None, None, ALPHA, LAM, None, None, None))
        big = np.array([0, 1 << 31], np.int64)  # nnz ≥ 2^31: refused before colidx is read
        with pytest.raises(E, match="error -1: .*2\\^31"):
            qmf_amd._abi._check(qmf_amd.lib().qmfx_wals_fold_in(
                c.h, 0, 1, big.ctypes.data_as(qmf_amd._abi.P_i64), None, None, ALPHA, LAM, None,
                None, None))
        # nothing was launched by any of them, and nrows == 0 touches nothing
        assert c.solve_stats()["launches"] == launches
        F, losses, pivoted = c.wals_fold_in(0, [0], [], [], ALPHA, LAM)
        assert F.shape == (0, k) and c.solve_stats()["launches"] == launches
        with pytest.raises(E, match="no fold-in planned yet"):
            c.fold_in_classes()
        # the context still works after the refused calls
        F, losses, _ = c.wals_fold_in(0, rp, col, val, ALPHA, LAM)
        assert c.solve_stats()["launches"] == launches + 1
        check_rows("after-errors", F, losses, rp.astype(np.int64), col, val, Y0, 64)
        items, scores, counts, F2 = c.recommend_fold_in(rp, col, val, ALPHA, LAM, 5, False)
        assert np.array_equal(F, F2) and counts.tolist() == [5, 5]
