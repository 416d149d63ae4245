"""Explanations on the MI355X (qmfx_wals_explain, qmfx_wals_explain_rows; csrc/api_explain.cpp,
csrc/explain.hip) against numpy.

The case is test_foldin.foldin_case uploaded as side 0 against its 300 fixed rows, α = 40,
λ = 0.05: rows of every length in test_foldin.LENGTHS (0, 1, the 16-signal staging edges, 300
with repeated columns; zero-valued signals).  Row r explains a target list whose length rotates
through 0, 1, B, B + 1, B + 2 (B = 8, the kernel's right-hand-side block; the longest list
repeats a target); half of a list are columns of the row itself, the rest are drawn from all.
k covers one padded tile (1, 17), the LDS sizes up to the last (64, 128), the first scratch
size (144) and the largest system (256).

The reference is test_explain.explain_reference: numpy fp64 on the factors the device holds
(qmfx_get_factors), G = YᵀY in fp64.  Bars: 1e-9 (fp64) and 1e-4 (fp32), the project's.  On
exactly these cases, on the CPU: an fp32-accumulated G moves the fp64 result by at most 3.2e-7
of ‖ref‖∞, cond(A) ≤ 75, and total = y_t·x̂ holds in fp64 to 2.4e-14.
  full vector  per pair ‖dev − ref‖∞ ≤ bar·‖ref‖∞
  totals       |total − Σref| ≤ bar·Σ|ref|
  top-M        sources, positions, contributions (bit for bit) and counts equal a stable
               descending sort of the device's own full vector; the tail is −1 / 0.0
"""
import functools

import numpy as np
import pytest

import qmf_amd
from helpers import signed_ladder_case
from test_explain import explain_reference
from test_foldin import ALPHA, LAM, LENGTHS, NFIXED, foldin_case

pytestmark = pytest.mark.gpu

NROWS = len(LENGTHS)
BLOCK = 8  # kExplainRhs
LIST_LENGTHS = (0, 1, BLOCK, BLOCK + 1, BLOCK + 2)
KS = [1, 17, 64, 128, 144, 256]
E = qmf_amd.QmfxError


def bar(precision):
    return 1e-9 if precision == 64 else 1e-4


@functools.lru_cache(maxsize=None)
def case(k, precision):
    """(rowptr, col, val, Y0, rows, qptr, targets): the fold-in case and its queries."""
    rowptr, col, val, Y0 = foldin_case(k, precision)
    rng = np.random.default_rng(100 + k)
    lists = []
    for r in range(NROWS):
        n = LIST_LENGTHS[r % len(LIST_LENGTHS)]
        own = col[rowptr[r]:rowptr[r + 1]].astype(np.int64)
        t = np.concatenate([rng.choice(own, min(n // 2, len(own)), replace=False),
                            rng.integers(0, NFIXED, n)])[:n]
        if n == BLOCK + 2:
            t[-1] = t[0]
        lists.append(t.astype(np.int64))
    qptr = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    out = (rowptr, col, val, Y0, np.arange(NROWS, dtype=np.int64), qptr, np.concatenate(lists))
    for a in out:
        a.setflags(write=False)
    return out


def test_the_queries_cover_what_they_should():
    rowptr, col, _, _, _, qptr, targets = case(64, 64)
    assert sorted(set(np.diff(qptr).tolist())) == sorted(LIST_LENGTHS)
    own = other = 0
    for r in range(NROWS):
        t = targets[qptr[r]:qptr[r + 1]]
        mine = np.isin(t, col[rowptr[r]:rowptr[r + 1]])
        own, other = own + int(mine.sum()), other + int((~mine).sum())
        if len(t) == BLOCK + 2:
            assert t[-1] == t[0]
    assert own > 0 and other > 0
    # every list length meets the empty row or a long row at some point of the rotation
    assert np.diff(qptr)[LENGTHS.index(300)] > 0


def context(k, precision, csr=True):
    rowptr, col, val, Y0 = case(k, precision)[:4]
    c = qmf_amd.Context(k, precision)
    c.set_shape(NROWS, NFIXED)
    if csr:
        c.upload_csr(0, rowptr, col, val)
    c.set_factors(1, Y0)
    return c


@functools.lru_cache(maxsize=None)
def reference(k, precision):
    """explain_reference of every pair, on the factors an fp32 / fp64 context holds (the case
    rounds them first, so they are what qmfx_get_factors returns)."""
    rowptr, col, val, Y, rows, qptr, targets = case(k, precision)
    ref = []
    for q in range(NROWS):
        for t in targets[qptr[q]:qptr[q + 1]]:
            ref.append(explain_reference(rowptr, col, val, Y, q, int(t), ALPHA, LAM)[0])
    return ref


def check_selection(tag, out, rowptr, col, rows, qptr, topm):
    """The lists against a stable descending sort of the device's own full vector."""
    sources, positions, contribs, counts, totals, (allv, allptr) = out
    assert sources.shape == positions.shape == contribs.shape == (len(totals), topm)
    pair_row = np.repeat(rows, np.diff(qptr))
    for p, r in enumerate(pair_row):
        v = allv[allptr[p]:allptr[p + 1]]
        n = int(rowptr[r + 1] - rowptr[r])
        assert len(v) == n
        cnt = min(topm, n)
        assert counts[p] == cnt, (tag, p, counts[p], cnt)
        order = np.argsort(-v, kind="stable")[:cnt]
        assert np.array_equal(positions[p, :cnt], order), (tag, p)
        assert np.array_equal(sources[p, :cnt], col[rowptr[r] + order]), (tag, p)
        assert np.array_equal(contribs[p, :cnt].view(np.int64), v[order].view(np.int64)), (tag, p)
        assert np.all(sources[p, cnt:] == -1) and np.all(positions[p, cnt:] == -1)
        assert np.all(contribs[p, cnt:] == 0.0) and not np.any(np.signbit(contribs[p, cnt:]))
        if n == 0:
            assert totals[p] == 0.0


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", KS)
def test_contributions_match_numpy_and_the_lists_match_the_full_vector(k, precision):
    rowptr, col, val, Y0, rows, qptr, targets = case(k, precision)
    with context(k, precision) as c:
        assert np.array_equal(c.factors(1), Y0)
        outs = {m: c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, m, full=True)
                for m in (1, 5, 128)}
    ref = reference(k, precision)
    allv, allptr = outs[5][5]
    totals = outs[5][4]
    assert len(ref) == len(totals) == len(targets)
    verr = terr = 0.0
    for p, want in enumerate(ref):
        got = allv[allptr[p]:allptr[p + 1]]
        assert got.shape == want.shape
        if len(want):
            verr = max(verr, np.max(np.abs(got - want)) / np.max(np.abs(want)))
            terr = max(terr, abs(totals[p] - want.sum()) / np.abs(want).sum())
        else:
            assert totals[p] == 0.0
    print("EXPLAIN k=%d p=%d pairs=%d verr=%.3g terr=%.3g (bar %.1g)"
          % (k, precision, len(ref), verr, terr, bar(precision)))
    assert verr <= bar(precision) and terr <= bar(precision)
    for m, out in outs.items():
        # the full vector and the totals do not depend on topm
        assert np.array_equal(out[5][0].view(np.int64), allv.view(np.int64))
        assert np.array_equal(out[4].view(np.int64), totals.view(np.int64))
        check_selection("k=%d p=%d m=%d" % (k, precision, m), out, rowptr, col, rows, qptr, m)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [17, 144])
def test_tie_rule(k, precision):
    """One row holds the same column three times with equal values: the three contributions
    are bitwise equal and rank by position, next to each other."""
    rng = np.random.default_rng(9)
    Y0 = rng.uniform(-0.5, 0.5, (NFIXED, k)).astype(np.float32).astype(np.float64)
    col = np.array([4, 9, 9, 20, 9, 31], np.int32)
    val = np.array([1.0, 2.0, 2.0, 0.5, 2.0, 3.0])
    rowptr = np.array([0, 6], np.int64)
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(1, NFIXED)
        c.set_factors(1, Y0)
        for m in (2, 6):
            src, pos, con, cnt, tot, (allv, _) = c.wals_explain_rows(
                0, rowptr, col, val, [0, 1], [9], ALPHA, LAM, m, full=True)
            assert allv[1] == allv[2] == allv[4]
            order = np.argsort(-allv, kind="stable")[:m]
            assert pos[0].tolist() == order.tolist() and cnt[0] == m
            assert np.array_equal(con[0], allv[order]) and src[0].tolist() == col[order].tolist()
        at = pos[0].tolist()
        assert at.index(1) + 1 == at.index(2) and at.index(2) + 1 == at.index(4)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [17, 128, 144])
def test_rows_variant_is_bit_identical_without_a_csr(k, precision):
    rowptr, col, val, Y0, rows, qptr, targets = case(k, precision)
    with context(k, precision) as c:
        a = c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, 5, full=True)
    with context(k, precision, csr=False) as c:
        b = c.wals_explain_rows(0, rowptr, col, val, qptr, targets, ALPHA, LAM, 5, full=True)
        with pytest.raises(E, match="error -1: no interactions uploaded for this side"):
            c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, 5)
    for x, y in zip(a[:5] + a[5], b[:5] + b[5]):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                              y.view(np.int64) if y.dtype == np.float64 else y)


@pytest.mark.parametrize("k", KS)
def test_total_is_the_score_of_the_folded_in_row(k):
    """The independent route (precision 64): total = y_t·x̂ with x̂ from qmfx_wals_fold_in."""
    rowptr, col, val, Y0, rows, qptr, targets = case(k, 64)
    with context(k, 64, csr=False) as c:
        totals = c.wals_explain_rows(0, rowptr, col, val, qptr, targets, ALPHA, LAM, 1)[4]
        X = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)[0]
    ref = reference(k, 64)
    pair_row = np.repeat(rows, np.diff(qptr))
    worst = 0.0
    for p, (r, t) in enumerate(zip(pair_row, targets)):
        scale = np.abs(ref[p]).sum()
        if scale > 0:
            worst = max(worst, abs(totals[p] - Y0[t] @ X[r]) / scale)
        else:
            assert totals[p] == 0.0
    print("EXPLAIN fold-in route k=%d err=%.3g" % (k, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [64, 144])
def test_leaves_the_context_untouched(k, precision):
    rowptr, col, val, Y0, rows, qptr, targets = case(k, precision)
    with context(k, precision) as c:
        total = c.wals_half(0, ALPHA, LAM)
        before = (c.factors(0), c.factors(1), c.row_losses(0), c.failed_rows(), c.row_classes(0))
        c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, 5, full=True)
        c.wals_explain_rows(0, rowptr, col, val, qptr, targets, ALPHA, LAM, 5)
        after = (c.factors(0), c.factors(1), c.row_losses(0), c.failed_rows(), c.row_classes(0))
        csr = c.download_csr(0)
        total2 = c.wals_half(0, ALPHA, LAM)
        again = c.factors(0)
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    assert np.array_equal(csr[0], rowptr) and np.array_equal(csr[1], col)
    assert np.array_equal(csr[2], val)
    assert total2 == total and np.array_equal(again, before[0])


def test_errors_launch_nothing_and_leave_the_context_working():
    k = 16
    rowptr, col, val, Y0, rows, qptr, targets = case(k, 64)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(NROWS, NFIXED)
        with pytest.raises(E, match="error -1: no factors on the other side"):
            c.wals_explain_rows(0, rowptr, col, val, qptr, targets, ALPHA, LAM, 5)
        c.upload_csr(0, rowptr, col, val)
        with pytest.raises(E, match="error -1: no factors on the other side"):
            c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, 5)
        c.set_factors(1, Y0)
        launches = c.solve_stats()["launches"]
        both = (lambda side, r, qp, t, m: c.wals_explain(side, r, qp, t, ALPHA, LAM, m),
                lambda side, r, qp, t, m: c.wals_explain_rows(side, rowptr, col, val, qp, t,
                                                              ALPHA, LAM, m))
        for f in both:
            for side in (-1, 2):
                with pytest.raises(E, match="error -1: side must be 0 or 1"):
                    f(side, rows, qptr, targets, 5)
            for m in (0, 129):
                with pytest.raises(E, match="error -1: topm must be in 1..128"):
                    f(0, rows, qptr, targets, m)
            for bad in (-1, NFIXED):
                t = targets.copy()
                t[3] = bad
                with pytest.raises(E, match="error -1: target out of range"):
                    f(0, rows, qptr, t, 5)
            qp = qptr.copy()
            qp[2], qp[3] = qptr[3], qptr[2]
            assert qp[3] < qp[2]
            with pytest.raises(E, match="error -1: qptr not monotone"):
                f(0, rows, qp, targets, 5)
        for bad in (-1, NROWS):
            r = rows.copy()
            r[1] = bad
            with pytest.raises(E, match="error -1: row out of range"):
                c.wals_explain(0, r, qptr, targets, ALPHA, LAM, 5)
        with pytest.raises(E, match="error -1: column index out of range"):
            c.wals_explain_rows(0, [0, 1], [NFIXED], [1.0], [0, 1], [0], ALPHA, LAM, 5)
        # the other side has neither a CSR (first form) nor fixed-side factors
        with pytest.raises(E, match="error -1: no factors on the other side"):
            c.wals_explain(1, [0], [0, 1], [0], ALPHA, LAM, 5)
        # nfactors > 256: refused, but no such context can be made to ask
        with pytest.raises(E, match="nfactors > 256"):
            qmf_amd.Context(257, 64)
        # nothing was launched by any of them; no queries and no pairs touch nothing
        assert c.solve_stats()["launches"] == launches
        out = c.wals_explain(0, [], [0], [], ALPHA, LAM, 5)
        assert out[0].shape == (0, 5) and out[5] is None
        out = c.wals_explain(0, [2, 3], [0, 0, 0], [], ALPHA, LAM, 5, full=True)
        assert out[4].shape == (0,) and out[5][0].shape == (0,)
        out = c.wals_explain_rows(0, [0], [], [], [0], [], ALPHA, LAM, 5)
        assert out[0].shape == (0, 5)
        assert c.solve_stats()["launches"] == launches
        # the context still works after the refused calls
        out = c.wals_explain(0, rows, qptr, targets, ALPHA, LAM, 5, full=True)
        assert c.solve_stats()["launches"] == launches + 1
        check_selection("after-errors", out, rowptr, col, rows, qptr, 5)


@pytest.mark.parametrize("precision", [64, 32])
def test_a_system_that_is_not_positive_definite(precision):
    """Rows of the signed ladder whose system numpy's Cholesky rejects: -5, naming the first
    such query; a following valid call succeeds."""
    k = 16
    (urp, ucol, uval), _, Y = signed_ladder_case(k, 3, precision, "strong")
    G = Y.T @ Y
    bad, good = [], []
    for r in range(len(urp) - 1):
        sl = slice(int(urp[r]), int(urp[r + 1]))
        Yr = Y[ucol[sl]]
        A = G + (Yr.T * (ALPHA * uval[sl])) @ Yr + LAM * np.eye(k)
        ev = np.linalg.eigvalsh(A)
        try:
            np.linalg.cholesky(A)
            if ev[0] > 1e-3:
                good.append(r)
        except np.linalg.LinAlgError:
            if ev[0] < -1e-3:  # clearly indefinite: no rounding decides it
                bad.append(r)
    assert len(bad) >= 1 and len(good) >= 2, (len(bad), len(good))
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(len(urp) - 1, len(Y))
        c.upload_csr(0, urp, ucol, uval)
        c.set_factors(1, Y)
        rows = [good[0], good[1], bad[0], good[0], bad[-1]]
        qptr = [0, 2, 2, 5, 6, 7]
        with pytest.raises(E, match="error -5: the row system of query 2 is not positive definite"):
            c.wals_explain(0, rows, qptr, np.arange(7), ALPHA, LAM, 3)
        with pytest.raises(E, match="error -5: the row system of query 0 is not positive definite"):
            c.wals_explain(0, rows[:2], [0, 1, 2], [5, 6], ALPHA, -1e3, 3)   # λ ≤ 0
        out = c.wals_explain(0, rows[:2], [0, 2, 3], [1, 2, 3], ALPHA, LAM, 3, full=True)
        assert np.all(np.isfinite(out[4])) and np.all(out[3] == np.minimum(
            3, np.diff(urp)[[good[0], good[0], good[1]]]))
