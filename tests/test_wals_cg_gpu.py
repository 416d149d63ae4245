"""qmfx_wals_half_cg on the MI355X against the numpy restatement of its contract.

Tolerance (per case, wals_cg_ref.references): δ = the largest row-normalised difference between
the reference run in the context's dtype and in longdouble; the device passes within 16·δ of the
longdouble result (a 64-lane reduction tree and an MFMA-ordered G differ from numpy's summation
order).  test_wals_cg.py shows that the rule rejects wrong variants of the algorithm.  Loss terms
use the same rule relative to the magnitude of the sums behind them (cg_half's scale).
"""
import functools

import numpy as np
import pytest

import qmf_amd
import wals_cg_ref as ref
from wals_cg_ref import ALPHA, LAM, BLOCK, CASES

pytestmark = pytest.mark.gpu


def case_id(c):
    return "k%d-ny%d-n%d-s%d" % c


def context(data, k, precision):
    rowptr, col, val, Y, X0 = data
    c = qmf_amd.Context(k, precision)
    c.set_shape(len(rowptr) - 1, len(Y))
    c.upload_csr(0, rowptr, col, val)
    c.set_factors(1, Y)
    c.set_factors(0, X0)
    return c


@functools.lru_cache(maxsize=None)
def solved(case, precision):
    """One case: data, references with δ, and the device's result (shared, never modified)."""
    k, ny, nrows, steps = case
    data = ref.make_case(k, ny, nrows, precision)
    ld, dt, dx, dl = ref.references(data, precision, steps)
    with context(data, k, precision) as c:
        total = c.wals_half_cg(0, ALPHA, LAM, steps)
        out = dict(data=data, ld=ld, dx=dx, dl=dl, total=total, X=c.factors(0),
                   loss=c.row_losses(0), failed=c.failed_rows(), Y=c.factors(1),
                   csr=c.download_csr(0))
    return out


def check(X, loss, total, ld, dx, dl, label):
    ex = ref.row_err(X, ld[0])
    el = ref.loss_err(loss, ld[1], ld[2])
    et = abs(total - float(ld[1].sum())) / float(ld[2].sum())
    print("%s: δx %.3e device %.3e (×%.2f) | δloss %.3e device %.3e sum %.3e"
          % (label, dx, ex, ex / dx if dx else 0, dl, el, et))
    assert ex <= 16 * dx
    assert el <= 16 * dl
    assert et <= 16 * dl


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_matches_reference(case, precision):
    s = solved(case, precision)
    check(s["X"], s["loss"], s["total"], s["ld"], s["dx"], s["dl"],
          "%s fp%d" % (case_id(case), precision))
    assert len(s["failed"]) == 0
    rowptr = s["data"][0]
    empty = np.diff(rowptr) == 0
    assert np.all(s["X"][empty] == 0) and np.all(s["loss"][empty] == 0)
    assert np.all(np.isfinite(s["X"]))


@pytest.mark.parametrize("precision", [64, 32])
def test_row_at_its_solution_stays_put(precision):
    """Row 3 of every case starts at its solution (rounded to the context precision)."""
    case = (64, 17, 2 * BLOCK + 3, 2)
    s = solved(case, precision)
    X0 = s["data"][4]
    eps = 2.0 ** (-24 if precision == 32 else -53)
    # the start solves the system up to its own rounding; CG moves it by no more than that
    # times the condition number (≲ 10³)
    moved = np.abs(s["X"][3] - X0[3]).max() / np.abs(X0[3]).max()
    print("fp%d: row at its solution moved by %.2e" % (precision, moved))
    assert moved <= 1e3 * eps * 64


@pytest.mark.parametrize("precision", [64, 32])
def test_fixed_side_and_csr_untouched(precision):
    s = solved((64, 17, 2 * BLOCK + 3, 2), precision)
    rowptr, col, val, Y, _ = s["data"]
    assert np.array_equal(s["Y"], Y)
    rp, cl, vl = s["csr"]
    assert np.array_equal(rp, rowptr) and np.array_equal(cl, col) and np.array_equal(vl, val)


@pytest.mark.parametrize("precision", [64, 32])
def test_same_state_same_bits(precision):
    k, ny, nrows, steps = 100, 17, 2 * BLOCK + 3, 3
    data = ref.make_case(k, ny, nrows, precision)
    outs = []
    with context(data, k, precision) as c:
        for _ in range(2):
            c.set_factors(0, data[4])
            total = c.wals_half_cg(0, ALPHA, LAM, steps)
            outs.append((total, c.factors(0), c.row_losses(0)))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("precision", [64, 32])
def test_exact_half_after_cg_is_unchanged(precision):
    """The exact half after a CG half gives the bits it gives without it."""
    k, ny, nrows = 64, 17, 2 * BLOCK + 3
    data = ref.make_case(k, ny, nrows, precision)
    with context(data, k, precision) as c:
        want = (c.wals_half(0, ALPHA, LAM), c.factors(0), c.row_losses(0))
    with context(data, k, precision) as c:
        c.wals_half_cg(0, ALPHA, LAM, 2)
        got = (c.wals_half(0, ALPHA, LAM), c.factors(0), c.row_losses(0))
        assert np.array_equal(c.factors(1), data[3])
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("precision", [64, 32])
def test_indefinite_row_is_flagged(precision):
    """Row 5 gets one signal with 1 + αv < 0, strong enough that p·A·p < 0 along it: b is
    dominated by c·y with c ≈ −1250, x₀ = 0, so p₀ = b ∥ y and d = c²·(yᵀGy + w‖y‖⁴ + λ‖y‖²)
    with w‖y‖² ≈ −1250 against yᵀGy/‖y‖² + λ of order 1."""
    k, ny, nrows, steps = 64, 17, 2 * BLOCK + 3, 3
    rowptr, col, val, Y, X0 = ref.make_case(k, ny, nrows, precision)
    val = val.copy()
    X0 = X0.copy()
    bad = 5
    assert rowptr[bad + 1] - rowptr[bad] == 64
    val[rowptr[bad]] = -1000.0
    X0[bad] = 0
    data = (rowptr, col, val, Y, X0)
    ld, _, dx, dl = ref.references(data, precision, steps)
    assert list(np.flatnonzero(ld[3])) == [bad]
    with context(data, k, precision) as c:
        c.wals_half_cg(0, ALPHA, LAM, steps)
        X, loss, failed = c.factors(0), c.row_losses(0), c.failed_rows()
    assert list(failed) == [bad]
    assert np.all(np.isfinite(X[bad])) and np.isfinite(loss[bad])
    assert np.array_equal(X[bad], X0[bad])  # stopped before the first update
    keep = np.arange(nrows) != bad
    ex = ref.row_err(X[keep], ld[0][keep])
    el = ref.loss_err(loss[keep], ld[1][keep], ld[2][keep])
    print("fp%d other rows: δx %.3e device %.3e, δloss %.3e device %.3e" % (precision, dx, ex, dl, el))
    assert ex <= 16 * dx and el <= 16 * dl


@pytest.mark.parametrize("precision", [64, 32])
def test_heavy_rows_are_solved_exactly(precision, monkeypatch):
    """With QMFX_HEAVY_MIN lowered, the 129-signal rows are split-K heavy rows: they get the
    exact half's bits, the other rows the CG result."""
    monkeypatch.setenv("QMFX_HEAVY_MIN", "100")
    monkeypatch.setenv("QMFX_SEG_LEN", "50")
    k, ny, nrows, steps = 64, 17, 2 * BLOCK + 3, 2
    data = ref.make_case(k, ny, nrows, precision)
    rowptr = data[0]
    heavy = np.diff(rowptr) > 100
    assert heavy.sum() == 5
    ld, _, dx, dl = ref.references(data, precision, steps)
    with context(data, k, precision) as c:
        assert c.row_classes(0)["heavy"] == 5
        c.wals_half(0, ALPHA, LAM)
        exact, exact_loss = c.factors(0), c.row_losses(0)
    with context(data, k, precision) as c:
        c.wals_half_cg(0, ALPHA, LAM, steps)
        X, loss = c.factors(0), c.row_losses(0)
        assert len(c.failed_rows()) == 0
    assert np.array_equal(X[heavy], exact[heavy])
    assert np.array_equal(loss[heavy], exact_loss[heavy])
    ex = ref.row_err(X[~heavy], ld[0][~heavy])
    el = ref.loss_err(loss[~heavy], ld[1][~heavy], ld[2][~heavy])
    print("fp%d non-heavy rows: δx %.3e device %.3e, δloss %.3e device %.3e" % (precision, dx, ex, dl, el))
    assert ex <= 16 * dx and el <= 16 * dl


def test_side_never_set_starts_from_zero():
    k, ny, nrows, steps = 16, 17, BLOCK + 1, 2
    rowptr, col, val, Y, X0 = ref.make_case(k, ny, nrows, 64)
    data = (rowptr, col, val, Y, np.zeros_like(X0))
    ld, _, dx, dl = ref.references(data, 64, steps)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nrows, ny)
        c.upload_csr(0, rowptr, col, val)
        c.set_factors(1, Y)
        total = c.wals_half_cg(0, ALPHA, LAM, steps)
        check(c.factors(0), c.row_losses(0), total, ld, dx, dl, "x₀ = 0")


def test_rejections_launch_nothing():
    k, ny, nrows = 16, 17, BLOCK + 1
    data = ref.make_case(k, ny, nrows, 64)
    with context(data, k, 64) as c:
        for args, msg in [((2, ALPHA, LAM, 2), "side must be 0 or 1"),
                          ((-1, ALPHA, LAM, 2), "side must be 0 or 1"),
                          ((0, ALPHA, LAM, 0), "steps must be at least 1"),
                          ((1, ALPHA, LAM, 2), "no interactions uploaded")]:
            with pytest.raises(qmf_amd.QmfxError, match=msg):
                c.wals_half_cg(*args)
        assert np.array_equal(c.factors(0), data[4])  # nothing ran
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(nrows, ny)
        c.upload_csr(0, *data[:3])
        with pytest.raises(qmf_amd.QmfxError, match="fixed side has no factors"):
            c.wals_half_cg(0, ALPHA, LAM, 2)
    # more than 256 factors: no context of that size exists to call it on
    with pytest.raises(qmf_amd.QmfxError, match="256"):
        qmf_amd.Context(257, 64)


def test_sharded_context_is_rejected():
    k, ny, nrows = 16, 17, BLOCK + 1
    data = ref.make_case(k, ny, nrows, 64)
    with context(data, k, 64) as c:
        qmf_amd.dist_init_all([c])
        with pytest.raises(qmf_amd.QmfxError, match="one device"):
            c.wals_half_cg(0, ALPHA, LAM, 2)


def test_time_goes_into_the_solve_stats():
    case = (64, 17, 2 * BLOCK + 3, 2)
    k, ny, nrows, steps = case
    data = ref.make_case(k, ny, nrows, 64)
    with context(data, k, 64) as c:
        c.reset_stats()
        c.wals_half_cg(0, ALPHA, LAM, steps)
        st = c.solve_stats()
    n = np.diff(data[0])
    rows = len(n)
    want = (steps + 1) * (2 * k * k * rows + 4 * k * n.sum())
    print("solve stats:", st)
    assert st["launches"] == 1 and st["ms"] > 0
    assert st["flops"] == want
