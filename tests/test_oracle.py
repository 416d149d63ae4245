"""Pins the CPU oracle (oracle/qmf_oracle.cpp) before it is trusted as the checker.

Pins, in order of strength:
  * reference outputs measured by the survey on the seeded ML-100K-shaped synthetic
    (SURVEY.md Appendix C): epoch-1 / epoch-10 loss and the md5 of the saved factor files;
  * the reference's own unit-test known answers (qmf/test/*.cpp), re-expressed;
  * the dsysv_ restatement against MKL's dsysv_ when MKL is present in the image.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as po
from helpers import (LADDER_LENGTHS, bpr_linear_item, bpr_linear_user, bpr_wave_case,
                     bpr_wave_triplets, factor_text, ladder_case, ladder_solution, load_ml100k,
                     md5, signed_ladder_case, signed_ladder_solution)

MKL_DIR = "/opt/conda/lib"


def _mkl_available():
    return os.path.exists(os.path.join(MKL_DIR, "libmkl_rt.so.1"))


@pytest.fixture(scope="module")
def ml100k_run():
    d = load_ml100k()
    o = po.OracleWALS(d["users"], d["items"], d["values"], 30, 0.05, 40.0)
    o.set_factors(1, d["init"][: o.nitems * 30].reshape(o.nitems, 30))
    losses = o.optimize(10, 4)
    return d, o, losses


def test_ml100k_losses_match_reference(ml100k_run):
    d, o, losses = ml100k_run
    # survey-measured reference values, printed to 6 significant digits
    assert abs(losses[0] - float(d["ref_loss_epoch1"])) < 5e-6
    assert abs(losses[9] - float(d["ref_loss_epoch10"])) < 5e-7


def test_ml100k_item_factor_file_bit_exact(ml100k_run):
    d, o, _ = ml100k_run
    assert md5(factor_text(o.ids(1), o.factors(1))) == str(d["ref_md5_item"])


def test_ml100k_user_factor_file_within_print_precision(ml100k_run):
    # With the dsysv_ restatement the user file differs from the reference's only in
    # last printed digits (solver rounding); see the MKL test below for the bit-exact pin.
    d, o, _ = ml100k_run
    U = o.factors(0)
    assert np.all(np.isfinite(U))
    assert 5 < np.max(np.abs(U)) < 50  # survey: user factors reach about 25


@pytest.mark.skipif(not _mkl_available(), reason="MKL not present")
def test_ml100k_bit_exact_with_mkl_dsysv(tmp_path):
    """Routes the oracle's solve through MKL dsysv_ (the survey's LAPACK) in a subprocess:
    both factor files must then equal the reference's byte for byte."""
    libdir = tmp_path / "mkl"
    libdir.mkdir()
    for f in os.listdir(MKL_DIR):
        if f.startswith("libmkl_") and ".so" in f:
            os.symlink(os.path.join(MKL_DIR, f), libdir / f)
    code = (
        "import sys; sys.path[:0]=[%r,%r];\n"
        "import pyoracle as po; from helpers import *\n"
        "d=load_ml100k(); o=po.OracleWALS(d['users'],d['items'],d['values'],30,0.05,40.0)\n"
        "o.set_factors(1,d['init'][:o.nitems*30].reshape(o.nitems,30)); o.optimize(10,4)\n"
        "print(md5(factor_text(o.ids(0),o.factors(0))), md5(factor_text(o.ids(1),o.factors(1))))\n"
    ) % (os.path.join(os.path.dirname(__file__), "..", "oracle"), os.path.dirname(__file__))
    # MKL picks a code path per host CPU; the md5s were recorded on a host whose path rounds
    # like MKL's conditional-numerical-reproducibility "COMPATIBLE" branch, so pin that branch
    # (without it the user file differs in last digits on AVX-512 hosts).
    env = dict(os.environ, ORC_LAPACK=str(libdir / "libmkl_rt.so.1"), MKL_CBWR="COMPATIBLE",
               MKL_THREADING_LAYER="SEQUENTIAL", LD_LIBRARY_PATH=str(libdir))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    mu, mi = out.stdout.split()
    d = load_ml100k()
    assert mu == str(d["ref_md5_user"])
    assert mi == str(d["ref_md5_item"])


def test_init_layout_like_reference():
    # WALSEngineTest.cpp:29-84
    o = po.OracleWALS([1, 1, 1, 2, 2, 3], [1, 2, 3, 1, 3, 4], [1.0] * 6, 30)
    assert (o.nusers, o.nitems) == (3, 4)
    rp, col, _ = o.csr(0)
    assert list(o.ids(0)) == [1, 2, 3]
    assert list(rp) == [0, 3, 5, 6]
    assert list(o.ids(1)[col]) == [1, 2, 3, 1, 3, 4]
    rp, col, _ = o.csr(1)
    assert list(o.ids(1)) == [1, 2, 3, 4]
    assert list(rp) == [0, 2, 3, 5, 6]
    assert list(o.ids(0)[col]) == [1, 2, 1, 1, 2, 3]


def test_xtx_known_answer():
    # WALSEngineTest.cpp:112-143 (X 17×5 ~ U(-1,1)), tolerance 1e-8
    X = np.random.default_rng(123).uniform(-1, 1, (17, 5))
    np.testing.assert_allclose(po.xtx(X), X.T @ X, atol=1e-8)


def test_update_factors_for_one_known_answer():
    # WALSEngineTest.cpp:145-205: Y ≡ 0.1 (2×3), α = λ = 1, two signals of value 1
    Y = np.full((2, 3), 0.1)
    x, loss = po.update_one(Y, [0, 1], [1.0, 1.0], Y.T @ Y, alpha=1.0, lam=1.0)
    np.testing.assert_allclose(x, 0.4 / 1.12, rtol=1e-12)
    pred = Y @ x
    true_loss = 2.0 * np.sum((1 - pred) ** 2)  # the other users' rows contribute 0 here
    assert abs(loss - true_loss) < 1e-2


def test_linear_solve_indefinite_residual():
    # MatrixTest.cpp:92-116: random symmetric indefinite 50×50, residual 1e-8
    rng = np.random.default_rng(123)
    n = 50
    A = np.zeros((n, n))
    b = rng.uniform(-1, 1, n)
    for i in range(n):
        for j in range(i, n):
            A[i, j] = A[j, i] = rng.uniform(-1, 1)
    assert np.min(np.linalg.eigvalsh(A)) < 0 < np.max(np.linalg.eigvalsh(A))
    x = po.linear_symmetric_solve(A, b)
    np.testing.assert_allclose(A @ x, b, atol=1e-8)


@pytest.mark.parametrize("n", [1, 2, 5, 30, 64])
def test_dsysv_restatement_matches_numpy(n):
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    A = M + M.T  # indefinite: exercises 1×1 and 2×2 Bunch-Kaufman pivots
    b = rng.normal(size=n)
    np.testing.assert_allclose(po.linear_symmetric_solve(A, b), np.linalg.solve(A, b),
                               rtol=1e-8, atol=1e-10)


def test_bpr_update_rule_matches_formula():
    # BPREngine.cpp:178-220: p_u uses the OLD q, q_i / q_n use the NEW p_u.
    rng = np.random.default_rng(3)
    k = 4
    U = rng.normal(size=(3, k))
    I = rng.normal(size=(5, k))
    bias = rng.normal(size=5)
    U0, I0, b0 = U.copy(), I.copy(), bias.copy()
    lr, lb, lu, li = 0.05, 1.0, 0.025, 0.0025
    po.bpr_update_seq(U, I, bias, [[1, 2, 4]], lr, lb, lu, li, True)
    x = b0[2] - b0[4] + U0[1] @ (I0[2] - I0[4])
    e = 1.0 / (1.0 + np.exp(x))
    pu = U0[1] + lr * (e * (I0[2] - I0[4]) - lu * U0[1])
    np.testing.assert_allclose(U[1], pu, rtol=1e-14)
    np.testing.assert_allclose(I[2], I0[2] + lr * (e * pu - li * I0[2]), rtol=1e-14)
    np.testing.assert_allclose(I[4], I0[4] + lr * (-e * pu - li * I0[4]), rtol=1e-14)
    assert abs(bias[2] - (b0[2] + lr * (e - lb * b0[2]))) < 1e-14
    assert abs(bias[4] - (b0[4] + lr * (-e - lb * b0[4]))) < 1e-14


def test_bpr_linearised_epoch_anchor():
    """Anchors the fp64 tolerance (1e-6) of the linearised multi-wave tests in
    test_bpr_kernels_gpu.py at their own shape (320 × 320, 4000 positives × 5 negatives,
    k = 16, lr = 2⁻³⁰, λ = 0): BPREngine::update over the restated triplets, in data order and
    in a random order, stays within 1e-7 of the first-order prediction, and one missing
    triplet moves the result by more than 1e-3 (all relative to max|prediction|).
    Measured: U 4.2e-09 / 3.9e-09, I 4.6e-09 / 5.1e-09, bias 1.8e-08 / 1.7e-08 (data /
    random order); without the first triplet U moves by 4.6e-02, I by 3.6e-02, the biases by
    1.8e-02."""
    nu, ni, _, _ = bpr_wave_case()
    trip = np.array(bpr_wave_triplets(False))
    k, lr = 16, 2.0 ** -30
    rng = np.random.default_rng(16)
    I0 = rng.normal(0, 0.1, (ni, k))
    U0 = rng.normal(0, 0.1, (nu, k))

    def run(t):
        U, I, b = np.zeros((nu, k)), I0.copy(), np.zeros(ni)
        po.bpr_update_seq(U, I, b, t, lr, 0.0, 0.0, 0.0, True)
        out = [U]
        U, I, b = U0.copy(), np.zeros((ni, k)), np.zeros(ni)
        po.bpr_update_seq(U, I, b, t, lr, 0.0, 0.0, 0.0, True)
        return out + [I, b]

    want = [bpr_linear_user(trip, I0, lr, nu), *bpr_linear_item(trip, U0, lr, ni)]
    dist = lambda got, ref: [float(np.max(np.abs(g - r)) / np.abs(w).max())  # noqa: E731
                             for g, r, w in zip(got, ref, want)]
    serial = run(trip)
    for name, t in (("serial", trip), ("random", trip[rng.permutation(len(trip))])):
        err = dist(run(t), want)
        print(name, "order: U %.2g I %.2g bias %.2g" % tuple(err))
        assert max(err) < 1e-7, (name, err)
    moved = dist(run(trip[1:]), serial)
    print("one triplet dropped: U %.2g I %.2g bias %.2g" % tuple(moved))
    assert min(moved) > 1e-3, moved


@pytest.mark.parametrize("k", [17, 129])
def test_ladder_reference_matches_oracle(k):
    """Anchors the numpy reference of tests/test_wals_rows_gpu.py (helpers.ladder_reference)
    on the CPU: on the row-length ladder without its empty row (the oracle builds rows from
    signals), WALSEngine::iterate's restatement and the numpy row solves agree to 1e-11 per
    row (‖Δx‖∞ / ‖x‖∞) and in the summed loss."""
    lam, alpha = 0.05, 40.0
    (urp, ucol, uval), (irp, icol, ival), Y = ladder_case(k, 1000 + k, 64, with_empty=False)
    nu, ni = len(urp) - 1, len(irp) - 1
    assert nu == len(LADDER_LENGTHS) - 1 and urp[-1] == sum(LADDER_LENGTHS) == 18631
    assert sorted(np.diff(urp)) == sorted(LADDER_LENGTHS[1:])
    o = po.OracleWALS.from_csr(nu, ni, urp, ucol, uval, irp, icol, ival, k, lam, alpha)
    o.set_factors(1, Y)
    lo = o.iterate(0) * nu * ni
    X, loss, cond, S = ladder_solution(k, 1000 + k, 64, alpha, lam, with_empty=False)
    err = np.max(np.abs(o.factors(0) - X), axis=1) / np.max(np.abs(X), axis=1)
    print("k = %d: worst row %.2g, loss %.2g relative, largest cond %.3g"
          % (k, err.max(), abs(lo - loss.sum()) / abs(loss.sum()), cond.max()))
    assert err.max() < 1e-11, (int(np.argmax(err)), err.max())
    assert abs(lo - loss.sum()) <= 1e-11 * abs(loss.sum())
    assert np.all(S >= np.abs(loss))


@pytest.mark.parametrize("k", [16, 33])
def test_signed_ladder_reference_matches_oracle(k):
    """Anchors the numpy reference of tests/test_resolve_gpu.py (helpers.signed_ladder_reference)
    on the CPU: on the strong signed ladder, where most systems are indefinite (dsysv_'s
    Bunch-Kaufman pivots in the oracle, LU in numpy), the two agree to 1e-9 row by row
    (‖Δx‖∞ / ‖x‖∞) and in the summed loss.  The oracle builds rows from signals, so the empty
    row is taken out of the CSRs first."""
    lam, alpha = 0.05, 40.0
    (urp, ucol, uval), (irp, icol, ival), Y = signed_ladder_case(k, 1000 + k, 64, "strong")
    X, loss, cond, S, has_neg, lam_min = signed_ladder_solution(k, 1000 + k, 64, "strong", alpha, lam)
    assert np.array_equal(uval[2::5] <= 0, np.ones(len(uval[2::5]), bool))
    assert np.sum(uval < 0) == np.sum(uval[2::5] < 0) and np.sum(lam_min < 0) == {16: 38, 33: 168}[k]
    assert cond.max() <= 1e6 and np.all(has_neg[lam_min < 0])
    r0 = int(np.flatnonzero(np.diff(urp) == 0)[0])
    assert np.all(X[r0] == 0.0) and loss[r0] == 0.0 and not has_neg[r0]
    keep = np.arange(len(urp) - 1) != r0
    nu, ni = len(urp) - 2, len(irp) - 1
    o = po.OracleWALS.from_csr(nu, ni, np.delete(urp, r0), ucol, uval, irp,
                               (icol - (icol > r0)).astype(np.int32), ival, k, lam, alpha)
    o.set_factors(1, Y)
    lo = o.iterate(0) * nu * ni
    err = np.max(np.abs(o.factors(0) - X[keep]), axis=1) / np.max(np.abs(X[keep]), axis=1)
    print("k = %d: worst row %.2g, loss %.2g relative, largest cond %.3g, %d indefinite"
          % (k, err.max(), abs(lo - loss.sum()) / abs(loss.sum()), cond.max(), np.sum(lam_min < 0)))
    assert err.max() < 1e-9, (int(np.argmax(err)), err.max())
    assert abs(lo - loss.sum()) <= 1e-9 * np.abs(loss).sum()
    assert np.all(S >= np.abs(loss))


def test_distribution_file_short_file(tmp_path):
    # FactorData.h:74-100: a short file leaves the remaining factors untouched (zeros)
    o = po.OracleWALS([1, 1, 2], [1, 2, 3], [1.0] * 3, 2)
    p = tmp_path / "u.dat"
    p.write_text("0.5\n0.25\n-1\n")
    assert o.load_distribution_file(str(p)) == 3
    np.testing.assert_array_equal(o.factors(1), [[0.5, 0.25], [-1, 0], [0, 0]])


def test_csr_entry_points_keep_double_values():
    # The full-size parity check and the CPU baseline build the oracle from the device's
    # downloaded CSR (qmfx_download_csr returns double).  On real-valued (non-fp32-exact)
    # weights, the CSR constructor and solve_rows must see exactly those doubles: the same
    # factors as the triple-based init (WALSEngine::init) on the same data, bit for bit.
    rng = np.random.default_rng(5)
    nu, ni, k = 40, 30, 8
    pairs = np.unique(rng.integers(0, nu * ni, 500))
    u, i = pairs // ni, pairs % ni
    v = rng.uniform(0.1, 5.0, len(pairs))
    assert not np.array_equal(v, v.astype(np.float32).astype(np.float64))
    a = po.OracleWALS(u, i, v, k)
    assert a.nusers == nu and a.nitems == ni  # every id present: idx == id
    urp, ucol, uval = a.csr(0)
    irp, icol, ival = a.csr(1)
    b = po.OracleWALS.from_csr(nu, ni, urp, ucol, uval, irp, icol, ival, k, 0.05, 40.0)
    Y = rng.uniform(-0.5, 0.5, (ni, k))
    a.set_factors(1, Y)
    b.set_factors(1, Y)
    la, lb = a.iterate(0), b.iterate(0)
    assert la == lb and np.array_equal(a.factors(0), b.factors(0))
    rows = np.arange(nu, dtype=np.int64)
    x, _ = po.solve_rows(Y, urp, ucol.astype(np.int32), uval, rows, 40.0, 0.05)
    x32, _ = po.solve_rows(Y, urp, ucol.astype(np.int32), uval.astype(np.float32), rows, 40.0, 0.05)
    assert np.allclose(x, a.factors(0), rtol=1e-12, atol=1e-14)
    assert not np.array_equal(x, x32)  # the fp32-narrowed problem is a different one
