"""The pivoted re-solve on the MI355X, row by row against numpy: which rows the Cholesky kernels
flag, and what wals_fallback_kernel (qmf_amd/csrc/fallback.hip) then writes for them — x, the
row loss, the status word and the two counters behind error −6 — on every route.

The fixture is helpers.signed_ladder_case: the 181-row ladder of tests/test_wals_rows_gpu.py
with every fifth signal made negative.  "strong" negates it (v ∈ (−5, 0]): at k ≥ 16 most
systems are indefinite, at k ≤ 8 they all stay SPD with a negative weight.  "mild" sets it to
−0.01·|v|: every system stays SPD and as well conditioned as the unsigned ladder's, so a row is
flagged there only by a kernel that cannot take a negative weight (the whitened form, the
fp32 split Gram).  The reference is helpers.signed_ladder_reference (numpy fp64, anchored on
the CPU oracle by tests/test_oracle.py::test_signed_ladder_reference_matches_oracle).  Every
bound below comes from numpy's cond₂ (max|eigenvalue| / min|eigenvalue|) of the reference
system, never from the device's output.

Per case (one wals_half(0, 40, 0.05) in a fresh context), every row on its own:
  factors  ‖x_dev − x_ref‖∞ / ‖x_ref‖∞ ≤
             fp64: min(1e-7, max(1e-9, C·k·cond_r·2⁻⁵³)) — 1e-9 the SPD bar, 1e-7 the project's
                   bar for the re-solve, C = C_FP64 below; cond_r ≤ 1e6 is asserted;
             fp32: min(2e-3, max(1e-4, k·cond_r·2⁻²⁴)); on the strong recipe rows with
                   k·cond_r·2⁻²⁴ > 2e-3 are left out (no fp32 solve of them means anything),
                   counted, printed and asserted to be at most 25 % of the case;
  loss     |loss_dev − loss_ref| ≤ tol·S_r, tol 1e-9 / 1e-4, times max(1, cond_r / 1e3) on the
           strong recipe (x's error enters through xᵀb); S_r = Σ|c| + |xᵀ(A − λI)x| + 2|xᵀb|
           (Σ|c|, not Σc: with negative c the sum itself cancels); the returned sum equals
           Σ row_losses to 1e-12·Σ|loss_r|;
  flags    F = failed_rows(): every row with λmin(A) < −1e-6 is in F; every row in F has a
           negative weight; every row with a negative weight in a whitened bucket is in F; so
           is every such row — split-K or whole — whose Gram is the split (√w) form, NEGW
           below; the empty row is not in F and its x and loss are exactly 0.

Which routes flag a negative weight as such (the others only on a non-positive pivot):
  whitened rows, all three kernels ....... woodbury.hip:57, :316, :630 (`wl < 0` ballot)
  fp32 one-wave direct, nt = 6, 7, 8 ...... direct.h:32 (Perm::split), :140 (negw), :564
  fp32 multi-wave, nt = 16 ................ big.h:29 (BigCfg::SPLIT), wals_big.hip:665, :712
  their split-K segments carry the flag through partc: direct.h:577 → :496,
  wals_big.hip:847 → :855, max-reduced over a row's segments in wals_heavy.hip:52 / :106.
  No fp64 tiling and no other fp32 tiling (nt ≤ 5, 9..15) has a split Gram: the split-K cases
  the ladder module runs (k = 64, 200) have none, hence the k = 128 / 256 fp32 cases here.

Measured on an MI355X: 71 cases in 20 s, the slowest 1.5 s (k = 256); all pass on the
unmodified library (no kernel bug found).

C_FP64: the largest err / (k·cond_r·2⁻⁵³) over every row of every fp64 case with k ≥ 16 is
0.42 (0.31 in test_many_flagged_rows) → next power of two 0.5, times 4: C = 2.  At k = 1 and
k = 3 the figure is 9.9e3 and 4.4 with err = 1.1e-12 and less: investigated, and it is not the
solve.  There cond₂ ≤ 3 while b = Σ c·y cancels between positive and negative c — Σ|c||y| / |b|
reaches 3.7e4 on a k = 1 row of 163 signals, so rounding b alone moves x by up to 4e-12 in
numpy as on the device.  Those rows sit at the 1e-9 floor whatever C is.

Largest per-row errors over all cases, beside the bound of that row:
  precision recipe route       factors (bound)          loss / scale (tol)
  fp64      strong whitened    2.1e-13 (1e-9)           3.4e-14 (1e-9)
  fp64      strong direct      1.5e-12 (1e-9)           1.9e-13 (1e-9)
  fp64      strong multi-wave  3.6e-12 (1e-9)           9.9e-14 (1e-9)
  fp64      strong split-K     4.1e-13 (1e-9)           1.1e-13 (1e-9)
  fp64      mild   whitened    1.2e-14 (1e-9)           2.4e-16 (1e-9)
  fp64      mild   direct      5.2e-15 (1e-9)           4.4e-16 (1e-9)
  fp64      mild   multi-wave  1.3e-14 (1e-9)           1.5e-16 (1e-9)
  fp64      many rows (k = 16) 1.1e-14 (1e-9)           8.0e-16 (1e-9)
  fp32      strong whitened    3.7e-7  (1e-4)           7.0e-7  (1e-4)
  fp32      strong direct      7.1e-6  (1.2e-4)         1.4e-5  (1e-4)
  fp32      strong split-K     4.4e-7  (6.5e-4)         7.0e-7  (1e-4)
  fp32      mild   direct      1.4e-6  (1e-4)           7.6e-8  (1e-4)
  fp32      mild   multi-wave  7.4e-8  (7.4e-4)         2.9e-10 (1e-4)
  fp32      mild   split-K     7.1e-8  (2.0e-4)         6.3e-10 (1e-4)
With C = 2 the fp64 bound leaves the 1e-9 floor only above k·cond_r = 4.5e6; the largest on
these cases is 3.0e7 (k = 192, cond₂ = 1.6e5: bound 6.7e-9), far below the 1e-7 cap.
Row systems: A 1.0e-15·max|A| (fp64), 5.4e-8·max|G| (fp32, bound 6.1e-5); b 3.0e-16, Σc 5.4e-16.

fp32 strong rows left out (k·cond_r·2⁻²⁴ > 2e-3), computed on the CPU before the list was
fixed: k = 8: 0, k = 32: 8 (4.4 %), k = 64: 17 (9.4 %); k = 128: 64 (35 %) and k = 200: 82
(45 %) exceed the cap and are not run in fp32 strong.

Single-line mutants of the library, each run once (new cases failing of 71; cases of
test_wals_gpu + test_heavy_gpu failing too, of 81):
  build_system's padding diagonal 0 instead of 1 ............... 12 new (every off-tile k with
      a flagged row: error −6), 2 old
  tail mask one short (`e < m − 1` in the staging of Y rows; the mask dropped outright reads
      past the CSR's end on the last row, so it is not run on a device) ... 61 new, 7 old
  b's swap left out when p ≠ j ................................... 38 new, 6 old
  argmax tie rule reversed (largest row index) ................... 0 new, 0 old — as it should:
      either pivot of an exact tie is a valid partial pivot
  share rounded down (⌊nslots / grid⌋; rounded up by one more it still covers every slot) ..
      2 new (both 4097-row cases: the last slot is never scanned), 0 old
  −λ‖x‖² left out of the re-solve's loss ......................... 51 new, 6 old
  `wl < 0` ballot of the register-resident whitened kernel (woodbury.hip:57) removed ........
      5 new (k = 17, 32, 33, 48 strong, k = 32 mild fp64), 1 old
  negw not stored to partc (wals_big.hip:847) .................... 1 new
      (test_mild_split_k_fp32_split_gram[256]), 0 old
"""
import time

import numpy as np
import pytest

import qmf_amd
from helpers import (LADDER_LENGTHS, csr_from_triples, ladder_case, ladder_reference,
                     ladder_solution, signed_ladder_case, signed_ladder_solution)

pytestmark = pytest.mark.gpu

ALPHA, LAM = 40.0, 0.05
NROWS = len(LADDER_LENGTHS)
C_FP64 = 2.0
# Largest whitened bucket per precision and factor tiling: WB_MAX of tests/test_wals_rows_gpu.py
# restated (ctx.h default_whitened_ntn).
WB_MAX = {32: {2: 1, 3: 1, 4: 4, 5: 2, 6: 3, 7: 3, 8: 8, 16: 8},
          64: {2: 1, 3: 1, 4: 3, 5: 2, 6: 3, 7: 3, 8: 5, 16: 5}}
# (precision, nt) whose direct / split-K Gram takes √w and so flags every negative weight:
# direct.h:32 `split = sizeof(T) == 4 && NT >= 6` (one-wave kernel, nt ≤ 8) and big.h:29
# `SPLIT = sizeof(T) == 4 && NT == 16` (multi-wave kernel, nt ≥ 9).
NEGW = {(32, 6), (32, 7), (32, 8), (32, 16)}
HEAVY = {"QMFX_HEAVY_MIN": "128", "QMFX_SEG_LEN": "64"}


def seed_of(k):
    return 1000 + k


def fp64_bound(k, cond):
    return np.minimum(1e-7, np.maximum(1e-9, C_FP64 * k * cond * 2.0 ** -53))


def run_signed(k, precision, recipe, monkeypatch, whiten=True, heavy=False, env=None):
    """One user half on the signed ladder with every check of the module's docstring.
    Returns (factors, row losses, flagged rows)."""
    if not whiten:
        monkeypatch.setenv("QMFX_NO_WHITEN", "1")
    for key, v in {**(HEAVY if heavy else {}), **(env or {})}.items():
        monkeypatch.setenv(key, v)
    t0 = time.perf_counter()
    (urp, ucol, uval), (irp, icol, ival), Y = signed_ladder_case(k, seed_of(k), precision, recipe)
    X, loss, cond, S, has_neg, lam_min = signed_ladder_solution(k, seed_of(k), precision, recipe,
                                                               ALPHA, LAM)
    t1 = time.perf_counter()
    n = np.diff(urp)
    assert sorted(n) == sorted(LADDER_LENGTHS) and len(n) == NROWS
    assert cond.max() <= 1e6, cond.max()
    nt = (k + 15) // 16
    with qmf_amd.Context(k, precision) as c:  # the QMFX_* settings are read at create
        c.set_shape(NROWS, len(irp) - 1)
        c.upload_csr(0, urp, ucol, uval)
        c.upload_csr(1, irp, icol, ival)
        c.set_factors(1, Y)
        rc = c.row_classes(0)
        total = c.wals_half(0, ALPHA, LAM)
        F, rl = c.factors(0), c.row_losses(0)
        failed = np.sort(c.failed_rows())
    flagged = np.zeros(NROWS, bool)
    flagged[failed] = True
    # ---- routes, from n alone
    mx = WB_MAX[precision].get(nt, 0) if whiten else 0
    bucket = (np.maximum(n, 1) + 15) // 16
    assert rc["whitened"] == [int(np.sum(bucket == j + 1)) if j < mx else 0 for j in range(8)], rc
    is_w = bucket <= mx
    is_h = (n > 128) & ~is_w if heavy else np.zeros(NROWS, bool)
    assert rc["heavy"] == int(is_h.sum()), rc
    route = np.where(is_w, "whitened", np.where(is_h, "split-K", "multi-wave" if nt > 8 else "direct"))
    # ---- flags
    r0 = int(np.flatnonzero(n == 0)[0])
    assert not flagged[r0] and np.all(F[r0] == 0.0) and rl[r0] == 0.0
    assert loss[r0] == 0.0 and np.all(X[r0] == 0.0) and not has_neg[r0]
    missed = np.flatnonzero((lam_min < -1e-6) & ~flagged)
    assert len(missed) == 0, [(int(r), int(n[r]), route[r], lam_min[r]) for r in missed[:8]]
    spurious = np.flatnonzero(flagged & ~has_neg)
    assert len(spurious) == 0, [(int(r), int(n[r]), route[r]) for r in spurious[:8]]
    must = has_neg & (is_w | ((precision, nt) in NEGW))
    missed = np.flatnonzero(must & ~flagged)
    assert len(missed) == 0, [(int(r), int(n[r]), route[r]) for r in missed[:8]]
    # ---- per row
    full = n > 0
    xerr = np.zeros(NROWS)
    xerr[full] = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    left_out = np.zeros(NROWS, bool)
    if precision == 64:
        xbound, ltol = fp64_bound(k, cond), 1e-9
        print("RESOLVE_C k=%d recipe=%s w=%d h=%d largest err/(k·cond·2^-53) = %.3g"
              % (k, recipe, whiten, heavy, (xerr / (k * cond * 2.0 ** -53)).max()))
    else:
        raw = k * cond * 2.0 ** -24
        xbound, ltol = np.minimum(2e-3, np.maximum(1e-4, raw)), 1e-4
        if recipe == "strong":
            left_out = raw > 2e-3
            print("RESOLVE_LEFT_OUT k=%d p=32 rows with k·cond·2^-24 > 2e-3: %d of %d"
                  % (k, left_out.sum(), NROWS))
            assert left_out.sum() <= 0.25 * NROWS, left_out.sum()
    lscale = S * (np.maximum(1.0, cond / 1e3) if recipe == "strong" else 1.0)
    lerr = np.abs(rl - loss) / np.where(lscale > 0, lscale, 1.0)  # in units of the row's scale
    for name in ("whitened", "direct", "multi-wave", "split-K"):
        m = (route == name) & full & ~left_out
        if m.any():
            print("RESOLVE k=%d p=%d %s w=%d h=%d route=%s rows=%d flagged=%d xerr=%.3g xbound=%.3g "
                  "lerr=%.3g ltol=%.3g" % (k, precision, recipe, whiten, heavy, name, m.sum(),
                                           (flagged & m).sum(), xerr[m].max(),
                                           xbound[m][np.argmax(xerr[m] / xbound[m])],
                                           lerr[m].max(), ltol))
    print("RESOLVE_TIME k=%d p=%d reference %.2f s (0 when shared), device and checks %.2f s"
          % (k, precision, t1 - t0, time.perf_counter() - t1))
    bad = np.flatnonzero((xerr > xbound) & ~left_out)
    assert len(bad) == 0, [(int(r), int(n[r]), route[r], bool(flagged[r]), xerr[r], xbound[r])
                           for r in bad[:8]]
    bad = np.flatnonzero((np.abs(rl - loss) > ltol * lscale) & ~left_out)
    assert len(bad) == 0, [(int(r), int(n[r]), route[r], bool(flagged[r]), rl[r], loss[r],
                            lscale[r]) for r in bad[:8]]
    assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum(), (total, rl.sum())
    return F, rl, failed


OFF_TILE = [1, 3, 17, 33, 65, 100, 129, 200, 255]


@pytest.mark.parametrize("k", [16 * nt for nt in range(1, 17)] + OFF_TILE)
def test_strong_fp64(k, monkeypatch):
    """Every factor tiling and off-tile k (the re-solve's unit padding diagonal and Y's zero
    tail, eliminated over all KP columns), whitened and direct rows side by side."""
    run_signed(k, 64, "strong", monkeypatch)


@pytest.mark.parametrize("k", [32, 65, 128, 255])
def test_strong_fp64_no_whiten(k, monkeypatch):
    """All 181 rows on the direct kernels: only a non-positive pivot flags a row."""
    run_signed(k, 64, "strong", monkeypatch, whiten=False)


@pytest.mark.parametrize("k,precision", [(64, 64), (200, 64), (64, 32)])
def test_strong_split_k(k, precision, monkeypatch):
    """Rows longer than 128 cut into 64-signal segments: the reduced image's pivots flag.
    (fp32 k = 200 is not run: 82 of its 181 rows have k·cond·2⁻²⁴ > 2e-3, above the 25 % cap.)"""
    run_signed(k, precision, "strong", monkeypatch, heavy=True)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k,whiten", [(k, True) for k in (16, 32, 64, 100, 128, 256)] +
                         [(64, False), (256, False)])
def test_mild(k, whiten, precision, monkeypatch):
    """Negative weights on SPD systems: the whitened kernels and the fp32 split Gram
    (k = 100, 128, 256) must flag them, and nothing else may be wrong about them."""
    run_signed(k, precision, "mild", monkeypatch, whiten=whiten)


@pytest.mark.parametrize("k", [128, 256])
def test_mild_split_k_fp32_split_gram(k, monkeypatch):
    """The two split-K tilings with a split Gram (NEGW): a segment's negative-weight flag
    reaches the row only through partc, and on SPD systems nothing else would flag the row."""
    _, _, failed = run_signed(k, 32, "mild", monkeypatch, heavy=True)
    n = np.diff(signed_ladder_case(k, seed_of(k), 32, "mild")[0][0])
    assert np.all(n[failed] > 0) and np.sum(n[failed] > 128) == 52  # every split-K row


@pytest.mark.parametrize("k", [8, 32])
def test_strong_fp32(k, monkeypatch):
    """fp32 contexts: k = 8 is the "negative weight, SPD" regime on the plain fp32 Cholesky;
    at k = 32 the flagged rows are re-solved in fp64 from the fp32 YᵀY.  (k = 128 is not run:
    64 of its 181 rows have k·cond·2⁻²⁴ > 2e-3, above the 25 % cap; the mild cases cover the
    fp32 tilings above k = 64.)"""
    run_signed(k, 32, "strong", monkeypatch)


def test_pieces_and_row_chunks_are_bit_identical(monkeypatch):
    """QMFX_PIECES=3 (slot_begin ≠ 0 in the re-solve's scan) and QMFX_ROW_CHUNK=37 (several
    launches per kernel): the same factors, losses and flagged set, bit for bit."""
    one = run_signed(64, 64, "strong", monkeypatch)
    cut = run_signed(64, 64, "strong", monkeypatch, env={"QMFX_PIECES": "3", "QMFX_ROW_CHUNK": "37"})
    assert len(one[2]) > 100
    for a, b in zip(one, cut):
        assert np.array_equal(a, b)


# ---- qmfx_wals_row_system: build_system's staging on its own
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [1, 17, 64, 129, 256])
def test_row_system_every_staging_edge(k, precision):
    """A, b and Σc of rows around the 16-signal staging (the `e < m` tail mask) and of long
    rows, against numpy.  The empty row's A is G + λI itself: YᵀY of the one-wave and the
    multi-wave Gram kernels at these k."""
    (urp, ucol, uval), (irp, icol, ival), Y = signed_ladder_case(k, seed_of(k), precision, "strong")
    n = np.diff(urp)
    G = Y.T @ Y
    gerr = 0.0 if precision == 64 else len(Y) * 2.0 ** -24 * np.abs(G).max()
    worst = [0.0, 0.0, 0.0]
    with qmf_amd.Context(k, precision) as c:
        c.set_shape(NROWS, len(irp) - 1)
        c.upload_csr(0, urp, ucol, uval)
        c.upload_csr(1, irp, icol, ival)
        c.set_factors(1, Y)
        for length in (0, 1, 15, 16, 17, 31, 32, 33, 170, 640):
            r = int(np.flatnonzero(n == length)[0])
            sl = slice(int(urp[r]), int(urp[r + 1]))
            Yr, w = Y[ucol[sl]], ALPHA * uval[sl]
            A = G + (Yr.T * w) @ Yr + LAM * np.eye(k)
            b = Yr.T @ (1.0 + w)
            bscale = np.max(np.abs(Yr).T @ np.abs(1.0 + w)) if length else 0.0
            Ad, bd, cs = c.row_system(0, r, ALPHA, LAM)
            ea, eb, ec = np.abs(Ad - A).max(), np.abs(bd - b).max(), abs(cs - np.sum(1.0 + w))
            assert ea <= gerr + 1e-12 * np.abs(A).max(), (length, ea)
            assert eb <= 1e-12 * bscale, (length, eb, bscale)
            assert ec <= 1e-12 * np.sum(np.abs(1.0 + w)), (length, ec)
            worst = [max(worst[0], ea / np.abs(A).max()), max(worst[1], eb / max(bscale, 1e-300)),
                     max(worst[2], ec / max(np.sum(np.abs(1.0 + w)), 1e-300))]
    print("ROW_SYSTEM k=%d p=%d A %.3g (bound %.3g) b %.3g Σc %.3g (1e-12)"
          % (k, precision, worst[0], gerr / np.abs(G).max() + 1e-12, worst[1], worst[2]))


# ---- more than one workgroup in the re-solve
MANY_K, MANY_ITEMS = 16, 300


def many_rows(nrows, negative):
    """`nrows` user rows of three signals over 300 items (columns r, r + 101, r + 202 mod 300),
    values uniform(0.5, 5) with the middle one −5 on the rows of `negative`; Y uniform(−½, ½),
    so that −200·y yᵀ outweighs YᵀY (eigenvalues near 25) and such a row is indefinite.
    Returns the CSRs, Y and the batched numpy solution (X, loss, cond₂, S, λmin)."""
    rng = np.random.default_rng(nrows)
    Y = rng.uniform(-0.5, 0.5, (MANY_ITEMS, MANY_K))
    r = np.arange(nrows)
    cols = np.sort(np.stack([(r + 101 * j) % MANY_ITEMS for j in range(3)], 1), axis=1)
    vals = rng.uniform(0.5, 5.0, (nrows, 3))
    vals[negative, 1] = -5.0
    _, _, ucsr, icsr = csr_from_triples(np.repeat(r, 3), cols.ravel(), vals.ravel())
    assert np.array_equal(ucsr[1].reshape(nrows, 3), cols) and len(icsr[0]) == MANY_ITEMS + 1
    Yr, w = Y[cols], ALPHA * vals
    M = Y.T @ Y + np.einsum("rj,rji,rjl->ril", w, Yr, Yr)
    A = M + LAM * np.eye(MANY_K)
    b = np.einsum("rj,rji->ri", 1.0 + w, Yr)
    X = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    quad, xb = np.einsum("ri,ril,rl->r", X, M, X), np.einsum("ri,ri->r", X, b)
    ev = np.linalg.eigvalsh(A)
    cond = np.abs(ev).max(axis=1) / np.abs(ev).min(axis=1)
    loss = np.sum(1.0 + w, axis=1) + quad - 2.0 * xb
    S = np.sum(np.abs(1.0 + w), axis=1) + np.abs(quad) + 2.0 * np.abs(xb)
    return ucsr, icsr, Y, (X, loss, cond, S, ev[:, 0])


def check_many(nrows, negative):
    ucsr, icsr, Y, (X, loss, cond, S, lam_min) = many_rows(nrows, negative)
    assert cond.max() <= 1e6, cond.max()
    with qmf_amd.Context(MANY_K, 64) as c:
        c.set_shape(nrows, MANY_ITEMS)
        c.upload_csr(0, *ucsr)
        c.upload_csr(1, *icsr)
        c.set_factors(1, Y)
        total = c.wals_half(0, ALPHA, LAM)
        F, rl, failed = c.factors(0), c.row_losses(0), c.failed_rows()
    xerr = np.max(np.abs(F - X), axis=1) / np.max(np.abs(X), axis=1)
    xbound = fp64_bound(MANY_K, cond)
    lscale = S * np.maximum(1.0, cond / 1e3)
    print("MANY nrows=%d flagged=%d indefinite=%d xerr=%.3g (largest bound %.3g, err/(k·cond·2^-53) "
          "%.3g) lerr=%.3g" % (nrows, len(failed), (lam_min < 0).sum(), xerr.max(), xbound.max(),
                               (xerr / (MANY_K * cond * 2.0 ** -53)).max(),
                               (np.abs(rl - loss) / lscale).max()))
    bad = np.flatnonzero(xerr > xbound)
    assert len(bad) == 0, [(int(r), xerr[r], xbound[r]) for r in bad[:8]]
    bad = np.flatnonzero(np.abs(rl - loss) > 1e-9 * lscale)
    assert len(bad) == 0, [(int(r), rl[r], loss[r], lscale[r]) for r in bad[:8]]
    assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum(), (total, rl.sum())
    return set(failed.tolist()), lam_min


@pytest.mark.parametrize("nrows", [4096, 4097, 8193])
def test_many_flagged_rows(nrows):
    """fallback_grid = 1, 2, 3 workgroups, each scanning its share in 256-slot windows in
    which (nearly) every slot is flagged: every row against numpy, none lost at a share edge."""
    F, lam_min = check_many(nrows, np.arange(nrows))
    assert np.sum(lam_min < 0) >= 0.9 * nrows, np.sum(lam_min < 0)
    assert F >= set(np.flatnonzero(lam_min < -1e-6).tolist())


@pytest.mark.parametrize("nrows", [4096, 4097, 8193])
def test_few_flagged_rows_at_window_and_share_edges(nrows):
    """Only rows 255, 256, 2048, 2049 and nrows − 1 carry the negative value: exactly the
    indefinite ones among them are flagged (fp64 k = 16 has no route that flags a negative
    weight as such), and every row is right."""
    negative = np.array([255, 256, 2048, 2049, nrows - 1])
    F, lam_min = check_many(nrows, negative)
    assert np.all(np.abs(lam_min) > 1e-6)
    assert len(F) >= 4 and F == set(np.flatnonzero(lam_min < 0).tolist()) <= set(negative.tolist())


# ---- error paths
def small_case(k, nitems=20):
    """Five user rows of 2, 0, 1, 3 and 17 signals over `nitems` items."""
    rng = np.random.default_rng(5)
    lens = np.array([2, 0, 1, 3, 17])
    urp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ucol = np.concatenate([np.sort(rng.choice(nitems, n, replace=False)) for n in lens]).astype(np.int32)
    uval = rng.uniform(0.5, 5.0, int(urp[-1]))
    rows = np.repeat(np.arange(5), lens)
    order = np.lexsort((rows, ucol))
    irp = np.concatenate([[0], np.cumsum(np.bincount(ucol, minlength=nitems))]).astype(np.int64)
    return (urp, ucol, uval), (irp, rows[order].astype(np.int32), uval[order]), \
        rng.uniform(-0.3, 0.3, (nitems, k))


def check_half_against_numpy(c, urp, ucol, uval, Y):
    X, loss, _, S = ladder_reference(urp, ucol, uval, Y, ALPHA, LAM)
    total = c.wals_half(0, ALPHA, LAM)
    F, rl = c.factors(0), c.row_losses(0)
    assert len(c.failed_rows()) == 0
    full = np.diff(urp) > 0
    assert np.all(F[~full] == 0.0) and np.all(rl[~full] == 0.0)
    err = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    assert err.max() < 1e-9, err
    assert np.all(np.abs(rl - loss) <= 1e-9 * S)
    assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum()


def test_singular_rows_are_counted_and_the_context_survives():
    """An all-zero fixed side with λ = 0: every system is the zero matrix (padding apart).
    The direct kernel's first pivot is 0 on every row — the empty row included, whose system is
    YᵀY + λI = 0 itself — so all five rows are flagged, found exactly singular by the
    re-solve (its first column has no non-zero pivot) and counted in the −6 message.  The
    context then solves a well-posed half."""
    k = 8
    (urp, ucol, uval), (irp, icol, ival), Y = small_case(k)
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(5, len(irp) - 1)
        c.upload_csr(0, urp, ucol, uval)
        c.upload_csr(1, irp, icol, ival)
        c.set_factors(1, np.zeros_like(Y))
        with pytest.raises(qmf_amd.QmfxError, match=r"-6: 5 singular row system"):
            c.wals_half(0, ALPHA, 0.0)
        c.set_factors(1, Y)
        check_half_against_numpy(c, urp, ucol, uval, Y)


def test_non_finite_fixed_side_fails_and_the_context_survives():
    """One NaN in the fixed side makes YᵀY + λI's factorization fail (chol_inv's !(d > 0)):
    error −5 with whitened rows present.  No loop of chol_inv.hip, the whitened and direct
    kernels or fallback.hip depends on a value (the re-solve's only early exit is an exactly
    zero pivot column; NaN compares false and the elimination runs its KP steps), so the half
    ends; with finite factors the same context then matches numpy."""
    k = 32
    (urp, ucol, uval), (irp, icol, ival), Y = ladder_case(k, seed_of(k), 64)
    Ynan = Y.copy()
    Ynan[5, 3] = np.nan
    with qmf_amd.Context(k, 64) as c:
        c.set_shape(NROWS, len(irp) - 1)
        c.upload_csr(0, urp, ucol, uval)
        c.upload_csr(1, irp, icol, ival)
        c.set_factors(1, Ynan)
        assert c.row_classes(0)["whitened"][0] == 17
        with pytest.raises(qmf_amd.QmfxError, match="not positive definite"):
            c.wals_half(0, ALPHA, LAM)
        c.set_factors(1, Y)
        X, loss, _, S = ladder_solution(k, seed_of(k), 64, ALPHA, LAM)
        total = c.wals_half(0, ALPHA, LAM)
        F, rl = c.factors(0), c.row_losses(0)
        assert len(c.failed_rows()) == 0
    full = np.diff(urp) > 0
    err = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    assert err.max() < 1e-9 and np.all(F[~full] == 0.0)
    assert np.all(np.abs(rl - loss) <= 1e-9 * S)
    assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum()
