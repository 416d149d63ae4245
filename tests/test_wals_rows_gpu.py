"""WALS row kernels on the MI355X, row by row against numpy: every row length at which a route
changes, every factor tiling, off-tile factor counts, other (α, λ), split-K segment edges.

The fixture is helpers.ladder_case: 181 user rows, one of every length 0..170 and
255/256/257, 383/384/385, 511/512/513, 640, in a seeded random row order, so every whitened
bucket edge (n = 16j, 16j + 1), the last whitened and first direct length of every tiling,
every n mod 4 of the 4-wide MFMA tail and every partial LDS stage of the multi-wave kernel is
a row of its own, and a row with no signals is among them.  The reference is
helpers.ladder_reference (numpy fp64, anchored on the CPU oracle by
tests/test_oracle.py::test_ladder_reference_matches_oracle); an fp32 context's inputs are
rounded to fp32 first, so both sides solve the same problem.

Per case (one wals_half(0, …)), every row on its own:
  factors  ‖x_dev − x_ref‖∞ / ‖x_ref‖∞ < 1e-9 (fp64) or max(1e-4, k·cond_r·2⁻²⁴) (fp32: the
           project's two stated bars; the fp32 bound is asserted to stay ≤ 2e-3);
  loss     |loss_dev − loss_ref| ≤ tol·S_r, S_r = Σc + |xᵀ(A − λI)x| + 2|xᵀb|, tol 1e-9 / 1e-4
           (fp32 summation's worst case (n + k)·2⁻²⁴ stays under 1e-4 for n + k ≤ 1600); the
           returned sum equals Σ row_losses to 1e-12·Σ|loss_r|;
  no row took the pivoted re-solve (it would mask a kernel); the empty row's x and loss are
  exactly 0; row_classes holds exactly the ladder's count in every whitened bucket the
  tiling has a kernel for (WB_MAX below restates the policy), the rest direct / heavy.

An empty row is in bounds on every route by construction: the whitened kernels read a row's
(column, value) only in lanes below n and gather the all-zero padding row otherwise, and the
direct, multi-wave and split-K Gram loops return before their first load when n = 0.

Measured on an MI355X, 162 cases in 15 s (all pass on the unmodified library; no kernel bug
found).  Largest per-row errors over all cases, beside their bounds:

  precision route       factors (bound)                     loss / S_r (tol)
  fp64      whitened    1.8e-14 (1e-9)                      5.8e-16 (1e-9)
  fp64      direct      1.0e-14 (1e-9)                      6.5e-16 (1e-9)
  fp64      multi-wave  2.6e-14 (1e-9)                      4.0e-16 (1e-9)
  fp64      split-K     1.1e-14 (1e-9)                      3.4e-16 (1e-9)
  fp32      whitened    1.7e-6  (7.4e-4 there)              1.8e-7  (1e-4)
  fp32      direct      8.1e-6  (1e-4 there: k = 1)         1.0e-7  (1e-4)
  fp32      multi-wave  1.4e-5  (2e-3 there: k = 256, λ = 1e-3)  1.5e-7  (1e-4)
  fp32      split-K     4.5e-6  (5.7e-4 there: k = 200)     6.7e-8  (1e-4)

Largest fp32 bound k·cond·2⁻²⁴ at λ ≥ 0.05: 9.4e-4 (k = 256), under the 2e-3 cap.  Only
(α, λ) = (40, 1e-3) at k = 256 exceeds it (cond₂ = 274 → 4.2e-3); those rows are held to 2e-3.

Single-line mutants of the library, each run once (new cases failing of 162; older WALS tests
of test_wals_gpu / test_heavy_gpu / test_configs_gpu that fail too, of 93):
  padding diagonal of G + λI's image 0 instead of 1 ............ 42 new (only through the
      no-re-solve assertion: the pivoted re-solve repairs the factors), 2 old
  −λ‖x‖² left out of the unwhitening GEMM's row loss ............ 41 new, 31 old
  rows of n = 16j + 1 sent to whitened bucket j ................. 80 new, 50 old
  second signal per lane ignored in the fp32 n > 64 buckets ..... 11 new, 8 old
  split-K reduce skips a row's last segment (tiles) ............. 8 new, 10 old
  fp64 direct Gram drops the last signal when n mod 4 = 1 ....... 49 new, 31 old
"""
import time

import numpy as np
import pytest

import qmf_amd
from helpers import LADDER_LENGTHS, ladder_case, ladder_solution

pytestmark = pytest.mark.gpu

ALPHA, LAM = 40.0, 0.05
NROWS = len(LADDER_LENGTHS)
# Largest whitened bucket (n ≤ 16·NTN) per precision and factor tiling nt = ⌈k/16⌉, restated
# from DESIGN §3.3: n ≤ KP/2 and ≤ 64; k = 64 whitens n ≤ 64 (fp32) / 48 (fp64); the
# two-signals-per-lane buckets of k = 128 / 256 reach n = 128 (fp32) / 80 (fp64); no whitened
# kernel at k ≤ 16 or on the multi-wave tilings nt = 9..15.
WB_MAX = {32: {2: 1, 3: 1, 4: 4, 5: 2, 6: 3, 7: 3, 8: 8, 16: 8},
          64: {2: 1, 3: 1, 4: 3, 5: 2, 6: 3, 7: 3, 8: 5, 16: 5}}
HEAVY = {"QMFX_HEAVY_MIN": "128", "QMFX_SEG_LEN": "64"}  # SEG_LEN 64: the clamp's minimum


def seed_of(k):
    return 1000 + k


def run_ladder(k, precision, monkeypatch, alpha=ALPHA, lam=LAM, whiten=True, heavy=False):
    """One user half on the ladder with every check of the module's docstring.  Returns the
    context's row classes."""
    if not whiten:
        monkeypatch.setenv("QMFX_NO_WHITEN", "1")
    for key, v in (HEAVY if heavy else {}).items():
        monkeypatch.setenv(key, v)
    t0 = time.perf_counter()
    (urp, ucol, uval), (irp, icol, ival), Y = ladder_case(k, seed_of(k), precision)
    X, loss, cond, S = ladder_solution(k, seed_of(k), precision, alpha, lam)
    t1 = time.perf_counter()
    n = np.diff(urp)
    assert sorted(n) == sorted(LADDER_LENGTHS) and len(n) == NROWS
    nt = (k + 15) // 16
    with qmf_amd.Context(k, precision) as c:  # the QMFX_* settings are read at create
        c.set_shape(NROWS, len(irp) - 1)
        c.upload_csr(0, urp, ucol, uval)
        c.upload_csr(1, irp, icol, ival)
        c.set_factors(1, Y)
        rc = c.row_classes(0)
        total = c.wals_half(0, alpha, lam)
        F, rl, failed = c.factors(0), c.row_losses(0), c.failed_rows()
        whitened_launches = c.kernel_stats(1)["launches"]
    # ---- routes: the plan holds the ladder's count in every bucket that has a kernel
    mx = WB_MAX[precision].get(nt, 0) if whiten else 0
    bucket = (np.maximum(n, 1) + 15) // 16  # NTN of a row
    want = [int(np.sum(bucket == j + 1)) if j < mx else 0 for j in range(8)]
    assert all(w == (0 if j >= mx else 17 if j == 0 else 16) for j, w in enumerate(want))
    assert rc["whitened"] == want, (rc, want)
    is_w = bucket <= mx
    is_h = (n > 128) & ~is_w if heavy else np.zeros(NROWS, bool)
    assert rc["heavy"] == int(is_h.sum()) and rc["direct"] == NROWS - sum(want) - rc["heavy"], rc
    assert rc["segments"] == int(np.sum((n[is_h] + 63) // 64)), rc
    # the whitened form needs λ > 0: without it (or without buckets) its kernels never launch
    uses_w = mx > 0 and lam > 0
    assert whitened_launches == (1 if uses_w else 0), whitened_launches
    if not uses_w:
        is_w = np.zeros(NROWS, bool)
    # ---- SPD systems: the pivoted re-solve must not have run
    assert len(failed) == 0, failed
    # ---- the empty row
    r0 = int(np.flatnonzero(n == 0)[0])
    assert np.all(F[r0] == 0.0) and rl[r0] == 0.0 and loss[r0] == 0.0 and np.all(X[r0] == 0.0)
    # ---- per row
    full = n > 0
    xerr = np.zeros(NROWS)
    xerr[full] = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    if precision == 64:
        xbound, ltol = np.full(NROWS, 1e-9), 1e-9
    else:
        # The tolerance must not go vacuous: never above 2e-3.  At the reference's λ (and any
        # larger one) k·cond·2⁻²⁴ stays below that on this recipe and the test asserts it;
        # λ = 1e-3 at k = 256 has rows with cond₂ = 274 (numpy), k·cond·2⁻²⁴ = 4.2e-3: those
        # rows are held to 2e-3 instead.
        xbound, ltol = np.maximum(1e-4, k * cond * 2.0 ** -24), 1e-4
        assert xbound.max() <= 2e-3 or lam < LAM, xbound.max()
        xbound = np.minimum(xbound, 2e-3)
    lerr = np.abs(rl - loss) / np.where(S > 0, S, 1.0)  # in units of S_r
    route = np.where(is_w, "whitened", np.where(is_h, "split-K", "multi-wave" if nt > 8 else "direct"))
    for name in ("whitened", "direct", "multi-wave", "split-K"):
        m = (route == name) & full
        if m.any():
            print("LADDER k=%d p=%d a=%g l=%g w=%d h=%d route=%s rows=%d xerr=%.3g xbound=%.3g "
                  "lerr=%.3g ltol=%.3g" % (k, precision, alpha, lam, whiten, heavy, name, m.sum(),
                                           xerr[m].max(), xbound[m].max(), lerr[m].max(), ltol))
    print("LADDER_TIME k=%d p=%d reference %.2f s (0 when shared), device and checks %.2f s"
          % (k, precision, t1 - t0, time.perf_counter() - t1))
    bad = np.flatnonzero(xerr >= xbound)
    assert len(bad) == 0, [(int(r), int(n[r]), route[r], xerr[r], xbound[r]) for r in bad[:8]]
    bad = np.flatnonzero(np.abs(rl - loss) > ltol * S)
    assert len(bad) == 0, [(int(r), int(n[r]), route[r], rl[r], loss[r], S[r]) for r in bad[:8]]
    assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum(), (total, rl.sum())
    return rc


@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("nt", range(1, 17))
def test_every_tiling(nt, precision, whiten, monkeypatch):
    """k = 16·nt for every factor tiling, whitening on and QMFX_NO_WHITEN=1 (all 181 rows on
    the direct route: one-wave at nt ≤ 8, multi-wave above)."""
    rc = run_ladder(16 * nt, precision, monkeypatch, whiten=whiten)
    if not whiten:
        assert rc["direct"] == NROWS and sum(rc["whitened"]) == 0


OFF_TILE = [1, 2, 3, 5, 15, 17, 31, 33, 47, 63, 65, 79, 81, 100, 127, 129, 143, 145, 161, 177,
            209, 225, 241, 255]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k,whiten", [(k, True) for k in OFF_TILE] +
                         [(k, False) for k in (17, 65, 129, 255)])
def test_off_tile_factor_counts(k, whiten, precision, monkeypatch):
    """k one past and one short of a tile (and a few in between): the padding columns — the
    unit diagonal of G + λI's image, the padded L⁻¹, the zero tails of Y — on every route."""
    rc = run_ladder(k, precision, monkeypatch, whiten=whiten)
    if not whiten:
        assert rc["direct"] == NROWS


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("alpha,lam", [(1.0, 0.0), (0.5, 10.0), (40.0, 1e-3)])
@pytest.mark.parametrize("k", [32, 64, 100, 128, 256])
def test_other_alpha_lambda(k, alpha, lam, precision, monkeypatch):
    """Away from the reference's (40, 0.05).  λ = 0 has no whitened form (YᵀY alone is
    well-posed with 1024 items, but the whitening needs λ > 0): every row is solved by the
    direct kernels, which run_ladder asserts from the whitened class's launch count."""
    run_ladder(k, precision, monkeypatch, alpha=alpha, lam=lam)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("k", [32, 64, 100, 128, 200, 256])
def test_split_k_segment_edges(k, precision, monkeypatch):
    """QMFX_HEAVY_MIN=128, QMFX_SEG_LEN=64: every ladder row longer than 128 is split-K (52
    rows), n = 128 stays whole, 129 / 257 / 385 / 513 end in a one-signal segment and
    256 / 384 / 512 / 640 are exact multiples of the segment."""
    rc = run_ladder(k, precision, monkeypatch, heavy=True)
    assert rc["heavy"] == 52
    assert rc["segments"] == sum((n + 63) // 64 for n in LADDER_LENGTHS if n > 128) == 193
