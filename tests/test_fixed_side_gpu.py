"""The fixed-side stages of a WALS half on the MI355X at every fixed-side row count: G = YᵀY
(gram_partial_kernel / gram_tiles_kernel and their reduce kernels), L⁻¹ of G + λI
(chol_inv_kernel / chol_inv_global_kernel), Z = Y·L⁻ᵀ and, after the row kernels, x = L⁻ᵀx' with
rowloss −= λ‖x‖² (whiten_kernel / whiten_lds_kernel).  tests/test_wals_rows_gpu.py moves the row
length and the factor count; its fixed side always has max(1024, 4k) rows of uniform(−0.01, 0.01)
factors, for which L⁻¹ is nearly a multiple of I.  This module moves the fixed side's row count
and makes L⁻¹ matter.

1. test_gram_is_exact_at_every_block_edge.  The solved side is one row with one signal of value
   exactly 0 (w = 0, c = 1), α = 1, λ = 0.25, Y drawn from {−2, −1, 0, 1, 2}/8, so
   qmfx_wals_row_system returns A = G + λI, b = that row of Y, Σc = 1.  Every product of G is a
   multiple of 1/64 and every partial sum over at most 69 633 rows an integer below 2²⁴ of them:
   G is exact in fp32 and fp64 in any summation order, and the test compares A − λI with numpy's
   Y.T @ Y bit for bit, with no tolerance.  Row counts (a fresh context each): GRAM_BASE, one
   short of / equal to / one past one and two multiples of BigCfg::SIG (32 rows fp32, 16 fp64),
   and the counts at which rows_per_block = ⌈n / gpart_blocks⌉ rounded up to 4 leaves 64:
   65 536, 65 537 (68 rows per block, the last of 964 blocks has 53), 69 632, 69 633 (72 rows,
   last block 9) at nt ≤ 8 and 16 384, 16 385, 17 408, 17 409 above; gram_blocks() restates the
   launcher's formula and the test asserts those properties of the list.

2. test_whitening_inverse_and_unwhitening.  helpers.fixed_side_case(M, N): every row of both
   sides has 1..16 signals (whitened bucket 1) and every fixed-side row is gathered by some
   solved row, so a wrong row of Z, a wrong element of L⁻¹ or a wrong unwhitened row is some
   row's wrong answer.  Factors are helpers.correlated_factors (uniform · a k×k matrix with
   singular values 1 .. 0.1, scaled to ‖Y‖₂ = 1), values uniform(0.05, 1], α = 1, λ = 0.05; the
   test asserts that the largest off-diagonal entry of numpy's L⁻¹ is at least 0.1 of its
   largest diagonal entry (smallest seen: 0.16).  (M, N) runs over each value of FIXED_LADDER
   with its successor (1 .. 1025: a wave's 32-row block, whiten_kernel's 128-row and
   whiten_lds_kernel's 256-row workgroup, each ± 1); half 0 whitens N rows and unwhitens M, half
   1 the reverse, each against the other side's factors as set by the test.  The reference is
   helpers.ladder_reference, the bars are those of test_wals_rows_gpu.py, per row:
     factors  ‖x_dev − x_ref‖∞ / ‖x_ref‖∞ < 1e-9 (fp64) or max(1e-4, k·cond_r·2⁻²⁴) (fp32; asserted
              ≤ 2e-3, largest here 5.7e-4 at k = 256);
     loss     |loss_dev − loss_ref| ≤ 1e-9·S_r (fp64) / 1e-4·S_r (fp32); the returned total equals
              Σ row losses to 1e-12·Σ|loss_r|;
   row_classes holds every row in whitened bucket 1, the whitened class launched once, and no
   row took the pivoted re-solve.  The fp64 k ≤ 128 ladders run a second time with
   QMFX_WHITEN_GRID=1 (one workgroup: each wave strides over up to five 32-row blocks), checked
   against numpy again.  The numpy reference is the cost (2.8 ms per row at k = 256 fp32, where
   cond needs eigvalsh; fp64 cases skip cond), so a (k, precision) ladder is cut into consecutive
   runs of halves of about 3 s of reference work each: no row count is dropped.

Measured on an MI355X: 41 cases in 50 s, all passing on the unmodified library (no kernel bug
found); the Gram cases take 0.1 – 0.3 s each, the slowest whitening case 2.3 s (reference 2.2 s;
the device calls of a whole 54-half ladder take 0.02 – 0.2 s).  Largest per-row errors, beside
their bars:

  kernels                                       factors (bar)             loss / S_r (bar)
  fp32 whiten_kernel, chol_inv_kernel           4.9e-6  (2.9e-4 there)    1.6e-6  (1e-4)
  fp32 whiten_kernel, chol_inv_global_kernel    5.8e-6  (5.7e-4 there)    8.3e-7  (1e-4)
  fp64 whiten_lds_kernel, chol_inv_kernel       1.1e-14 (1e-9)            3.7e-15 (1e-9)
  fp64 the same, QMFX_WHITEN_GRID=1             1.1e-14 (1e-9)            3.7e-15 (1e-9)
  fp64 whiten_kernel, chol_inv_global_kernel    1.9e-14 (1e-9)            2.3e-15 (1e-9)

Single-line mutants of the library, all in bounds, none committed, each built and run once
(failing cases of this module's 41: Gram + whitening; failing cases of the 255 older WALS tests
in test_wals_gpu / test_heavy_gpu / test_configs_gpu / test_wals_rows_gpu):
  whiten_kernel skips its second row group's store .............. 0 + 24 (every whiten_kernel
      case), 82 old
  whiten_lds_kernel's stride one 32-row block too long ........... 0 + 4 (the four
      QMFX_WHITEN_GRID=1 cases), 4 old (test_whitening_grid_strides_bit_identical at k = 64
      and 128, two test_heavy_gpu cases at k = 128 fp64)
  gram_partial_kernel's r1 one short ............................. 5 + 11 (every one-wave Gram
      case), 118 old
  gram_tiles_kernel's fetch guard e < r1 − 1 ..................... 4 + 21 (every tiled Gram
      case), 122 old
  chol_inv_global_kernel's inverse ignores lane q = 3 ............ 0 + 17 (every k > 128 case),
      28 old
  −λ‖x‖² of the unwhitening applied to order[max(ro − 1, 0)] ..... 0 + 32 (every whitening
      case), 102 old
These mutants hit every block, so the older whole-problem tests see them too; what this module
adds is the edge cases: exactness at the partial last block of every launch shape, a reference
for the strided whitening (the older check compares two device runs), and row-by-row factors
with an L⁻¹ whose off-diagonal part matters.
"""
import itertools
import time

import numpy as np
import pytest

import qmf_amd
from helpers import (FIXED_ALPHA, FIXED_LADDER, FIXED_LAM, fixed_side_case, fixed_side_solution)

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------
# 1. YᵀY exactly
# ---------------------------------------------------------------------------------------------
GRAM_LAM = 0.25
GRAM_BASE = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 66, 67, 68, 127, 128, 129, 255, 256, 257)
SIG = {32: 32, 64: 16}  # BigCfg<T, NT>::SIG (big.h): rows per LDS stage of gram_tiles_kernel
# where rows_per_block leaves 64: gpart_blocks (api_ctx.cpp) is 1024 at nt ≤ 8, 256 above
GRAM_LARGE = {1024: (65536, 65537, 69632, 69633), 256: (16384, 16385, 17408, 17409)}


def gram_max_blocks(nt):
    return 1024 if nt <= 8 else 256


def gram_blocks(n, nt):
    """(rows_per_block, nblocks) of launch_gram_nt / gram_big for n rows, restated."""
    mb = gram_max_blocks(nt)
    rpb = (n + mb - 1) // mb
    rpb = (rpb + 3) // 4 * 4
    rpb = max(rpb, 64)
    return rpb, (n + rpb - 1) // rpb


def gram_counts(k, precision):
    sig = SIG[precision]
    edges = [m * sig + d for m in (1, 2) for d in (-1, 0, 1)]
    return sorted(set(GRAM_BASE) | set(edges)) + list(GRAM_LARGE[gram_max_blocks((k + 15) // 16)])


@pytest.mark.parametrize("k,precision", [(16, 32), (16, 64), (100, 32), (128, 32), (64, 64),
                                         (80, 64), (144, 32), (255, 32), (256, 64)])
def test_gram_is_exact_at_every_block_edge(k, precision):
    """A − λI of qmfx_wals_row_system equals numpy's Y.T @ Y bit for bit (see the module
    docstring for why no rounding can occur), A is symmetric, b and Σc are exact."""
    nt = (k + 15) // 16
    counts = gram_counts(k, precision)
    assert all(m * SIG[precision] + d in counts for m in (1, 2) for d in (-1, 0, 1))
    # the list really reaches rows_per_block > 64 with a last block that is no multiple of 4
    tails = [(n, *gram_blocks(n, nt)) for n in counts]
    assert all(nb <= gram_max_blocks(nt) for _, _, nb in tails)
    assert any(rpb > 64 and (n - (nb - 1) * rpb) % 4 != 0 for n, rpb, nb in tails), tails
    assert any(rpb > 64 and n == nb * rpb for n, rpb, nb in tails), tails
    if nt <= 8:
        assert gram_blocks(65537, nt) == (68, 964) and 65537 - 963 * 68 == 53
    t0 = time.perf_counter()
    Yall = np.random.default_rng(9000 + k).integers(-2, 3, (max(counts), k)) / 8.0
    for n in counts:
        Y = Yall[:n]
        G = Y.T @ Y
        # every term is a multiple of 1/64 and every partial sum an integer below 2²⁴ of them
        assert np.all(G * 64 == np.round(G * 64)) and n * 4 < 2 ** 24
        col = n - 1
        one = np.array([0, 1], np.int64)
        irp = np.zeros(n + 1, np.int64)
        irp[col + 1:] = 1
        with qmf_amd.Context(k, precision) as c:
            c.set_shape(1, n)
            c.upload_csr(0, one, np.array([col], np.int32), np.array([0.0]))
            c.upload_csr(1, irp, np.array([0], np.int32), np.array([0.0]))
            c.set_factors(1, Y)
            A, b, csum = c.row_system(0, 0, 1.0, GRAM_LAM)
        Gd = A - GRAM_LAM * np.eye(k)
        bad = np.argwhere(Gd != G)
        assert len(bad) == 0, (n, gram_blocks(n, nt), len(bad),
                               [(int(i), int(j), Gd[i, j], G[i, j]) for i, j in bad[:4]])
        assert np.array_equal(A, A.T), n
        assert np.array_equal(b, Y[col]), n
        assert csum == 1.0, n
    print("GRAM_TIME k=%d p=%d %d row counts %.2f s" % (k, precision, len(counts),
                                                        time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------
# 2. whitening, L⁻¹ and unwhitening, row by row
# ---------------------------------------------------------------------------------------------
PAIRS = tuple(zip(FIXED_LADDER[:-1], FIXED_LADDER[1:]))
UNITS = tuple((m, n, side) for m, n in PAIRS for side in (0, 1))  # half 0, then half 1
CASE_MS = 3000.0


def row_ms(k, precision):
    """The numpy reference's cost per solved row in ms, a fit to one measurement (fp64: the
    solve; fp32: also eigvalsh for the bound): what chunks() cuts the ladder by."""
    r = k / 256.0
    return 0.1 + 1.2 * r * r + 1.5 * r ** 3 if precision == 32 else 0.03 + 0.3 * r * r + 0.26 * r ** 3


def chunks(k, precision):
    """UNITS cut into consecutive runs of at most CASE_MS of reference work each."""
    out, cur, cost = [], [], 0.0
    for m, n, side in UNITS:
        ms = (m, n)[side] * row_ms(k, precision)
        if cur and cost + ms > CASE_MS:
            out.append(tuple(cur))
            cur, cost = [], 0.0
        cur.append((m, n, side))
        cost += ms
    out.append(tuple(cur))
    return out


def family(k, precision):
    gemm = "whiten_lds_kernel" if precision == 64 and k <= 128 else "whiten_kernel"
    return gemm + " + " + ("chol_inv_global_kernel" if k > 128 else "chol_inv_kernel")


def run_units(k, precision, units, monkeypatch, grid=None):
    """The halves `units` ((m, n, side): side's rows solved against the other side's factors),
    one context per (m, n), with every check of the module's docstring."""
    if grid is not None:
        monkeypatch.setenv("QMFX_WHITEN_GRID", str(grid))  # read at every launch
    t_ref = t_dev = 0.0
    worst = {"xerr": 0.0, "xbound": 0.0, "lerr": 0.0, "ratio": np.inf, "rows": 0}
    for (m, n), sides in itertools.groupby(units, key=lambda u: u[:2]):
        ucsr, icsr, F = fixed_side_case(m, n, k, precision)
        with qmf_amd.Context(k, precision) as c:
            c.set_shape(m, n)
            c.upload_csr(0, *ucsr)
            c.upload_csr(1, *icsr)
            for _, _, side in sides:
                t0 = time.perf_counter()
                X, loss, cond, S, ratio = fixed_side_solution(m, n, k, precision, side)
                t1 = time.perf_counter()
                nrows, nfixed = (m, n)[side], (n, m)[side]
                c.set_factors(1 - side, F[1 - side])
                rc = c.row_classes(side)
                total = c.wals_half(side, FIXED_ALPHA, FIXED_LAM)
                D, rl, failed = c.factors(side), c.row_losses(side), c.failed_rows()
                launches = c.kernel_stats_side(1, side)["launches"]
                t_ref, t_dev = t_ref + t1 - t0, t_dev + time.perf_counter() - t1
                where = (k, precision, m, n, side)
                # ---- every row is whitened (bucket 1) and the whitened class launched once
                lens = np.diff((ucsr, icsr)[side][0])
                assert lens.min() >= 1 and lens.max() <= 16, (where, lens.min(), lens.max())
                assert rc == {"whitened": [nrows] + [0] * 7, "direct": 0, "heavy": 0,
                              "segments": 0}, (where, rc)
                assert launches == 1, (where, launches)
                # ---- every fixed-side row is gathered by a whitened row
                assert len(np.unique((ucsr, icsr)[side][1])) == nfixed, where
                # ---- the pivoted re-solve must not have run (it would mask a stage)
                assert len(failed) == 0, (where, failed[:8])
                # ---- L⁻¹ matters: far from a multiple of I
                if nfixed >= 2:
                    assert ratio >= 0.1, (where, ratio)
                    worst["ratio"] = min(worst["ratio"], ratio)
                # ---- per row
                xerr = np.max(np.abs(D - X), axis=1) / np.max(np.abs(X), axis=1)
                if precision == 64:
                    xbound, ltol = np.full(nrows, 1e-9), 1e-9
                else:
                    xbound, ltol = np.maximum(1e-4, k * cond * 2.0 ** -24), 1e-4
                    assert xbound.max() <= 2e-3, (where, xbound.max())  # never vacuous
                lerr = np.abs(rl - loss) / S
                bad = np.flatnonzero(~(xerr < xbound))
                assert len(bad) == 0, (where, [(int(r), xerr[r], xbound[r]) for r in bad[:8]])
                bad = np.flatnonzero(~(np.abs(rl - loss) <= ltol * S))
                assert len(bad) == 0, (where, [(int(r), rl[r], loss[r], S[r]) for r in bad[:8]])
                assert abs(total - rl.sum()) <= 1e-12 * np.abs(rl).sum(), (where, total, rl.sum())
                worst["xerr"] = max(worst["xerr"], xerr.max())
                worst["xbound"] = max(worst["xbound"], xbound.max())
                worst["lerr"] = max(worst["lerr"], lerr.max())
                worst["rows"] += nrows
    print("FIXED k=%d p=%d grid=%s family=%s halves=%d rows=%d xerr=%.3g xbound=%.3g lerr=%.3g "
          "ltol=%.0e min_offdiag_ratio=%.3g" % (k, precision, grid, family(k, precision),
                                                len(units), worst["rows"], worst["xerr"],
                                                worst["xbound"], worst["lerr"],
                                                1e-9 if precision == 64 else 1e-4, worst["ratio"]))
    print("FIXED_TIME k=%d p=%d grid=%s reference %.2f s (0 when shared), device calls %.2f s"
          % (k, precision, grid, t_ref, t_dev))


# (k, precision, QMFX_WHITEN_GRID): the fp64 k ≤ 128 ladders run a second time on one workgroup
# (each of its 8 waves strides over several 32-row blocks), directly after the first run of the
# same units, whose cached references they share
CONFIGS = [(32, 32), (64, 32), (100, 32), (128, 32), (256, 32),
           (32, 64), (64, 64), (100, 64), (128, 64), (256, 64), (241, 64)]
CASES, IDS = [], []
for _k, _p in CONFIGS:
    _ch = chunks(_k, _p)
    for _i, _units in enumerate(_ch):
        for _grid in (None, 1) if (_p == 64 and _k <= 128) else (None,):
            CASES.append((_k, _p, _grid, _units))
            IDS.append("k%d-fp%d-%s-%dof%d" % (_k, _p, "grid1" if _grid else "full", _i + 1,
                                               len(_ch)))
assert sorted(u for c in CASES if c[:3] == (256, 32, None) for u in c[3]) == sorted(UNITS)


@pytest.mark.parametrize("k,precision,grid,units", CASES, ids=IDS)
def test_whitening_inverse_and_unwhitening(k, precision, grid, units, monkeypatch):
    """Both halves of every (M, N) of the ladder among `units`: the whitening GEMM over the
    fixed side's rows, L⁻¹, and the unwhitening GEMM over the solved rows, against numpy."""
    run_units(k, precision, units, monkeypatch, grid)
