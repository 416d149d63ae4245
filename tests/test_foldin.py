"""CPU-side checks of the fold-in interface (include/qmfx.h qmfx_wals_fold_in,
qmfx_fold_in_classes, qmfx_fold_in_order, qmfx_recommend_fold_in): the header declares the
calls, the ctypes table carries them with the header's argument types, and the numpy
restatements that the GPU tests compare against (the device-built row plan, the fold-in case
and its per-row errors) give the hand-computed answers on small cases."""
import ctypes
import os
import re

import numpy as np

import qmf_amd
from helpers import ROOT, ladder_reference

ALPHA, LAM = 40.0, 0.05
NFIXED = 300
# The row lengths of the fold-in case: every whitened bucket edge (16j, 16j + 1) up to the
# largest bucket any tiling has (n = 128), one row past it, and a row as long as the fixed side
# (with repeated columns).  96 / 97 and 112 / 113 fill buckets 6 and 7 of the fp32 k = 128
# tiling, so that no bucket with a kernel stays empty.
LENGTHS = (0, 1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 300)

_CTYPES = {"qmfx_ctx*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
           "double": ctypes.c_double, "const int64_t*": ctypes.POINTER(ctypes.c_int64),
           "int64_t*": ctypes.POINTER(ctypes.c_int64),
           "const int32_t*": ctypes.POINTER(ctypes.c_int32),
           "int32_t*": ctypes.POINTER(ctypes.c_int32),
           "const double*": ctypes.POINTER(ctypes.c_double),
           "double*": ctypes.POINTER(ctypes.c_double)}


def plan_reference(rowptr, max_ntn):
    """The row plan of a fold-in restated in numpy: a row of n signals belongs to whitened
    bucket (max(n, 1) + 15) // 16 when that is ≤ max_ntn, else to the direct rows.  Returns
    (order, wb): the whitened buckets in ascending order with rows ascending inside each, then
    the direct rows by descending n with ties by ascending row; wb[b] = the first slot of
    bucket b + 1 for b < 8, wb[8] = the first direct slot.  This is what build_buckets lays out
    for the same rows in one piece without split-K rows."""
    n = np.diff(np.asarray(rowptr, np.int64))
    rows = np.arange(len(n))
    ntn = (np.maximum(n, 1) + 15) // 16
    white = ntn <= max_ntn
    w = rows[white][np.lexsort((rows[white], ntn[white]))]
    d = rows[~white][np.lexsort((rows[~white], -n[~white]))]
    wb = np.array([int(np.sum(ntn[white] < b + 1)) for b in range(9)], np.int64)
    return np.concatenate([w, d]).astype(np.int64), wb


def classes_of(wb, nrows):
    """qmfx_fold_in_classes' 11 counts from plan_reference's boundaries."""
    return [int(wb[b + 1] - wb[b]) for b in range(8)] + [int(nrows - wb[8]), 0, 0]


def foldin_case(k, precision, seed=7, lengths=LENGTHS, nfixed=NFIXED):
    """(rowptr, col, val, Y): one new row of every length in `lengths` against `nfixed` fixed
    rows with factors Y uniform(-0.01, 0.01); a row's columns are distinct and ascending,
    except a row at least as long as the fixed side, whose columns are drawn with repetition
    (ascending); values uniform(0, 5) with every seventh exactly 0.  precision 32 rounds the
    values and Y to fp32 first, so the numpy reference solves the problem the device holds."""
    rng = np.random.default_rng(seed + k)
    lens = np.asarray(lengths, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = []
    for n in lens:
        if n >= nfixed:
            c = np.sort(rng.integers(0, nfixed, n))
            assert len(np.unique(c)) < n
        else:
            c = np.sort(rng.choice(nfixed, n, replace=False))
        cols.append(c)
    col = np.concatenate(cols).astype(np.int32)
    val = rng.uniform(0.0, 5.0, int(rowptr[-1]))
    val[::7] = 0.0
    Y = rng.uniform(-0.01, 0.01, (nfixed, k))
    if precision == 32:
        val = val.astype(np.float32).astype(np.float64)
        Y = Y.astype(np.float32).astype(np.float64)
    return rowptr, col, val, Y


def row_errors(F, losses, rowptr, col, val, Y, alpha=ALPHA, lam=LAM):
    """Per-row errors against numpy's fp64 solve of the systems formed from Y, normalised as
    tests/test_wals_rows_gpu.py does: ‖x − x_ref‖∞ / ‖x_ref‖∞ (0 for a row without signals,
    whose x must be exactly 0) and |loss − loss_ref| / S_r.  Returns (xerr, lerr, X, loss)."""
    X, loss, _, S = ladder_reference(rowptr, col, val, Y, alpha, lam)
    n = np.diff(rowptr)
    full = n > 0
    xerr = np.zeros(len(n))
    xerr[full] = np.max(np.abs(F - X)[full], axis=1) / np.max(np.abs(X[full]), axis=1)
    xerr[~full] = np.where(np.all(F[~full] == 0.0, axis=1), 0.0, np.inf)
    lerr = np.abs(losses - loss) / np.where(S > 0, S, 1.0)
    return xerr, lerr, X, loss


def bars(precision):
    """The project's bars on a solved row (factors, loss)."""
    return (1e-9, 1e-9) if precision == 64 else (1e-4, 1e-4)


def _declared(name):
    src = open(os.path.join(ROOT, "include", "qmfx.h")).read()
    decl = re.search(r"int %s\(([^;]*)\);" % name, src)
    assert decl, name + " is not declared"
    args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
    types = []
    for a in args.split(","):
        words = a.split()
        t = " ".join(words[:-1])          # drop the parameter name
        if words[-1].startswith("*"):
            t += "*"
        types.append(t.replace(" *", "*"))
    return types


def test_abi_table_matches_the_header():
    for name, nargs in (("qmfx_wals_fold_in", 11), ("qmfx_fold_in_classes", 2),
                        ("qmfx_fold_in_order", 2), ("qmfx_recommend_fold_in", 13)):
        types = _declared(name)
        assert len(types) == nargs, (name, types)
        sig = qmf_amd._abi.SIGNATURES[name]
        assert len(sig) == nargs, name
        for i, (t, s) in enumerate(zip(types, sig)):
            assert _CTYPES[t] is s, (name, i, t, s)
        assert hasattr(qmf_amd.lib(), name)
    for m in ("wals_fold_in", "fold_in_classes", "fold_in_order", "recommend_fold_in"):
        assert callable(getattr(qmf_amd.Context, m))


def test_plan_reference_on_a_hand_computed_case():
    #        row: 0  1   2   3   4   5   6   7   8
    n = np.array([0, 40, 16, 17, 40, 1, 200, 33, 64])
    rp = np.concatenate([[0], np.cumsum(n)])
    order, wb = plan_reference(rp, 2)
    # bucket 1 (n ≤ 16): rows 0, 2, 5; bucket 2 (n ≤ 32): row 3; direct: 200, 64, 40, 40, 33
    assert order.tolist() == [0, 2, 5, 3, 6, 8, 1, 4, 7]
    assert wb.tolist() == [0, 3, 4, 4, 4, 4, 4, 4, 4]
    assert classes_of(wb, len(n)) == [3, 1, 0, 0, 0, 0, 0, 0, 5, 0, 0]
    order, wb = plan_reference(rp, 0)  # no whitened kernels: every row direct
    assert order.tolist() == [6, 8, 1, 4, 7, 3, 2, 5, 0]
    assert wb.tolist() == [0] * 9
    order, wb = plan_reference(rp, 8)
    assert order.tolist() == [0, 2, 5, 3, 1, 4, 7, 8, 6]
    assert classes_of(wb, len(n)) == [3, 1, 3, 1, 0, 0, 0, 0, 1, 0, 0]


def test_foldin_case_has_every_length_and_a_repeated_column():
    rp, col, val, Y = foldin_case(8, 32)
    assert np.diff(rp).tolist() == list(LENGTHS) and Y.shape == (NFIXED, 8)
    assert col.min() >= 0 and col.max() < NFIXED
    for r in range(len(LENGTHS)):
        c = col[rp[r]:rp[r + 1]]
        assert np.all(np.diff(c) >= 0)
        assert (len(np.unique(c)) < len(c)) == (LENGTHS[r] >= NFIXED)
    assert np.array_equal(val, val.astype(np.float32).astype(np.float64))
    # the reference's solution of the case has zero error against itself, and a perturbed
    # one is measured in units of the row's largest factor
    X, loss, _, _ = ladder_reference(rp, col, val, Y, ALPHA, LAM)
    xerr, lerr, _, _ = row_errors(X, loss, rp, col, val, Y)
    assert np.all(xerr == 0.0) and np.all(lerr == 0.0)
    F = X.copy()
    F[3, 0] += 1e-3 * np.max(np.abs(X[3]))
    F[0, 1] = 1e-30  # the empty row must be exactly 0
    xerr, _, _, _ = row_errors(F, loss, rp, col, val, Y)
    assert abs(xerr[3] - 1e-3) < 1e-12 and xerr[0] == np.inf
