"""CPU-side checks of the similar-rows interface (include/qmfx.h qmfx_similar and
qmfx_factor_norms): the header declares both calls and the two metrics, the ctypes table
carries them with the right output types, and the numpy reference that the GPU tests compare
against gives the hand-computed answer on a six-row case with a duplicate row, a row that is
exactly twice another (an exact cosine tie) and a zero row."""
import ctypes
import os
import re

import numpy as np

import pyoracle as po
import qmf_amd
from helpers import ROOT
from test_recommend import topn_reference

DOT, COSINE = 0, 1


def norms_reference(F):
    """norm(a) = sqrt(dot(a, a)): the squares summed in factor order, one rounded multiply and
    one rounded add each (numpy's elementwise operations), then numpy's correctly rounded sqrt."""
    F = np.asarray(F, np.float64)
    n2 = np.zeros(F.shape[0])
    for f in range(F.shape[1]):
        n2 = n2 + F[:, f] * F[:, f]
    return np.sqrt(n2)


def similar_reference(F, rows, topn, metric, exclude_self):
    """The contract of qmfx_similar restated in numpy: (neighbours[n, topn] int64,
    scores[n, topn], counts[n] int32) of the query rows `rows` of F among the rows of F."""
    F = np.asarray(F, np.float64)
    rows = np.asarray(rows, np.int64)
    S = po.test_scores(F, F, rows)
    if metric == COSINE:
        nrm = norms_reference(F)
        den = nrm[rows][:, None] * nrm[None, :]
        S = np.where(den > 0, S / np.where(den > 0, den, 1), 0.0)
    return topn_reference(S, topn, seen=[[r] for r in rows] if exclude_self else None)


def test_header_declares_both_calls_and_the_metrics():
    src = open(os.path.join(ROOT, "include", "qmfx.h")).read()
    decl = re.search(r"int qmfx_similar\(([^;]*)\);", src)
    assert decl, "qmfx_similar is not declared"
    args = decl.group(1)
    assert "int side" in args and "const int64_t* rows" in args and "int metric" in args
    assert "int exclude_self" in args
    assert "int64_t* neighbours" in args and "double* scores" in args and "int32_t* counts" in args
    norms = re.search(r"int qmfx_factor_norms\(([^;]*)\);", src)
    assert norms and "int side" in norms.group(1) and "double* norms" in norms.group(1)
    assert re.search(r"#define QMFX_SIM_DOT 0\b", src)
    assert re.search(r"#define QMFX_SIM_COSINE 1\b", src)
    assert qmf_amd.QMFX_SIM_DOT == DOT and qmf_amd.QMFX_SIM_COSINE == COSINE


def test_signature_table_types_the_outputs():
    sig = qmf_amd._abi.SIGNATURES["qmfx_similar"]
    assert len(sig) == 10
    assert sig[1] is ctypes.c_int and sig[2] is ctypes.c_int64
    assert sig[3] is ctypes.POINTER(ctypes.c_int64)   # rows
    assert sig[4] is sig[5] is sig[6] is ctypes.c_int  # topn, metric, exclude_self
    assert sig[7] is ctypes.POINTER(ctypes.c_int64)   # neighbours
    assert sig[8] is ctypes.POINTER(ctypes.c_double)  # scores
    assert sig[9] is ctypes.POINTER(ctypes.c_int32)   # counts
    nsig = qmf_amd._abi.SIGNATURES["qmfx_factor_norms"]
    assert len(nsig) == 3 and nsig[1] is ctypes.c_int
    assert nsig[2] is ctypes.POINTER(ctypes.c_double)
    L = qmf_amd.lib()
    assert hasattr(L, "qmfx_similar") and hasattr(L, "qmfx_factor_norms")
    assert callable(qmf_amd.Context.similar) and callable(qmf_amd.Context.factor_norms)


def test_numpy_reference_on_a_hand_computed_case():
    # row 1 duplicates row 0, row 2 is exactly 2 x row 0, row 3 is the zero row
    F = np.array([[3.0, 4.0],
                  [3.0, 4.0],
                  [6.0, 8.0],
                  [0.0, 0.0],
                  [4.0, -3.0],
                  [-3.0, -4.0]])
    assert norms_reference(F).tolist() == [5.0, 5.0, 10.0, 0.0, 5.0, 5.0]
    rows = [0, 3, 2]
    # dot with row 0: 25, 25, 50, 0, 0, -25
    nb, sc, cnt = similar_reference(F, rows, 4, DOT, True)
    assert nb.tolist() == [[2, 1, 3, 4], [0, 1, 2, 4], [0, 1, 3, 4]]
    assert sc.tolist() == [[50.0, 25.0, 0.0, 0.0], [0.0] * 4, [50.0, 50.0, 0.0, 0.0]]
    assert cnt.tolist() == [4, 4, 4]
    # cosine with row 0: 1, 1, 1 (scaling by 2 is exact), 0 (zero row), 0, -1: ties by index
    nb, sc, cnt = similar_reference(F, rows, 4, COSINE, True)
    assert nb.tolist() == [[1, 2, 3, 4], [0, 1, 2, 4], [0, 1, 3, 4]]
    assert sc.tolist() == [[1.0, 1.0, 0.0, 0.0], [0.0] * 4, [1.0, 1.0, 0.0, 0.0]]
    # the query itself comes first when it is not excluded (row 2: rows 0 and 1 tie with it)
    nb, sc, cnt = similar_reference(F, rows, 3, COSINE, False)
    assert nb.tolist() == [[0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert sc.tolist() == [[1.0] * 3, [0.0] * 3, [1.0] * 3]
    # a list longer than the eligible rows: five neighbours, the tail -1 / 0.0
    nb, sc, cnt = similar_reference(F, [5], 8, COSINE, True)
    assert cnt.tolist() == [5]
    assert nb.tolist() == [[3, 4, 0, 1, 2, -1, -1, -1]]
    assert sc.tolist() == [[0.0, 0.0, -1.0, -1.0, -1.0, 0.0, 0.0, 0.0]]
