"""CPU-side checks of the top-N recommendation interface (include/qmfx.h qmfx_recommend): the
header declares the call and its three exclude modes, the ctypes table carries it with the
right output types, and the numpy reference that the GPU tests compare against gives the
hand-computed answer on a small case with a tie and a seen list."""
import ctypes
import os
import re

import numpy as np

import qmf_amd
from helpers import ROOT


def topn_reference(S, topn, seen=None):
    """The contract of qmfx_recommend restated in numpy.  S[t] are user t's scores of every
    item; item a ranks before item b when S[t, a] > S[t, b], or they are equal and a < b
    (np.lexsort on (index, -score): -0.0 and +0.0 compare equal, so the index decides).
    seen[t] (optional) are the item indices that are not eligible.  Returns
    (items[n, topn] int64, scores[n, topn], counts[n] int32); unused slots are -1 / 0.0."""
    n, ni = S.shape
    items = np.full((n, topn), -1, np.int64)
    scores = np.zeros((n, topn))
    counts = np.zeros(n, np.int32)
    for t in range(n):
        order = np.lexsort((np.arange(ni), -S[t]))
        if seen is not None and len(seen[t]):
            order = order[~np.isin(order, seen[t])]
        top = order[:topn]
        counts[t] = len(top)
        items[t, :len(top)] = top
        scores[t, :len(top)] = S[t, top]
    return items, scores, counts


def test_header_declares_recommend_and_its_modes():
    src = open(os.path.join(ROOT, "include", "qmfx.h")).read()
    decl = re.search(r"int qmfx_recommend\(([^;]*)\);", src)
    assert decl, "qmfx_recommend is not declared"
    args = decl.group(1)
    assert "int64_t* items" in args and "double* scores" in args and "int32_t* counts" in args
    assert re.search(r"#define QMFX_REC_MAX_N 128\b", src)
    assert re.search(r"#define QMFX_REC_ALL 0\b", src)
    assert re.search(r"#define QMFX_REC_UNSEEN_SIGNALS 1\b", src)
    assert re.search(r"#define QMFX_REC_UNSEEN_POSITIVES 2\b", src)


def test_signature_table_has_recommend_with_typed_outputs():
    sig = qmf_amd._abi.SIGNATURES["qmfx_recommend"]
    assert len(sig) == 9
    assert sig[1] is ctypes.c_int64 and sig[2] is ctypes.POINTER(ctypes.c_int64)
    assert sig[6] is ctypes.POINTER(ctypes.c_int64)   # items
    assert sig[7] is ctypes.POINTER(ctypes.c_double)  # scores
    assert sig[8] is ctypes.POINTER(ctypes.c_int32)   # counts
    assert hasattr(qmf_amd.lib(), "qmfx_recommend")
    assert callable(qmf_amd.Context.recommend)


def test_numpy_reference_on_a_hand_computed_case():
    # 3 users × 6 items; user 0 has a three-way tie at 2.0 (items 1, 3, 4) and -0.0 == +0.0
    S = np.array([[1.0, 2.0, 0.5, 2.0, 2.0, 3.0],
                  [-0.0, 0.0, -1.0, 5.0, 0.0, -0.0],
                  [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    items, scores, counts = topn_reference(S, 4)
    assert items.tolist() == [[5, 1, 3, 4], [3, 0, 1, 4], [5, 4, 3, 2]]
    assert scores[0].tolist() == [3.0, 2.0, 2.0, 2.0]
    assert counts.tolist() == [4, 4, 4]
    # seen lists: user 0 has seen 5 and 3, user 1 everything but item 2, user 2 everything
    seen = [np.array([3, 5]), np.array([0, 1, 3, 4, 5]), np.arange(6)]
    items, scores, counts = topn_reference(S, 4, seen)
    assert items.tolist() == [[1, 4, 0, 2], [2, -1, -1, -1], [-1, -1, -1, -1]]
    assert scores.tolist() == [[2.0, 2.0, 1.0, 0.5], [-1.0, 0.0, 0.0, 0.0], [0.0] * 4]
    assert counts.tolist() == [4, 1, 0]
