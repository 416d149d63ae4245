"""CPU-side checks of the explanation interface (include/qmfx.h qmfx_wals_explain,
qmfx_wals_explain_rows): the header declares the calls, the ctypes table carries them with the
header's argument types, and the numpy restatement that the GPU tests compare against gives the
hand-computed answer on a small case."""
import numpy as np

import qmf_amd
from test_foldin import _CTYPES, _declared


def explain_reference(rowptr, col, val, Y, row, target, alpha, lam, topm=None):
    """Plain numpy fp64: A = YᵀY + Σ_e αv_e·y_e y_eᵀ + λI over the signals e of `row` in CSR
    order, z = A⁻¹y_target, contrib_e = (1 + αv_e)·(y_e·z).  Returns (contrib, order): the full
    vector in CSR order and the positions of its first `topm` (default: all) entries in rank
    order: descending contribution, equal contributions by ascending position (a stable sort).

    Worked by hand, k = 1: Y = [1, 2, 3]ᵀ, the row holds columns 0 and 1 with v = 1 and 0.5,
    α = 2, λ = 1.  G = 1 + 4 + 9 = 14, w = (2, 1), c = (3, 2),
    A = 14 + 2·1² + 1·2² + 1 = 21.  Target 2: z = 3/21 = 1/7,
    contrib = (3·1·(1/7), 2·2·(1/7)) = (3/7, 4/7), total = 1 — and indeed b = 3·1 + 2·2 = 7,
    x̂ = 7/21 = 1/3, y_t·x̂ = 3·(1/3) = 1.  Rank order: position 1, then position 0."""
    Y = np.asarray(Y, np.float64)
    sl = slice(int(rowptr[row]), int(rowptr[row + 1]))
    Yr = Y[np.asarray(col[sl], np.int64)]
    w = alpha * np.asarray(val[sl], np.float64)
    A = Y.T @ Y + (Yr.T * w) @ Yr + lam * np.eye(Y.shape[1])
    z = np.linalg.solve(A, Y[target])
    contrib = (1.0 + w) * (Yr @ z)
    order = np.argsort(-contrib, kind="stable")
    return contrib, order[:len(order) if topm is None else topm]


def test_abi_table_matches_the_header():
    for name, nargs in (("qmfx_wals_explain", 15), ("qmfx_wals_explain_rows", 17),
                        ("qmfx_row_lengths", 5)):
        types = _declared(name)
        assert len(types) == nargs, (name, types)
        sig = qmf_amd._abi.SIGNATURES[name]
        assert len(sig) == nargs, name
        for i, (t, s) in enumerate(zip(types, sig)):
            assert _CTYPES[t] is s, (name, i, t, s)
        assert hasattr(qmf_amd.lib(), name)
    for m in ("wals_explain", "wals_explain_rows", "row_lengths"):
        assert callable(getattr(qmf_amd.Context, m))


def test_explain_reference_on_a_hand_computed_case():
    Y = np.array([[1.0], [2.0], [3.0]])
    rowptr, col, val = np.array([0, 0, 2]), np.array([0, 1]), np.array([1.0, 0.5])
    contrib, order = explain_reference(rowptr, col, val, Y, 1, 2, 2.0, 1.0)
    assert np.allclose(contrib, [3.0 / 7.0, 4.0 / 7.0], rtol=1e-15, atol=0)
    assert abs(contrib.sum() - 1.0) < 1e-15
    assert order.tolist() == [1, 0]
    assert explain_reference(rowptr, col, val, Y, 1, 2, 2.0, 1.0, topm=1)[1].tolist() == [1]
    # a row without signals: nothing to rank
    contrib, order = explain_reference(rowptr, col, val, Y, 0, 2, 2.0, 1.0)
    assert contrib.shape == (0,) and order.shape == (0,)
    # equal contributions rank by position: the same column twice with the same value
    contrib, order = explain_reference(np.array([0, 3]), np.array([1, 0, 1]),
                                       np.array([0.5, 1.0, 0.5]), Y, 0, 2, 2.0, 1.0)
    assert contrib[0] == contrib[2] and contrib[0] > contrib[1]
    assert order.tolist() == [0, 2, 1]
