"""The serving calls on one context, one after the other, at sizes that grow and shrink.

recommend, similar, fold-in and explanations share device scratch that is grown on demand and
kept: the top-N selection's buffers (all three selecting calls), the uploaded foreign CSR
(fold-in and wals_explain_rows) and the row norms (either side).  A buffer that is reused at a
smaller size, or regrown behind a stale recorded size, would hand a kernel the wrong memory, and
every other test uses a fresh context per call shape.  Here ten calls run on one context per
(k, precision): tiny first, then the largest shape of each buffer, then smaller again, each
checked against the reference its own test file uses (exact where that is exact, 1e-9 / 1e-4
where it is not).  The plan queried after wals_explain_rows must still be the last fold-in's,
and a repeated call must return the bits of its first run.
"""
import numpy as np
import pytest

import pyoracle as po
import qmf_amd
from test_explain import explain_reference
from test_explain_gpu import check_selection
from test_foldin import ALPHA, LAM, LENGTHS, NFIXED, bars, foldin_case
from test_foldin_gpu import check_plan, check_rows, max_ntn
from test_recommend import topn_reference
from test_similar import COSINE, similar_reference

pytestmark = pytest.mark.gpu

NU, NI = 40, NFIXED
SIGNALS = 1


def _equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g,
                              w.view(np.int64) if w.dtype == np.float64 else w)


@pytest.mark.parametrize("k,precision", [(17, 32), (64, 64)])
def test_calls_of_growing_and_shrinking_sizes_share_one_context(k, precision):
    rowptr, col, val, I = foldin_case(k, precision)
    nrows = len(LENGTHS)
    rng = np.random.default_rng(1000 + k)
    U = rng.normal(0, 0.3, (NU, k))
    if precision == 32:
        U = U.astype(np.float32).astype(np.float64)
    # the users' own signals: 1..30 distinct ascending items each
    ulen = rng.integers(1, 31, NU)
    urp = np.concatenate([[0], np.cumsum(ulen)]).astype(np.int64)
    seen = [np.sort(rng.choice(NI, n, replace=False)) for n in ulen]
    ucol = np.concatenate(seen).astype(np.int32)
    mx = max_ntn(k, precision)
    fbar = bars(precision)[0]
    first3 = np.array([5, 0, 39], np.int64)
    everyone = rng.permutation(NU).astype(np.int64)
    # the explained rows (n = 1, 17, 64, 128, 300) as a CSR of their own, two targets each
    erows = [LENGTHS.index(n) for n in (1, 17, 64, 128, 300)]
    erp = np.concatenate([[0], np.cumsum([LENGTHS[r] for r in erows])]).astype(np.int64)
    ecol = np.concatenate([col[rowptr[r]:rowptr[r + 1]] for r in erows])
    eval_ = np.concatenate([val[rowptr[r]:rowptr[r + 1]] for r in erows])
    eqptr = np.arange(0, 2 * len(erows) + 1, 2, dtype=np.int64)
    etargets = rng.integers(0, NI, 2 * len(erows)).astype(np.int64)

    with qmf_amd.Context(k, precision) as c:
        c.set_shape(NU, NI)
        c.upload_csr(0, urp, ucol, np.ones(len(ucol)))
        c.set_factors(0, U)
        c.set_factors(1, I)
        rec1 = c.recommend(first3, 1)
        sim1 = c.similar(1, np.arange(NU, dtype=np.int64) * 7, 128, COSINE)
        rfi = c.recommend_fold_in(rowptr, col, val, ALPHA, LAM, 10)
        check_plan(c, rowptr, mx)
        rec2 = c.recommend(everyone, 128, SIGNALS)
        sim2 = c.similar(0, np.array([38, 2], np.int64), 3, COSINE)
        F3, loss3, piv3 = c.wals_fold_in(0, rowptr[:4], col[:rowptr[3]], val[:rowptr[3]], ALPHA, LAM)
        ex = c.wals_explain_rows(0, erp, ecol, eval_, eqptr, etargets, ALPHA, LAM, 4, full=True)
        # the plan is still the three-row fold-in's
        check_plan(c, rowptr[:4], mx)
        Fall, lossall, pivall = c.wals_fold_in(0, rowptr, col, val, ALPHA, LAM)
        check_plan(c, rowptr, mx)
        rec3 = c.recommend(first3, 1)

    _equal(rec1, topn_reference(po.test_scores(U, I, first3, None), 1))
    _equal(rec3, rec1)
    _equal(rec2, topn_reference(po.test_scores(U, I, everyone, None), 128,
                                [seen[u] for u in everyone]))
    _equal(sim1, similar_reference(I, np.arange(NU) * 7, 128, COSINE, True))
    _equal(sim2, similar_reference(U, [38, 2], 3, COSINE, True))

    items, scores, counts, F = rfi
    check_rows("shared k=%d recommend_fold_in" % k, F, lossall, rowptr, col, val, I, precision)
    rows_seen = [np.unique(col[rowptr[r]:rowptr[r + 1]]) for r in range(nrows)]
    _equal((items, scores, counts),
           topn_reference(po.test_scores(F, I, np.arange(nrows), None), 10, rows_seen))
    check_rows("shared k=%d three rows" % k, F3, loss3, rowptr[:4], col[:rowptr[3]],
               val[:rowptr[3]], I, precision)
    _equal((Fall,), (F,))  # the rows recommended from are the rows the later fold-in returns
    assert piv3 == 0 and pivall == 0

    allv, allptr = ex[5]
    totals = ex[4]
    verr = terr = 0.0
    for q in range(len(erows)):
        for p in range(eqptr[q], eqptr[q + 1]):
            want = explain_reference(erp, ecol, eval_, I, q, int(etargets[p]), ALPHA, LAM)[0]
            got = allv[allptr[p]:allptr[p + 1]]
            assert got.shape == want.shape
            verr = max(verr, np.max(np.abs(got - want)) / np.max(np.abs(want)))
            terr = max(terr, abs(totals[p] - want.sum()) / np.abs(want).sum())
    print("SHARED explain k=%d p=%d verr=%.3g terr=%.3g (bar %.1g)" % (k, precision, verr, terr, fbar))
    assert verr <= fbar and terr <= fbar
    check_selection("shared k=%d" % k, ex, erp, ecol, np.arange(len(erows)), eqptr, 4)
