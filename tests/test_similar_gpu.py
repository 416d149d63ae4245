"""Similar rows on the device (qmfx_similar / qmfx_factor_norms, csrc/recommend.hip) against
numpy.

Bar: exact.  dot(a, b) is the reference's double score bit for bit (pyoracle.test_scores), the
norm is the correctly rounded sqrt of the same unfused sum, the cosine is one rounded multiply
and one correctly rounded divide, and the order (score descending, then row index ascending)
is total, so every list is uniquely defined: neighbours, scores (bit for bit) and counts must
equal the numpy reference (test_similar.similar_reference), no tolerance.  Covers the norms
first (they also establish that the device's sqrt rounds as numpy's does), fp32 and fp64
contexts, k up to 256, both sides, both metrics, duplicate rows inside a tile and across
chunks, an exact cosine tie that is no dot tie, a zero row, the query's own row at tile and
chunk edges, chunks of several tiles, short lists, agreement with qmfx_recommend, query
batches, sharded contexts and the error returns.
"""
import functools

import numpy as np
import pytest

import qmf_amd
from test_similar import COSINE, DOT, norms_reference, similar_reference

pytestmark = pytest.mark.gpu


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("neighbours", "scores", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name


def _ctx(k, prec, side, F):
    """A context whose `side` holds F; the other side has one zero row."""
    c = qmf_amd.Context(k, prec)
    n = len(F)
    c.set_shape(*((n, 1) if side == 0 else (1, n)))
    c.set_factors(side, F)
    c.set_factors(1 - side, np.zeros((1, k)))
    return c


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("k", [16, 30, 130, 256])
def test_factor_norms_bit_for_bit(k, prec):
    rng = np.random.default_rng(k)
    n = 130
    F = rng.normal(0, 0.3, (n, k))
    F[5] = 0.0
    F[6] = 1e3
    F[9] = 1e-170           # the squares underflow to 0: the norm is 0.0
    F[10] = 1e-160          # the squares, and their sum, are subnormal doubles
    if prec == 32:          # the device stores fp32 (these two rows become zero rows)
        F = _f32(F)
    want = norms_reference(F)
    assert want[5] == 0.0 and want[9] == 0.0 and (prec == 32 or 0.0 < want[10] < 1e-150)
    for side in (0, 1):
        with _ctx(k, prec, side, F) as c:
            got = c.factor_norms(side)
            other = c.factor_norms(1 - side)
        assert got.dtype == np.float64 and np.array_equal(got, want), np.flatnonzero(got != want)
        assert other.tolist() == [0.0]


def _planted(rng, n, k, prec):
    F = rng.normal(0, 0.3, (n, k))
    F[7] = F[3]              # duplicates inside a tile ...
    F[n - 1] = F[3]          # ... and across chunks
    F[11] = 2.0 * F[3]       # an exact cosine tie that is no dot tie
    F[20] = 0.0              # a zero row
    return _f32(F) if prec == 32 else F


def _queries(rng, n, nq):
    """nq distinct rows in random order (the planted ones, the zero row and random others)
    plus two repeated ones (one of them once more where the length would be a multiple of the
    8 queries of a wave)."""
    fixed = np.array([3, 7, n - 1, 11, 20])
    rest = rng.choice(np.setdiff1d(np.arange(n), fixed), nq - len(fixed), replace=False)
    q = np.concatenate([fixed, rest])
    rng.shuffle(q)
    q = np.concatenate([q, q[[1, 0]]])
    if len(q) % 8 == 0:
        q = np.concatenate([q, q[:1]])
    return q.astype(np.int64)


@pytest.mark.parametrize("prec,k,side,n,nq,topn,metric,excl", [
    (64, 16, 1, 500, 40, 10, COSINE, True),
    (32, 30, 0, 777, 33, 7, COSINE, True),
    (64, 130, 1, 300, 20, 128, DOT, True),
    (32, 256, 1, 1000, 17, 1, COSINE, False),
    (64, 64, 1, 5000, 70, 50, COSINE, True),
])
def test_similar_matches_numpy(prec, k, side, n, nq, topn, metric, excl):
    rng = np.random.default_rng(k + n)
    F = _planted(rng, n, k, prec)
    q = _queries(rng, n, nq)
    assert len(q) % 8 != 0 and not np.all(np.diff(q) > 0)
    with _ctx(k, prec, side, F) as c:
        got = c.similar(side, q, topn, metric, excl)
    want = similar_reference(F, q, topn, metric, excl)
    _assert_equal(got, want)
    if metric == COSINE and topn >= 3 and excl:
        # row 3's two duplicates and its double (scaling by 2 is exact in the dot, the norm
        # and their product) have one and the same cosine, so the index orders them
        t = int(np.flatnonzero(q == 3)[0])
        assert got[0][t, :3].tolist() == [7, 11, n - 1]
        assert got[1][t, 0] == got[1][t, 1] == got[1][t, 2]


def test_similar_self_exclusion_at_tile_and_chunk_edges():
    rng = np.random.default_rng(12)
    n, k = 4099, 8
    F = rng.normal(0, 0.3, (n, k))
    q = np.array([0, 63, 64, 127, n - 1], dtype=np.int64)
    dup = np.array([2000, 1, 4000, 65, 300])      # each query's exact duplicate
    F[dup] = F[q]
    for metric in (COSINE, DOT):
        with _ctx(k, 64, 1, F) as c:
            excl = c.similar(1, q, 5, metric, True)
            incl = c.similar(1, q, 5, metric, False)
        _assert_equal(excl, similar_reference(F, q, 5, metric, True))
        _assert_equal(incl, similar_reference(F, q, 5, metric, False))
        assert not np.any(excl[0] == q[:, None])
        if metric == COSINE:    # nothing beats cosine 1; a dot product may
            assert excl[0][:, 0].tolist() == dup.tolist()
            assert incl[0][:, 0].tolist() == np.minimum(q, dup).tolist()
            assert incl[0][:, 1].tolist() == np.maximum(q, dup).tolist()


@functools.lru_cache(maxsize=None)
def _many_queries_case():
    """4,203 queries drawn from 50 rows over 8,000 rows: 132 query groups leave 25 chunks of 5
    tiles, so a workgroup carries thresholds and prunes from tile to tile, and the 50 query
    rows (spread over the matrix) fall into different chunks."""
    rng = np.random.default_rng(78)
    n, k = 8000, 8
    F = rng.normal(0, 0.3, (n, k))
    F[:, 0] = np.arange(n) / 6400.0      # later rows tend to score higher: many prunes
    F[4000:4100] = F[100]                # ties across tiles and chunks
    edge = np.array([0, 100, 4000, 4050, n - 1])
    base = np.sort(np.concatenate([edge, rng.choice(np.setdiff1d(np.arange(n), edge), 45,
                                                    replace=False)]))
    q = np.concatenate([rng.choice(base, 4200), [0, 100, 100]]).astype(np.int64)
    ref = {}
    for metric in (COSINE, DOT):
        ri, rs, rc = similar_reference(F, base, 128, metric, True)
        for a in (ri, rs, rc):
            a.setflags(write=False)
        ref[metric] = (ri, rs, rc)
    pos = np.searchsorted(base, q)
    for a in (F, q, pos):
        a.setflags(write=False)
    return n, k, F, q, pos, ref


@pytest.mark.parametrize("topn", [3, 128])
@pytest.mark.parametrize("metric", [COSINE, DOT])
def test_similar_chunks_of_several_tiles(metric, topn):
    n, k, F, q, pos, ref = _many_queries_case()
    with _ctx(k, 64, 1, F) as c:
        got = c.similar(1, q, topn, metric, True)
    ri, rs, rc = ref[metric]    # the top 128 in rank order: the top 3 are its first 3
    want = (ri[pos][:, :topn], rs[pos][:, :topn], np.minimum(rc[pos], topn).astype(np.int32))
    _assert_equal(got, want)


def test_similar_short_lists():
    rng = np.random.default_rng(5)
    n, k, topn = 50, 12, 128
    F = rng.normal(0, 0.3, (n, k))
    q = np.array([0, 49, 17], dtype=np.int64)
    with _ctx(k, 64, 0, F) as c:
        got = c.similar(0, q, topn, COSINE, True)
        got_all = c.similar(0, q, topn, COSINE, False)
    _assert_equal(got, similar_reference(F, q, topn, COSINE, True))
    assert got[2].tolist() == [49] * 3
    assert np.all(got[0][:, 49:] == -1) and np.all(got[1][:, 49:] == 0.0)
    _assert_equal(got_all, similar_reference(F, q, topn, COSINE, False))
    assert got_all[2].tolist() == [50] * 3
    # a side of one row: nothing is left once the query is excluded
    with _ctx(k, 64, 1, F[:1]) as c:
        nb, sc, cnt = c.similar(1, np.array([0]), 4, COSINE, True)
        assert cnt.tolist() == [0] and nb.tolist() == [[-1] * 4] and sc.tolist() == [[0.0] * 4]
        nb, sc, cnt = c.similar(1, np.array([0]), 4, DOT, False)
        assert cnt.tolist() == [1] and nb.tolist() == [[0, -1, -1, -1]]


@pytest.mark.parametrize("prec", [32, 64])
def test_similar_dot_equals_recommend_all(prec):
    """Side 1, dot, the query kept: qmfx_recommend(ALL) on a context whose user factors are
    the query item rows gives the same lists bit for bit."""
    rng = np.random.default_rng(31)
    n, k, topn = 900, 48, 25
    F = _planted(rng, n, k, prec)
    q = _queries(rng, n, 45)
    with _ctx(k, prec, 1, F) as c:
        got = c.similar(1, q, topn, DOT, False)
    with qmf_amd.Context(k, prec) as c:
        c.set_shape(len(q), n)
        c.set_factors(0, F[q])
        c.set_factors(1, F)
        rec = c.recommend(np.arange(len(q), dtype=np.int64), topn)
    _assert_equal(got, rec)


@pytest.mark.parametrize("batch_groups", ["1", "3"])
def test_similar_query_batches_equal_one_launch(batch_groups, monkeypatch):
    rng = np.random.default_rng(9)
    n, k, topn = 900, 48, 20
    F = _planted(rng, n, k, 64)
    q = rng.choice(n, 150, replace=False).astype(np.int64)
    out = []
    for env in (None, batch_groups):
        if env:
            monkeypatch.setenv("QMFX_EVAL_BATCH_GROUPS", env)
        with _ctx(k, 64, 1, F) as c:
            out.append(c.similar(1, q, topn, COSINE, True))
    _assert_equal(out[1], out[0])
    _assert_equal(out[0], similar_reference(F, q, topn, COSINE, True))


def test_similar_on_sharded_contexts():
    """Three ranks without a communicator: the factors are full replicas, so each rank gives
    the unsharded answer for rows outside its own range."""
    rng = np.random.default_rng(3)
    nu, ni, k, topn = 300, 400, 32, 12
    U, I = rng.normal(0, 0.3, (nu, k)), rng.normal(0, 0.3, (ni, k))
    pu = np.concatenate([np.arange(nu), rng.integers(0, nu, ni + 5000)]).astype(np.int64)
    pi = np.concatenate([rng.integers(0, ni, nu), np.arange(ni),
                         rng.integers(0, ni, 5000)]).astype(np.int64)

    def ctx():
        c = qmf_amd.Context(k, 64)
        c.group_signals(pu, pi, np.ones(len(pu)))
        c.set_factors(0, U)
        c.set_factors(1, I)
        return c

    want = {0: similar_reference(U, np.arange(nu), topn, COSINE, True),
            1: similar_reference(I, np.arange(ni), topn, COSINE, True)}
    with ctx() as c:
        rowptr = {s: c.download_csr(s)[0] for s in (0, 1)}
    for rank in range(3):
        with ctx() as c:
            c.dist_init(rank, 3, None)
            for side, n in ((0, nu), (1, ni)):
                lo, hi = qmf_amd.partition_rows(rowptr[side], 3, rank)
                outside = np.setdiff1d(np.arange(n), np.arange(lo, hi)).astype(np.int64)
                assert 0 < len(outside) < n
                got = c.similar(side, outside, topn, COSINE, True)
                _assert_equal(got, tuple(w[outside] for w in want[side]))


def test_similar_errors_leave_the_context_usable():
    rng = np.random.default_rng(1)
    n, k = 100, 8
    F = rng.normal(0, 0.3, (n, k))
    q = np.arange(5, dtype=np.int64)
    want = similar_reference(F, q, 5, COSINE, True)
    with _ctx(k, 64, 1, F) as c:
        # side, topn (both ends), metric, a row index out of range (both ends; side 0 has one row)
        for args in [(2, q, 5), (-1, q, 5), (1, q, 0), (1, q, 129), (1, q, 5, 2), (1, q, 5, -1),
                     (1, np.array([n]), 5), (1, np.array([0, -1]), 5), (0, np.array([1]), 5)]:
            with pytest.raises(qmf_amd.QmfxError) as e:
                c.similar(*args)
            assert str(e.value).split(": ", 1)[1].strip(), args
            _assert_equal(c.similar(1, q, 5), want)
        with pytest.raises(qmf_amd.QmfxError):
            c.factor_norms(2)
        nb, sc, cnt = c.similar(1, np.array([], np.int64), 5)
        assert nb.shape == (0, 5) and sc.shape == (0, 5) and cnt.shape == (0,)
        assert nb.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int32
        _assert_equal(c.similar(1, q, 5), want)
    # no factors on the context
    with qmf_amd.Context(k, 64) as c:
        for call in (lambda: c.similar(1, q, 5), lambda: c.factor_norms(1)):
            with pytest.raises(qmf_amd.QmfxError) as e:
                call()
            assert str(e.value).split(": ", 1)[1].strip()
    # nfactors > 256: qmfx_similar refuses it, but no such context can be made to ask
    with pytest.raises(qmf_amd.QmfxError):
        qmf_amd.Context(257, 64)


def test_similar_is_counted_in_the_solve_stats():
    rng = np.random.default_rng(2)
    n, k = 300, 16
    F = rng.normal(0, 0.3, (n, k))
    with _ctx(k, 64, 1, F) as c:
        c.reset_stats()
        c.similar(1, np.arange(10), 5)
        st = c.solve_stats()
    assert st["launches"] == 1 and st["ms"] > 0 and st["flops"] == 2.0 * 10 * n * k
