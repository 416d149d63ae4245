"""The data the device makes for itself, bit for bit: qmfx_gen_synthetic, qmfx_gen_synthetic_zipf
(qmf_amd/csrc/data.hip and the driver at the end of api_signals.cpp) and qmfx_fill_uniform against
the numpy restatements of tests/helpers.py (synth_reference, zipf_reference, fill_reference),
which tests/test_synth.py anchors on plain Python integers.  Every number bench.py and
tools/bench_*.py publish is measured on this data.

Every comparison is exact (np.array_equal; factors by their bit patterns).  The one margin is the
Zipf rank's, applied to the reference alone: the rank goes through exp/log/pow, so
helpers.zipf_draws counts the draws whose x lies within 1e-12 (relative) of an integer and, for
s ≠ 1, those whose ⌊x⌋ moves when the power's base moves by ± 2⁻⁵² (one rounding of `·u01 + 1`,
which the device may fuse; for s > 1 the base is about 1 − u01 and cancels, so that rounding can
exceed 1e-12 of x).  Every Zipf case first asserts that its own reference has no such draw
(test_synth.py asserts the same without a GPU); then the comparison is exact too.

Each generator case runs at precision 32 and 64 (the values 1..5 are exact in both) and asserts:
the returned nnz = qmfx_get_shape's nnz = the reference's m; rowptr, col and val of both sides
equal the reference's; row_classes of each side sums to its row count; qmfx_get_ids fails (no
id table).

Where each edge is covered (helpers.SYNTH_CASES / ZIPF_CASES, by test id):
  rowptr grid edges (nrows + 1 entries, 256 a block) .. test_uniform[users1 .. users512] against
      37 items, [items1 .. items512] against 37 users: row counts 1, 2, 255, 256, 257, 511, 512
  mostly empty rows .................................... [empty_rows] 5000 × 7, 40 draws
  single row / column .................................. [one_user] 1 × 300, [one_item] 300 × 1
  radix end_bit ........................................ [space_pow2] 64·128 = 2¹³,
      [space_pow2_minus1] 63·65 = 2¹² − 1, [space_pow2_plus1] 17·241 = 2¹² + 1,
      [space_1p5_pow2] 83·74 = 1.4995·2¹² (a third of the keys have the top bit set)
  key space beyond 2³² ................................. [space_gt32_users] (2²⁰ + 3) × 5003,
      [space_gt32_items] 5003 × (2²⁰ + 3), 20 000 draws each
  collisions ........................................... [collisions] 31 × 33, nnz = space / 2
      (m = 0.78 nnz); test_too_many_draws_is_refused: space / 2 + 1 fails, the context goes on,
      on that shape and on another
  seeds ................................................ [seed0], [seed_max] 2⁶⁴ − 1, [seed_wrap]
      (seed·31 + 7 wraps)
  several datasets in one context ...................... test_datasets_in_a_row_in_one_context:
      31 × 33, 83 × 74, 31 × 33 under a new seed, 257 × 37, a Zipf 83 × 74, 31 × 33 again
  Zipf ................................................. test_zipf[items{1,2,1000,5003}-s{0.5,1,2,8}]:
      pa = 0 (nitems = 1), 1, 619, 3093 (the golden-ratio values); at nitems ≤ 2, 2000 draws over
      at most 600 pairs; s = 8 sends 99.2 % of the draws to rank 0 (one item row holds every user)
  fill_uniform ......................................... test_fill_uniform[k-precision], k in 1, 16,
      30, 64, 100, 256: both sides at 1, 255, 256 (n·kp a multiple of 256) and 257 rows, bounds
      0.01 and 0.5, |x| ≤ bound, a second seed differs, the other side stays bit-identical
  the benchmark's data ................................. test_bench_recipe[c2 / c3 / c4]:
      bench.CONFIGS' seed and density with the dimensions divided by 20 / 200 / 20 and bench.py's
      fills at bound 0.01: the item side with seed + 100 for the WALS configs c2 and c3, the user
      side with seed + 100 and the item side with seed + 101 for the BPR config c4
The factors' padding columns (kp − k zeros a row) cannot be read through the C ABI;
tests/test_bpr_gpu.py's eval test shows that they do not enter a result.

Measured on an MI355X: 108 cases in 2.4 s, all passing; the slowest is 0.57 s
(test_uniform[users1-32], the first to load the library), then test_uniform[space_gt32_users-32] at
0.15 s and test_fill_uniform[16-32] at 0.09 s.

Bug found: a second dataset generated in a context that already held one came out wrong when
it had more draws than the one before (31 × 33 / 511 draws, then 83 × 74 / 2047 draws in the same
context: success with nnz = 0 and empty CSRs; a later 257 × 37 / 2377 draws never returned).
sort_unique_keys and sort_keys took hipcub's temporary storage from the stream-ordered pool; they
now allocate it as ingest.hip does.  test_datasets_in_a_row_in_one_context and the second half of
test_too_many_draws_is_refused reproduce it on the old library.

Single-line mutants of the library that change a value only, none committed, each built and run
once, before the two repeated-generation tests and the c4 recipe were added (failing cases of
this module's then 104; failing cases of the 3 older tests that call these
functions, test_heavy_gpu::test_zipf_generator_shape and
test_bpr_kernels_gpu::test_bpr_eval_ignores_padding_after_fill_uniform[32, 64]; test_bench_gpu was
not run against the mutants):
  the sort's end_bit one smaller ................................. 86 new, 1 old (the Zipf shape test)
  value seed seed·31 + 7 → seed·31 ............................... 92 new, 0 old
  user_major of the item-side values flipped ..................... 80 new, 0 old
  % 5 → % 4 ....................................................... 92 new, 0 old
  fill_uniform hashes r·kp + c .................................... 6 new (k = 1, 30, 100: kp ≠ k), 0 old
  Zipf pb forced to 0 ............................................. 20 new, 0 old
  s ≠ 1 branch raises to e instead of 1/e ......................... 12 new (s = 0.5 and 8 at
      nitems ≥ 2; at s = 2, e = 1/e = −1), 0 old
"""
import numpy as np
import pytest

import bench
import qmf_amd
from helpers import (SYNTH_CASES, ZIPF_CASES, fill_reference, synth_reference, zipf_reference)

pytestmark = pytest.mark.gpu

PRECISIONS = (32, 64)


def check_dataset(c, nnz, ref, nusers, nitems):
    """The context's CSRs equal the reference (m, ucsr, icsr) exactly; see the module docstring."""
    m, ucsr, icsr = ref
    assert nnz == m
    assert c.shape() == (nusers, nitems, m)
    for side, want, nrows in ((0, ucsr, nusers), (1, icsr, nitems)):
        rowptr, col, val = c.download_csr(side)
        assert rowptr.shape == want[0].shape and np.array_equal(rowptr, want[0]), side
        assert np.array_equal(col, want[1]), side
        assert np.array_equal(val, want[2]), side
        rc = c.row_classes(side)
        assert sum(rc["whitened"]) + rc["direct"] + rc["heavy"] == nrows, (side, rc)
        with pytest.raises(qmf_amd.QmfxError, match="no id table"):
            c.ids(side)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SYNTH_CASES))
def test_uniform(name, precision):
    nusers, nitems, nnz, seed = SYNTH_CASES[name]
    ref = synth_reference(nusers, nitems, nnz, seed)
    with qmf_amd.Context(16, precision) as c:
        got = c.gen_synthetic(nusers, nitems, nnz, seed)
        check_dataset(c, got, ref, nusers, nitems)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(ZIPF_CASES))
def test_zipf(name, precision):
    nusers, nitems, ndraws, seed, s = ZIPF_CASES[name]
    *ref, ambiguous = zipf_reference(nusers, nitems, ndraws, seed, s)
    assert ambiguous == 0  # the reference is exact: no draw within 1e-12 of an integer rank
    with qmf_amd.Context(16, precision) as c:
        got = c.gen_synthetic_zipf(nusers, nitems, ndraws, seed, s)
        check_dataset(c, got, ref, nusers, nitems)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_too_many_draws_is_refused(precision):
    """nnz = space / 2 + 1 is an error; the context then takes the largest accepted nnz, on the
    same shape and, after a second refusal, on another: each equals its reference."""
    nusers, nitems, nnz, seed = SYNTH_CASES["collisions"]
    assert nnz == nusers * nitems // 2
    with qmf_amd.Context(16, precision) as c:
        with pytest.raises(qmf_amd.QmfxError, match="nnz too large"):
            c.gen_synthetic(nusers, nitems, nnz + 1, seed)
        got = c.gen_synthetic(nusers, nitems, nnz, seed)
        check_dataset(c, got, synth_reference(nusers, nitems, nnz, seed), nusers, nitems)
        with pytest.raises(qmf_amd.QmfxError, match="nnz too large"):
            c.gen_synthetic(nusers, nitems, nnz + 1, seed)
        other = SYNTH_CASES["space_1p5_pow2"]
        got = c.gen_synthetic(*other)
        check_dataset(c, got, synth_reference(*other), other[0], other[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_datasets_in_a_row_in_one_context(precision):
    """Datasets one after the other in one context, each with more draws than the one before
    except the returns to the first shape (under a new seed, then under its own): uniform,
    uniform, the first shape again, a Zipf dataset, the first once more.  Each equals its own
    reference and has no id table."""
    a = SYNTH_CASES["collisions"]
    b = SYNTH_CASES["space_1p5_pow2"]
    a2 = a[:3] + (a[3] + 1000,)
    d = SYNTH_CASES["users257"]
    bz = (b[0], b[1], 3000, 77, 1.0)
    assert a[2] < b[2] < d[2] < bz[2]
    with qmf_amd.Context(16, precision) as c:
        for case in (a, b, a2, d):
            got = c.gen_synthetic(*case)
            check_dataset(c, got, synth_reference(*case), case[0], case[1])
        *ref, ambiguous = zipf_reference(*bz)
        assert ambiguous == 0
        got = c.gen_synthetic_zipf(*bz)
        check_dataset(c, got, ref, bz[0], bz[1])
        got = c.gen_synthetic(*a)
        check_dataset(c, got, synth_reference(*a), a[0], a[1])
    assert not np.array_equal(synth_reference(*a)[1][1], synth_reference(*a2)[1][1])


# ---- qmfx_fill_uniform -------------------------------------------------------------------------
FILL_SHAPES = ((1, 255), (255, 257), (257, 256), (256, 1))  # (nusers, nitems)
FILL_BOUNDS = (0.01, 0.5)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [1, 16, 30, 64, 100, 256])
def test_fill_uniform(k, precision):
    """c.factors(side) after qmfx_fill_uniform equals fill_reference bit for bit, on both sides,
    at every row count of FILL_SHAPES and both bounds; see the module docstring."""
    kp = (k + 15) // 16 * 16
    assert any(n * kp % 256 == 0 for s in FILL_SHAPES for n in s)
    with qmf_amd.Context(k, precision) as c:
        for j, shape in enumerate(FILL_SHAPES):
            c.set_shape(*shape)
            for bound in FILL_BOUNDS:
                seeds = (1000 * k + 10 * j, 1000 * k + 10 * j + 1)
                want = [fill_reference(shape[side], k, bound, seeds[side], precision) for side in (0, 1)]
                for side in (0, 1):
                    c.fill_uniform(side, bound, seeds[side])
                for side in (0, 1):
                    got = c.factors(side)
                    assert np.array_equal(bits(got), bits(want[side])), (shape, bound, side)
                    assert np.abs(got).max() <= bound
                # another seed on one side: that side changes, the other keeps every bit
                for side in (0, 1):
                    other = bits(c.factors(1 - side))
                    c.fill_uniform(side, bound, seeds[side] + 5)
                    got = c.factors(side)
                    assert np.array_equal(bits(got), bits(fill_reference(shape[side], k, bound,
                                                                        seeds[side] + 5, precision)))
                    assert not np.array_equal(bits(got), bits(want[side]))
                    assert np.array_equal(bits(c.factors(1 - side)), other)


# ---- the benchmark's own recipe ----------------------------------------------------------------
BENCH_SCALE = {"c2": 20, "c3": 200, "c4": 20}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config", sorted(BENCH_SCALE))
def test_bench_recipe(config, precision):
    """bench.py's dataset and initial factors, scaled down: bench.CONFIGS[config]'s seed, factor
    count and density (nnz / (nusers·nitems)) with both dimensions divided by BENCH_SCALE,
    gen_synthetic(seed), then the fills of the config's path in bench.py: fill_uniform(1, 0.01,
    seed + 100) for a WALS config, fill_uniform(0, 0.01, seed + 100) and fill_uniform(1, 0.01,
    seed + 101) for a BPR one."""
    nu, ni, nnz, k, seed = bench.CONFIGS[config]
    d = BENCH_SCALE[config]
    assert nu % d == 0 and ni % d == 0 and nnz % (d * d) == 0 and config not in bench.ZIPF
    nu, ni, nnz = nu // d, ni // d, nnz // (d * d)
    fills = {0: seed + 100, 1: seed + 101} if config in bench.BPR_CONFIGS else {1: seed + 100}
    with qmf_amd.Context(k, precision) as c:
        got = c.gen_synthetic(nu, ni, nnz, seed)
        check_dataset(c, got, synth_reference(nu, ni, nnz, seed), nu, ni)
        for side, fseed in fills.items():
            c.fill_uniform(side, 0.01, fseed)
        for side, fseed in fills.items():
            want = fill_reference((nu, ni)[side], k, 0.01, fseed, precision)
            assert np.array_equal(bits(c.factors(side)), bits(want)), side
