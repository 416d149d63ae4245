"""CPU anchor of tests/test_synth_gpu.py: the numpy restatements in tests/helpers.py of the
device's synthetic data generators (qmf_amd/csrc/data.hip, qmfx_gen_synthetic[_zipf]) and of
qmfx_fill_uniform are checked here against the same recipes written out in plain Python
integers, one draw at a time, and the case tables the GPU module runs are checked for the
properties each case is there for.  Nothing here touches the device."""
import math

import numpy as np
import pytest

from helpers import (M64, ROW_EDGES, SEED_MAX, SEED_WRAP, SYNTH_CASES, ZIPF_CASES, ZIPF_MARGIN,
                     ZIPF_S, fill_reference, mix64, mix64_np, mulhi64_np, synth_reference,
                     zipf_ambiguous, zipf_draws, zipf_permutation, zipf_reference)

EXTREMES = [0, 1, 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1,
            1 << 63, M64 - 1, M64, SEED_WRAP, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]


def inputs():
    rng = np.random.default_rng(64)
    return EXTREMES + [int(x) for x in rng.integers(0, 1 << 64, 2000, dtype=np.uint64)]


def test_mix64_np_equals_python_ints():
    xs = inputs()
    got = mix64_np(np.array(xs, np.uint64))
    assert got.dtype == np.uint64
    assert got.tolist() == [mix64(x) for x in xs]
    # the composition the generators use, at the extreme seeds
    for seed in (0, SEED_MAX, SEED_WRAP):
        got = mix64_np(np.uint64(seed) ^ mix64_np(np.array(xs, np.uint64)))
        assert got.tolist() == [mix64(seed ^ mix64(x)) for x in xs]


def test_mulhi64_np_equals_python_ints():
    xs = inputs()
    a = np.array(xs, np.uint64)
    spaces = EXTREMES + [10 ** 13, ((1 << 20) + 3) * 5003, 83 * 74, 1 << 13, 3 << 31]
    for b in spaces:
        assert mulhi64_np(a, b).tolist() == [(x * b) >> 64 for x in xs], b


def test_value_seed_wraps():
    """seed·31 + 7 is taken mod 2⁶⁴; SEED_WRAP and SEED_MAX are seeds for which that matters."""
    for seed in (SEED_WRAP, SEED_MAX):
        assert seed * 31 + 7 > M64
    assert 0 * 31 + 7 == 7


# ---- the generators in Python integers: a dict {(u, i): value} -------------------------------
def value_py(nitems, seed, u, i):
    return 1 + mix64(((seed * 31 + 7) & M64) ^ (u * nitems + i)) % 5


def synth_py(nusers, nitems, nnz, seed):
    space = nusers * nitems
    keys = {(mix64(seed ^ mix64(i)) * space) >> 64 for i in range(nnz)}
    return {(k // nitems, k % nitems): value_py(nitems, seed, k // nitems, k % nitems) for k in keys}


def zipf_py(nusers, nitems, ndraws, seed, s):
    """synth_keys_zipf_kernel and launch_synth_keys_zipf, one draw at a time, with the math
    module's exp/log/pow (not numpy's)."""
    pa = int(float(nitems) * 0.6180339887498949) | 1
    if nitems <= 1:
        pa = 1
    while nitems > 1 and math.gcd(pa, nitems) != 1:
        pa += 2
    pa %= max(nitems, 1)
    pb = mix64(seed ^ 0x7A1F) % max(nitems, 1)
    top = float(nitems) + 1.0
    out = {}
    for d in range(ndraws):
        h1 = mix64(seed ^ mix64(d))
        h2 = mix64(h1 ^ 0x2545F4914F6CDD1D)
        u = (h1 * nusers) >> 64
        u01 = float(h2 >> 11) * (1.0 / 9007199254740992.0)
        if abs(s - 1.0) < 1e-12:
            x = math.exp(u01 * math.log(top))
        else:
            e = 1.0 - s
            x = math.pow((math.pow(top, e) - 1.0) * u01 + 1.0, 1.0 / e)
        r = int(x) - 1 if x >= 1.0 else 0
        r = min(r, nitems - 1)
        it = (pa * r + pb) % nitems
        out[(u, it)] = value_py(nitems, seed, u, it)
    return out


def triples(csr):
    rowptr, col, val = csr
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return rows, col.astype(np.int64), val


def check_pair(ucsr, icsr, nusers, nitems, want=None):
    """Both orientations are well-formed CSRs (rowptr from 0 to m, columns ascending within a
    row and in range) of the same triples; `want`, a {(u, i): value}, equals them."""
    m = len(ucsr[1])
    for (rowptr, col, val), nrows, ncols in ((ucsr, nusers, nitems), (icsr, nitems, nusers)):
        assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
        assert len(rowptr) == nrows + 1 and rowptr[0] == 0 and rowptr[-1] == m
        assert len(col) == len(val) == m and np.all(np.diff(rowptr) >= 0)
        assert col.min() >= 0 and col.max() < ncols
        rows = np.repeat(np.arange(nrows), np.diff(rowptr))
        assert np.all(np.diff(rows * ncols + col.astype(np.int64)) > 0)  # sorted, distinct
        assert set(np.unique(val).tolist()) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    u, i, v = triples(ucsr)
    i2, u2, v2 = triples(icsr)
    o = np.lexsort((i2, u2))
    assert np.array_equal(u, u2[o]) and np.array_equal(i, i2[o]) and np.array_equal(v, v2[o])
    if want is not None:
        assert dict(zip(zip(u.tolist(), i.tolist()), v.tolist())) == want


SMALL = ("users1", "users2", "items1", "items257", "empty_rows", "one_item", "one_user",
         "space_pow2", "space_pow2_minus1", "space_pow2_plus1", "space_1p5_pow2", "collisions",
         "seed0", "seed_max", "seed_wrap", "space_gt32_users", "space_gt32_items")


@pytest.mark.parametrize("name", SMALL)
def test_synth_reference_equals_python_ints(name):
    nusers, nitems, nnz, seed = SYNTH_CASES[name]
    m, ucsr, icsr = synth_reference(nusers, nitems, nnz, seed)
    want = synth_py(nusers, nitems, nnz, seed)
    assert m == len(want)
    check_pair(ucsr, icsr, nusers, nitems, want)


@pytest.mark.parametrize("name", sorted(SYNTH_CASES))
def test_synth_cases_are_consistent(name):
    """Every uniform case: both orientations describe the same triples, m ≤ nnz with equality
    exactly when no two draws collide, and nnz ≤ space / 2 (the call accepts it)."""
    nusers, nitems, nnz, seed = SYNTH_CASES[name]
    space = nusers * nitems
    assert 0 < nnz <= space // 2
    m, ucsr, icsr = synth_reference(nusers, nitems, nnz, seed)
    check_pair(ucsr, icsr, nusers, nitems)
    keys = [(mix64(seed ^ mix64(i)) * space) >> 64 for i in range(min(nnz, 3000))]
    assert all(0 <= k < space for k in keys)
    if nnz <= 3000:
        assert m == len(set(keys)) <= nnz
        assert (m == nnz) == (len(set(keys)) == len(keys))


def test_synth_cases_hold_their_edges():
    """The properties the GPU cases are there for, on the reference."""
    for side, tag in ((0, "users"), (1, "items")):
        assert [SYNTH_CASES["%s%d" % (tag, n)][side] for n in ROW_EDGES] == list(ROW_EDGES)
    # mostly empty rows: leading, trailing and interior empty user rows, long item rows
    nusers, nitems, nnz, seed = SYNTH_CASES["empty_rows"]
    m, (urp, _, _), (irp, _, _) = synth_reference(nusers, nitems, nnz, seed)
    ulen = np.diff(urp)
    full = np.nonzero(ulen)[0]
    assert full[0] > 0 and full[-1] < nusers - 1 and np.any(np.diff(full) > 1)
    assert np.diff(irp).max() >= 5
    assert SYNTH_CASES["one_item"][1] == 1 and SYNTH_CASES["one_user"][0] == 1
    # radix end_bit: the four spaces about a power of two; keys with the top bit set are common
    sp = {n: SYNTH_CASES[n][0] * SYNTH_CASES[n][1] for n in SYNTH_CASES}
    assert sp["space_pow2"] == 1 << 13 and sp["space_pow2_minus1"] == (1 << 12) - 1
    assert sp["space_pow2_plus1"] == (1 << 12) + 1
    assert 1.45 < sp["space_1p5_pow2"] / (1 << 12) < 1.55
    for n in ("space_pow2_minus1", "space_pow2_plus1", "space_1p5_pow2"):
        assert math.gcd(SYNTH_CASES[n][0], SYNTH_CASES[n][1]) == 1
    for name, side in (("space_1p5_pow2", 0), ("space_pow2_minus1", 0)):
        nusers, nitems, nnz, seed = SYNTH_CASES[name]
        m, ucsr, icsr = synth_reference(nusers, nitems, nnz, seed)
        top = 1 << (sp[name].bit_length() - 1)
        for csr, ncols in ((ucsr, nitems), (icsr, nusers)):
            r, c, _ = triples(csr)
            assert np.count_nonzero(r * ncols + c >= top) > m // 5  # one bit fewer reorders these
    for n in ("space_gt32_users", "space_gt32_items"):
        assert sp[n] > 1 << 32
    assert SYNTH_CASES["space_gt32_users"][0] > 1 << 20 and SYNTH_CASES["space_gt32_items"][1] > 1 << 20
    # collisions: nnz is the most the call takes and a fifth of the draws repeat
    nusers, nitems, nnz, seed = SYNTH_CASES["collisions"]
    assert nnz == nusers * nitems // 2
    assert synth_reference(nusers, nitems, nnz, seed)[0] < 0.85 * nnz
    assert {SYNTH_CASES[n][3] for n in ("seed0", "seed_max", "seed_wrap")} == {0, SEED_MAX, SEED_WRAP}
    # the three seed cases differ in nothing else, and give three different datasets
    a, b, c = (synth_reference(*SYNTH_CASES[n]) for n in ("seed0", "seed_max", "seed_wrap"))
    assert not np.array_equal(a[1][1][:1000], b[1][1][:1000])
    assert not np.array_equal(b[1][1][:1000], c[1][1][:1000])


# ---- Zipf --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ZIPF_CASES))
def test_zipf_cases_are_exact_and_consistent(name):
    """No draw of a Zipf case in use is ambiguous (so the device must match the reference
    exactly), pa is coprime to nitems, both orientations describe the same triples."""
    nusers, nitems, ndraws, seed, s = ZIPF_CASES[name]
    m, ucsr, icsr, ambiguous = zipf_reference(nusers, nitems, ndraws, seed, s)
    assert ambiguous == 0
    pa, pb = zipf_permutation(nitems, seed)
    assert 0 <= pa < max(nitems, 2) and 0 <= pb < nitems
    assert math.gcd(pa, nitems) == 1  # gcd(0, 1) = 1: the nitems = 1 case
    assert sorted((pa * r + pb) % nitems for r in range(nitems)) == list(range(nitems))
    assert 0 < m <= ndraws
    check_pair(ucsr, icsr, nusers, nitems)


@pytest.mark.parametrize("name", sorted(ZIPF_CASES))
def test_zipf_reference_equals_python_ints(name):
    """The vectorised reference against the draw-by-draw one, which takes exp/log/pow from the
    math module: with no ambiguous draw the two libraries' last bits cannot matter."""
    nusers, nitems, ndraws, seed, s = ZIPF_CASES[name]
    m, ucsr, icsr, _ = zipf_reference(nusers, nitems, ndraws, seed, s)
    want = zipf_py(nusers, nitems, ndraws, seed, s)
    assert m == len(want)
    check_pair(ucsr, icsr, nusers, nitems, want)


def test_zipf_cases_hold_their_edges():
    assert {c[4] for c in ZIPF_CASES.values()} == set(ZIPF_S) == {0.5, 1.0, 2.0, 8.0}
    assert {c[1] for c in ZIPF_CASES.values()} == {1, 2, 1000, 5003}
    # pa: the nitems ≤ 1 special case, 1 at nitems = 2, the golden-ratio value itself otherwise
    assert zipf_permutation(1, 5)[0] == 0 and zipf_permutation(2, 5)[0] == 1
    assert zipf_permutation(1000, 5)[0] == 619 and zipf_permutation(5003, 5)[0] == 3093
    for n in range(1, 3000):  # and wherever the search for a coprime runs, it ends on one
        pa = zipf_permutation(n, 5)[0]
        assert math.gcd(pa, n) == 1 and pa < max(n, 2)
    for name, (nusers, nitems, ndraws, seed, s) in ZIPF_CASES.items():
        m = zipf_reference(nusers, nitems, ndraws, seed, s)[0]
        users, rank, _ = zipf_draws(nusers, nitems, ndraws, seed, s)
        assert rank.max() <= nitems - 1 and users.max() < nusers
        if nitems <= 2:
            assert ndraws > nusers * nitems >= m  # more draws than pairs there are
        if s == 8.0 and nitems > 1:
            # P(rank 0) = (1 − 2⁻⁷) / (1 − (nitems + 1)⁻⁷) ≥ 0.992: one item row holds every user
            assert np.count_nonzero(rank == 0) > 0.985 * ndraws
            irp = zipf_reference(nusers, nitems, ndraws, seed, s)[2][0]
            assert np.diff(irp).max() == nusers
        if s == 0.5 and nitems >= 1000:
            assert rank.max() > 0.99 * nitems  # the whole range is reached
    # the pb of the cases in use is not 0 where it can be anything else (a mutant pb = 0 shows)
    assert all(zipf_permutation(c[1], c[3])[1] != 0 for c in ZIPF_CASES.values() if c[1] >= 1000)


def test_zipf_ambiguity_window():
    """The window is what the issue derives, and a draw placed on an integer boundary is
    counted."""
    assert ZIPF_MARGIN == 1e-12
    x = [1.0, 2.0, 2.0 - 1e-13, 2.0 + 1e-13, 2.5, 1000.0 * (1 + 3e-12), 1000.0 * (1 - 3e-12),
         float("nan")]
    assert zipf_ambiguous(x).tolist() == [True, True, True, True, False, False, False, True]


# ---- fill_uniform ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("seed", [0, 102, SEED_MAX])
def test_fill_reference_equals_python_ints(seed, precision):
    n, k, bound = 7, 30, 0.01
    got = fill_reference(n, k, bound, seed, precision)
    assert got.shape == (n, k) and got.dtype == np.float64
    for r in range(n):
        for c in range(k):
            u01 = (mix64(seed ^ mix64(r * k + c)) >> 11) * 2.0 ** -53
            want = (2.0 * u01 - 1.0) * bound
            if precision == 32:
                want = float(np.float32(want))
            assert got[r, c] == want
    assert np.abs(got).max() <= bound and len(np.unique(got)) == n * k
