"""Shared helpers for the parity tests (fixture loading, reference-format text)."""
import functools
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_ml100k():
    z = np.load(os.path.join(GOLDEN, "ml100k_shape.npz"))
    d = {k: z[k] for k in z.files}
    d["init_e9"] = np.load(os.path.join(GOLDEN, "ml100k_init.npz"))["init_e9"]
    d["users"] = d["users"].astype(np.int64)
    d["items"] = d["items"].astype(np.int64)
    d["values"] = d["values"].astype(np.float64)
    d["init"] = d["init_e9"].astype(np.float64) / 1e9
    return d


def load_tiny():
    a = np.loadtxt(os.path.join(GOLDEN, "tiny.txt"), dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2].astype(np.float64)


def factor_text(ids, F):
    """Engine::saveFactors format (Engine.cpp:98-122): id then ' %.9f' per factor."""
    return "".join(str(int(i)) + "".join(" %.9f" % x for x in row) + "\n" for i, row in zip(ids, F))


def md5(s):
    return hashlib.md5(s.encode()).hexdigest()


def synth(nusers, nitems, nnz, seed, wmax=5):
    """Uniform unique (u, i) pairs with w in 1..wmax, shuffled (SURVEY.md §8(d) recipe)."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, nusers * nitems, size=int(nnz * 1.2)))
    keys = rng.permutation(keys)[:nnz]
    return (keys // nitems).astype(np.int64), (keys % nitems).astype(np.int64), \
        rng.integers(1, wmax + 1, size=len(keys)).astype(np.float64)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def csr_from_triples(users, items, values):
    """Independent numpy restatement of groupSignals (WALSEngine.cpp:130-163): ids sorted
    ascending as signed int64 give idx 0..n-1; each row's signals sorted by the other id;
    duplicates kept.  Returns (uids, iids, (urp, ucol, uval), (irp, icol, ival))."""
    users = np.asarray(users, np.int64)
    items = np.asarray(items, np.int64)
    values = np.asarray(values, np.float64)
    uids, uidx = np.unique(users, return_inverse=True)
    iids, iidx = np.unique(items, return_inverse=True)

    def side(rows, cols, nrows):
        order = np.lexsort((cols, rows))  # stable: by row, then col
        rp = np.zeros(nrows + 1, np.int64)
        np.add.at(rp, rows + 1, 1)
        return np.cumsum(rp), cols[order].astype(np.int32), values[order]

    return uids, iids, side(uidx, iidx, len(uids)), side(iidx, uidx, len(iids))


# ---- the row-length ladder of tests/test_wals_rows_gpu.py (and its CPU anchor in
# tests/test_oracle.py): one user row of every length at which a WALS row route changes
LADDER_LENGTHS = tuple(range(171)) + (255, 256, 257, 383, 384, 385, 511, 512, 513, 640)


@functools.lru_cache(maxsize=None)
def ladder_case(k, seed, precision, with_empty=True):
    """((urp, ucol, uval), (irp, icol, ival), Y): one user row of every length in
    LADDER_LENGTHS (181 rows, 18 631 signals; `with_empty=False` leaves the length-0 row out),
    lengths assigned to rows by a seeded permutation, over max(1024, 4k) items; each row's
    columns distinct and ascending; values uniform(0, 5) with every seventh exactly 0;
    Y uniform(-0.01, 0.01).  precision 32 rounds the values and Y to fp32 first (then widens),
    so a numpy fp64 reference solves exactly the problem an fp32 context holds.  Cached: the
    arrays are read-only."""
    rng = np.random.default_rng(seed)
    nitems = max(1024, 4 * k)
    lens = np.array([n for n in LADDER_LENGTHS if with_empty or n > 0], np.int64)
    lens = rng.permutation(lens)
    urp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ucol = np.concatenate([np.sort(rng.choice(nitems, n, replace=False)) for n in lens])
    ucol = ucol.astype(np.int32)
    uval = rng.uniform(0.0, 5.0, int(urp[-1]))
    uval[::7] = 0.0
    Y = rng.uniform(-0.01, 0.01, (nitems, k))
    if precision == 32:
        uval = uval.astype(np.float32).astype(np.float64)
        Y = Y.astype(np.float32).astype(np.float64)
    rows = np.repeat(np.arange(len(lens)), lens)
    order = np.lexsort((rows, ucol))  # by item, then user
    irp = np.concatenate([[0], np.cumsum(np.bincount(ucol, minlength=nitems))]).astype(np.int64)
    out = ((urp, ucol, uval), (irp, rows[order].astype(np.int32), uval[order]), Y)
    for a in (*out[0], *out[1], Y):
        a.setflags(write=False)
    return out


def ladder_reference(rowptr, col, val, Y, alpha, lam, with_cond=True):
    """Plain numpy fp64, row by row: A = YᵀY + Yᵣᵀ·diag(αv)·Yᵣ + λI, b = Yᵣᵀ(1 + αv),
    x = solve(A, b), loss = Σc + xᵀ(A − λI)x − 2xᵀb (include/qmfx.h).  Returns
    (X, loss, cond₂(A), S) per row, S = Σc + |xᵀ(A − λI)x| + 2|xᵀb| (the size of the loss's
    terms: what a loss error is measured against).  `with_cond=False` skips the per-row
    eigenvalues (the larger part of the cost at k = 256) and returns NaN for cond₂: for callers
    whose bound does not use it."""
    Y = np.asarray(Y, np.float64)
    k = Y.shape[1]
    G = Y.T @ Y
    nrows = len(rowptr) - 1
    X = np.zeros((nrows, k))
    loss, cond, S = np.zeros(nrows), np.zeros(nrows), np.zeros(nrows)
    for r in range(nrows):
        sl = slice(int(rowptr[r]), int(rowptr[r + 1]))
        Yr = Y[col[sl]]
        w = alpha * np.asarray(val[sl], np.float64)
        M = G + (Yr.T * w) @ Yr  # A − λI
        A = M + lam * np.eye(k)
        b = Yr.T @ (1.0 + w)
        x = np.linalg.solve(A, b)
        quad, xb, cs = x @ M @ x, x @ b, float(np.sum(1.0 + w))
        X[r] = x
        loss[r] = cs + quad - 2.0 * xb
        S[r] = cs + abs(quad) + 2.0 * abs(xb)
        if with_cond:
            ev = np.linalg.eigvalsh(A)  # A is symmetric positive definite: cond₂ = λmax / λmin
            cond[r] = ev[-1] / ev[0]
        else:
            cond[r] = np.nan
    return X, loss, cond, S


@functools.lru_cache(maxsize=None)
def ladder_solution(k, seed, precision, alpha, lam, with_empty=True):
    """ladder_reference of ladder_case(k, seed, precision)'s user half, computed once per
    session and shared by the cases on that problem; read-only."""
    (urp, ucol, uval), _, Y = ladder_case(k, seed, precision, with_empty)
    out = ladder_reference(urp, ucol, uval, Y, alpha, lam)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the ladder with negative values, for the pivoted re-solve (tests/test_resolve_gpu.py and
# its CPU anchor in tests/test_oracle.py)
SIGNED_RECIPES = ("strong", "mild")


@functools.lru_cache(maxsize=None)
def signed_ladder_case(k, seed, precision, recipe):
    """ladder_case(k, seed, precision) — the same row lengths, columns, seed and Y — with every
    signal of index i ≡ 2 (mod 5) within `uval` made negative: "strong" negates it
    (v ∈ (−5, 0]: most rows of k ≥ 16 become indefinite), "mild" sets it to −0.01·|v|
    (w = αv ∈ (−2, 0] at α = 40: every system stays SPD).  Both orientations carry the same
    values; for precision 32 the values are rounded to fp32 after the change.  Cached: the
    arrays are read-only."""
    assert recipe in SIGNED_RECIPES, recipe
    (urp, ucol, v64), (irp, icol, _), _ = ladder_case(k, seed, 64)
    Y = ladder_case(k, seed, precision)[2]
    uval = v64.copy()
    uval[2::5] = -uval[2::5] if recipe == "strong" else -0.01 * np.abs(uval[2::5])
    if precision == 32:
        uval = uval.astype(np.float32).astype(np.float64)
    rows = np.repeat(np.arange(len(urp) - 1), np.diff(urp))
    order = np.lexsort((rows, ucol))  # by item, then user: ladder_case's item orientation
    assert np.array_equal(rows[order], icol)
    ival = uval[order]
    for a in (uval, ival):
        a.setflags(write=False)
    return (urp, ucol, uval), (irp, icol, ival), Y


def signed_ladder_reference(rowptr, col, val, Y, alpha, lam):
    """ladder_reference for systems that need not be positive definite.  Returns
    (X, loss, cond₂, S, has_neg, lam_min) per row: cond₂ = max|eigenvalue| / min|eigenvalue|
    of A, has_neg = some weight αv < 0, lam_min = the smallest eigenvalue of A, and
    S = Σ|c| + |xᵀ(A − λI)x| + 2|xᵀb| (Σc itself may cancel or be negative here; with c ≥ 0 this
    is ladder_reference's S)."""
    Y = np.asarray(Y, np.float64)
    k = Y.shape[1]
    G = Y.T @ Y
    nrows = len(rowptr) - 1
    X = np.zeros((nrows, k))
    loss, cond, S, lam_min = (np.zeros(nrows) for _ in range(4))
    has_neg = np.zeros(nrows, bool)
    for r in range(nrows):
        sl = slice(int(rowptr[r]), int(rowptr[r + 1]))
        Yr = Y[col[sl]]
        w = alpha * np.asarray(val[sl], np.float64)
        M = G + (Yr.T * w) @ Yr  # A − λI
        A = M + lam * np.eye(k)
        b = Yr.T @ (1.0 + w)
        x = np.linalg.solve(A, b)
        quad, xb = x @ M @ x, x @ b
        X[r] = x
        loss[r] = float(np.sum(1.0 + w)) + quad - 2.0 * xb
        S[r] = float(np.sum(np.abs(1.0 + w))) + abs(quad) + 2.0 * abs(xb)
        ev = np.linalg.eigvalsh(A)
        cond[r] = np.abs(ev).max() / np.abs(ev).min()
        lam_min[r] = ev[0]
        has_neg[r] = bool(np.any(w < 0))
    return X, loss, cond, S, has_neg, lam_min


@functools.lru_cache(maxsize=None)
def signed_ladder_solution(k, seed, precision, recipe, alpha, lam):
    """signed_ladder_reference of signed_ladder_case(k, seed, precision, recipe)'s user half,
    computed once per session and shared by the cases on that problem; read-only."""
    (urp, ucol, uval), _, Y = signed_ladder_case(k, seed, precision, recipe)
    out = signed_ladder_reference(urp, ucol, uval, Y, alpha, lam)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the fixed-side stages of a half (tests/test_fixed_side_gpu.py): problems in which every
# row of both sides is whitened and L⁻¹ of YᵀY + λI is far from a multiple of I
FIXED_LADDER = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255,
                256, 257, 511, 512, 513, 1023, 1024, 1025)
FIXED_ALPHA, FIXED_LAM = 1.0, 0.05


@functools.lru_cache(maxsize=None)
def mixing_matrix(k):
    """A fixed seeded k×k matrix U·diag(s)·Vᵀ (U, V orthogonal) whose singular values s fall
    geometrically from 1 to 0.1."""
    rng = np.random.default_rng(7000 + k)
    U = np.linalg.qr(rng.standard_normal((k, k)))[0]
    V = np.linalg.qr(rng.standard_normal((k, k)))[0]
    s = 10.0 ** (-np.arange(k) / max(k - 1, 1))
    out = (U * s) @ V.T
    out.setflags(write=False)
    return out


def correlated_factors(n, k, seed, precision):
    """n×k factors R·C, R uniform(−1, 1) and C = mixing_matrix(k), scaled to ‖·‖₂ = 1 and, for
    precision 32, rounded to fp32 (then widened).  The columns are correlated, so the Cholesky
    factor of YᵀY + λI at λ = 0.05 has off-diagonal entries of the size of its diagonal."""
    rng = np.random.default_rng(seed)
    Y = rng.uniform(-1.0, 1.0, (n, k)) @ mixing_matrix(k)
    Y /= np.linalg.norm(Y, 2)
    if precision == 32:
        Y = Y.astype(np.float32).astype(np.float64)
    return Y


@functools.lru_cache(maxsize=64)
def fixed_side_case(m, n, k, precision):
    """((urp, ucol, uval), (irp, icol, ival), (X, Y)) for m users and n items: the signals
    (u, u mod n), (u, (u + 1) mod n), (u, (u + 7) mod n) of every user and (i mod m, i) of every
    item, de-duplicated, so that no row of either side is empty and every row of either side's
    factors is gathered by a row of the other; with max(m, n) / min(m, n) ≤ 4 no row has more
    than 16 signals.  Values uniform(0.05, 1]; X and Y are correlated_factors of m and n rows.
    precision 32 rounds values and factors to fp32 first.  Cached (the last 64): read-only."""
    u, i = np.arange(m, dtype=np.int64), np.arange(n, dtype=np.int64)
    users = np.concatenate([u, u, u, i % m])
    items = np.concatenate([u % n, (u + 1) % n, (u + 7) % n, i])
    keys = np.unique(users * n + items)
    users, items = keys // n, keys % n
    seed = (m * 2048 + n) * 512 + k
    values = 1.0 - np.random.default_rng(seed).uniform(0.0, 0.95, len(keys))
    if precision == 32:
        values = values.astype(np.float32).astype(np.float64)
    _, _, ucsr, icsr = csr_from_triples(users, items, values)
    F = (correlated_factors(m, k, seed + 1, precision), correlated_factors(n, k, seed + 2, precision))
    for a in (*ucsr, *icsr, *F):
        a.setflags(write=False)
    return ucsr, icsr, F


@functools.lru_cache(maxsize=64)
def fixed_side_solution(m, n, k, precision, side):
    """ladder_reference of the half that solves `side` of fixed_side_case(m, n, k, precision)
    against the other side's factors at (FIXED_ALPHA, FIXED_LAM), and the largest off-diagonal
    magnitude of numpy's L⁻¹ (L Lᵀ = FᵀF + λI of the fixed side) over its largest diagonal
    entry.  cond₂ per row only for precision 32 (the fp64 bound does not use it).  Cached (the
    last 64): read-only."""
    ucsr, icsr, F = fixed_side_case(m, n, k, precision)
    fixed = F[1 - side]
    out = ladder_reference(*(ucsr, icsr)[side], fixed, FIXED_ALPHA, FIXED_LAM,
                           with_cond=precision == 32)
    Linv = np.linalg.inv(np.linalg.cholesky(fixed.T @ fixed + FIXED_LAM * np.eye(k)))
    d = np.abs(np.diag(Linv))
    ratio = float(np.max(np.abs(Linv) - np.diag(d)) / d.max())
    for a in out:
        a.setflags(write=False)
    return (*out, ratio)


# ---- restatement of the BPR epoch's visiting order and negative draws (qmf_amd/csrc/bpr.hip
# bpr_epoch_kernel, api_bpr.cpp qmfx_bpr_epoch): counter-based and keyed by positive slot, so
# the multiset of (u, p, n) of an epoch does not depend on the number of waves
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def permutation(seed, npos, shuffle):
    if not shuffle:
        return 1, 0
    pa = (mix64(seed ^ 0xA5A5A5A5) % npos) | 1
    while np.gcd(pa, npos) != 1:
        pa += 2
    pa %= npos
    pa = pa or 1
    return pa, mix64(seed ^ 0x5A5A5A5A) % npos


def triplets(users, items, nitems, seed, num_neg, shuffle):
    npos = len(users)
    pos = {}
    for u, i in zip(users, items):
        pos.setdefault(int(u), set()).add(int(i))
    pa, pb = permutation(seed, npos, shuffle)
    seed_key = mix64(seed ^ 0xB5AD4ECEDA1CE2A9)
    out = []
    for i in range(npos):
        slot = (pa * i + pb) % npos
        u, p = int(users[slot]), int(items[slot])
        pkey = mix64(seed_key ^ slot)
        fk = (pkey & M32) ^ (pkey >> 32)
        for j in range(num_neg):
            attempt = 0
            while True:
                h = fmix32((fk + ((4099 * j + attempt) * 0x9E3779B9)) & M32)
                cand = (h * nitems) >> 32
                if cand not in pos[u] or attempt >= 4096:
                    break
                attempt += 1
            out.append((u, p, cand))
    return np.array(out, np.int64)


def bpr_wave_case(npos=4000):
    """The multi-wave BPR epoch case shared by tests/test_bpr_kernels_gpu.py and its CPU
    anchor in tests/test_oracle.py: 320 users × 320 items (20 concurrent waves on the
    device), `npos` unique positives in random order."""
    nu = ni = 320
    rng = np.random.default_rng(320)
    keys = rng.permutation(nu * ni)[:npos]
    return nu, ni, (keys // ni).astype(np.int64), (keys % ni).astype(np.int64)


@functools.lru_cache(maxsize=None)
def bpr_wave_triplets(shuffle, npos=4000, num_neg=5):
    """The (u, p, n) of the epoch with seed 31 (identity order) or 32 (shuffled) on
    bpr_wave_case(npos).  Computed once per session; callers must not write to it."""
    _, ni, users, items = bpr_wave_case(npos)
    trip = triplets(users, items, ni, 32 if shuffle else 31, num_neg, shuffle)
    trip.setflags(write=False)
    return trip


def bpr_linear_user(trip, I0, lr, nusers):
    """U after the triplets from U0 = 0, to first order in lr (x̂ = O(lr), so the loss
    derivative is ½ and the item rows move by O(lr²)): U[u] = ½·lr·Σ (I0[p] − I0[n])."""
    U = np.zeros((nusers, I0.shape[1]))
    np.add.at(U, trip[:, 0], 0.5 * lr * (I0[trip[:, 1]] - I0[trip[:, 2]]))
    return U


def bpr_linear_item(trip, U0, lr, nitems):
    """(I, bias) after the triplets from I0 = 0, bias0 = 0, to first order in lr:
    I[i] = ½·lr·(Σ_{p=i} U0[u] − Σ_{n=i} U0[u]), bias[i] = ½·lr·(#{p=i} − #{n=i})."""
    I = np.zeros((nitems, U0.shape[1]))
    b = np.zeros(nitems)
    np.add.at(I, trip[:, 1], 0.5 * lr * U0[trip[:, 0]])
    np.add.at(I, trip[:, 2], -0.5 * lr * U0[trip[:, 0]])
    np.add.at(b, trip[:, 1], 0.5 * lr)
    np.add.at(b, trip[:, 2], -0.5 * lr)
    return I, b


# ---- test-set evaluation (qmf_amd/csrc/eval.hip): the reference of tests/test_eval_edges_gpu.py,
# anchored on pyoracle by tests/test_eval.py
def eval_scores(U, I, users, bias=None):
    """pyoracle.test_scores over all the users at once: S = bias (or 0), then
    S = S + U[users, f, None] * I[None, :, f] in factor order.  Elementwise multiply then add,
    each rounded (no fused multiply-add), so row t is test_scores' row t bit for bit."""
    U = np.asarray(U, np.float64)
    I = np.asarray(I, np.float64)
    users = np.asarray(users, np.int64)
    S = np.zeros((len(users), I.shape[0]))
    if bias is not None:  # copied, not added to the zeros: a bias of -0.0 stays -0.0
        S[:] = np.asarray(bias, np.float64)[None, :]
    for f in range(I.shape[1]):
        S = S + U[users, f, None] * I[None, :, f]
    return S


def eval_reference(S, rows, rowptr, items, values):
    """What qmfx_eval_ranks returns, by brute force, for test slots whose scores are the rows
    S[rows[t]] (a user may fill several slots) and whose labels are the CSR (rowptr, items,
    values): the score of every labelled pair, for every positive label (value > 0, in label
    order, a repeated item counted each time) the number of items scored strictly higher, and
    Σ score² per slot."""
    rows = np.asarray(rows, np.int64)
    items = np.asarray(items, np.int64)
    r = rows[np.repeat(np.arange(len(rows)), np.diff(rowptr))]
    ls = S[r, items]
    above = np.array([np.count_nonzero(S[r[e]] > S[r[e], items[e]])
                      for e in np.nonzero(np.asarray(values) > 0)[0]], np.int64)
    sq = np.array([np.sum(S[u] ** 2) for u in range(len(S))])[rows]
    return ls, above, sq


def eval_chunks(ntest, nitems):
    """(chunks, items per chunk) of the rank kernel's grid: eval.hip's eval_chunks and the
    chunk length eval_ranks derives from it, restated (32 users per group, 64 items per tile,
    about 4096 workgroups)."""
    groups = -(-ntest // 32)
    tiles = -(-nitems // 64)
    n = max(1, min(4096 // max(groups, 1), tiles))
    chunk = -(-(-(-nitems // n)) // 64) * 64
    n = -(-nitems // chunk)
    return n, -(-(-(-nitems // n)) // 64) * 64


# ---- the device's synthetic data (qmf_amd/csrc/data.hip and the driver qmfx_gen_synthetic_zipf
# in api_signals.cpp) and qmfx_fill_uniform, restated in numpy uint64 arithmetic (which wraps
# mod 2⁶⁴ as the device's does).  tests/test_synth.py anchors each piece on Python integers;
# tests/test_synth_gpu.py compares the device with them bit for bit.
_U = np.uint64


def mix64_np(x):
    """mix64 over a uint64 array."""
    x = np.asarray(x, _U) + _U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def mulhi64_np(a, b):
    """The high 64 bits of the 128-bit product a·b, a a uint64 array and b one integer < 2⁶⁴,
    from 32-bit limbs (no partial sum reaches 2⁶⁴)."""
    a = np.asarray(a, _U)
    lo32, s32 = _U(M32), _U(32)
    a0, a1 = a & lo32, a >> s32
    b0, b1 = _U(int(b) & M32), _U(int(b) >> 32)
    ll, hl, lh, hh = a0 * b0, a1 * b0, a0 * b1, a1 * b1
    cross = (ll >> s32) + (hl & lo32) + (lh & lo32)
    return hh + (hl >> s32) + (lh >> s32) + (cross >> s32)


def _csr_pair(ukeys, nusers, nitems, seed):
    """Both CSR orientations of the pairs whose sorted distinct user-major keys u·nitems + i are
    `ukeys` (uint64): ((urp, ucol, uval), (irp, icol, ival)).  The value of (u, i) in both is
    1 + mix64((seed·31 + 7 mod 2⁶⁴) ^ (u·nitems + i)) % 5; the item side is the transposed keys
    i·nusers + u, sorted."""
    vseed = _U((int(seed) * 31 + 7) & M64)

    def values(u, i):
        return (_U(1) + mix64_np(vseed ^ (u * _U(nitems) + i)) % _U(5)).astype(np.float64)

    def side(keys, nrows, ncols):
        rows, cols = keys // _U(ncols), keys % _U(ncols)
        counts = np.bincount(rows.astype(np.int64), minlength=nrows)
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), rows, cols

    urp, u, i = side(ukeys, nusers, nitems)
    ucsr = (urp, i.astype(np.int32), values(u, i))
    irp, it, us = side(np.sort(i * _U(nusers) + u), nitems, nusers)
    icsr = (irp, us.astype(np.int32), values(us, it))
    for a in (*ucsr, *icsr):
        a.setflags(write=False)
    return ucsr, icsr


@functools.lru_cache(maxsize=None)
def synth_reference(nusers, nitems, nnz, seed):
    """What qmfx_gen_synthetic(nusers, nitems, nnz, seed) leaves in a context:
    (m, (urp, ucol, uval), (irp, icol, ival)).  Draw i's key is
    (mix64(seed ^ mix64(i)) · space) >> 64 with space = nusers·nitems; the kept pairs are the
    m sorted distinct keys.  Cached: the arrays are read-only."""
    h = mix64_np(_U(seed) ^ mix64_np(np.arange(nnz, dtype=_U)))
    keys = np.unique(mulhi64_np(h, nusers * nitems))
    return (len(keys), *_csr_pair(keys, nusers, nitems, seed))


def zipf_permutation(nitems, seed):
    """(pa, pb) of the rank → item bijection (pa·r + pb) mod nitems, as launch_synth_keys_zipf
    derives them: pa the first odd number from ⌊nitems·(golden ratio − 1)⌋ | 1 upwards that is
    coprime to nitems (1 for nitems ≤ 1), reduced mod nitems; pb = mix64(seed ^ 0x7a1f) mod
    nitems."""
    pa = int(float(nitems) * 0.6180339887498949) | 1
    if nitems <= 1:
        pa = 1
    while nitems > 1 and np.gcd(pa, nitems) != 1:
        pa += 2
    return pa % max(nitems, 1), mix64(seed ^ 0x7A1F) % max(nitems, 1)


ZIPF_MARGIN = 1e-12


def zipf_ambiguous(x):
    """⌊x·(1 − 1e-12)⌋ ≠ ⌊x·(1 + 1e-12)⌋, elementwise: x is too near an integer for its floor
    to be the same under every correctly working exp/log/pow."""
    x = np.asarray(x, np.float64)
    return ~(np.floor(x * (1.0 - ZIPF_MARGIN)) == np.floor(x * (1.0 + ZIPF_MARGIN)))


def zipf_draws(nusers, nitems, ndraws, seed, s):
    """(user, rank, ambiguous) of each draw of synth_keys_zipf_kernel: h1 = mix64(seed ^
    mix64(i)), h2 = mix64(h1 ^ 0x2545f4914f6cdd1d), user = (h1·nusers) >> 64, u01 = (h2 >> 11)·
    2⁻⁵³, x = exp(u01·ln(nitems + 1)) for |s − 1| < 1e-12 and ((nitems + 1)ᵉ − 1)·u01 + 1 to the
    power 1/e, e = 1 − s, otherwise; rank = ⌊x⌋ − 1 for x ≥ 1, else 0, clamped to nitems − 1.
    A draw is ambiguous when ⌊x·(1 − 1e-12)⌋ ≠ ⌊x·(1 + 1e-12)⌋ (the device's exp/log/pow may
    differ from numpy's in the last bits: x = exp(t), t < 45, a few ulp of t are 2e-14 of x)
    or, for s ≠ 1, when moving the power's base by ± 2⁻⁵² (one rounding of the `·u01 + 1`,
    which the device may fuse) moves ⌊x⌋."""
    h1 = mix64_np(_U(seed) ^ mix64_np(np.arange(ndraws, dtype=_U)))
    h2 = mix64_np(h1 ^ _U(0x2545F4914F6CDD1D))
    users = mulhi64_np(h1, nusers)
    u01 = (h2 >> _U(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    top = float(nitems) + 1.0
    if abs(s - 1.0) < 1e-12:
        x = np.exp(u01 * np.log(top))
        near = [x]
    else:
        e = 1.0 - s
        base = (np.power(top, e) - 1.0) * u01 + 1.0
        x = np.power(base, 1.0 / e)
        near = [np.power(base - 2.0 ** -52, 1.0 / e), np.power(base + 2.0 ** -52, 1.0 / e)]
    ambiguous = zipf_ambiguous(x)
    for y in near:
        ambiguous |= ~(np.floor(y) == np.floor(x))  # a NaN counts as ambiguous
    rank = np.where(x >= 1.0, np.floor(x) - 1.0, 0.0).astype(_U)
    return users, np.minimum(rank, _U(nitems - 1)), ambiguous


@functools.lru_cache(maxsize=None)
def zipf_reference(nusers, nitems, ndraws, seed, s):
    """What qmfx_gen_synthetic_zipf(nusers, nitems, ndraws, seed, s) leaves in a context, s > 0:
    (m, (urp, ucol, uval), (irp, icol, ival), number of ambiguous draws); the draws of
    zipf_draws, item = (pa·rank + pb) mod nitems (zipf_permutation), key = user·nitems + item,
    then as synth_reference.  Exact only when no draw is ambiguous.  Cached: read-only."""
    users, rank, ambiguous = zipf_draws(nusers, nitems, ndraws, seed, s)
    pa, pb = zipf_permutation(nitems, seed)
    items = (_U(pa) * rank + _U(pb)) % _U(nitems)  # pa, rank < 2³¹: no wrap
    keys = np.unique(users * _U(nitems) + items)
    return (len(keys), *_csr_pair(keys, nusers, nitems, seed), int(np.count_nonzero(ambiguous)))


def fill_reference(n, k, bound, seed, precision):
    """The n×k matrix qmfx_fill_uniform(side, bound, seed) writes: entry (r, c) is
    (2·u01 − 1)·bound in double, u01 = (mix64(seed ^ mix64(r·k + c)) >> 11)·2⁻⁵³, rounded to
    fp32 (then widened) for precision 32."""
    h = mix64_np(_U(seed) ^ mix64_np(np.arange(n * k, dtype=_U)))
    u01 = (h >> _U(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    out = ((2.0 * u01 - 1.0) * bound).reshape(n, k)
    if precision == 32:
        out = out.astype(np.float32).astype(np.float64)
    return out


# the cases of tests/test_synth_gpu.py: (nusers, nitems, nnz, seed), keyed by test id.  The CPU
# module checks the properties each is there for.
SEED_MAX = M64
SEED_WRAP = 0x9E3779B97F4A7C15  # seed·31 + 7 ≥ 2⁶⁴
ROW_EDGES = (1, 2, 255, 256, 257, 511, 512)  # rowptr_from_keys_kernel: n + 1 entries, 256 a block
SYNTH_CASES = {}
for _n in ROW_EDGES:
    SYNTH_CASES["users%d" % _n] = (_n, 37, max(1, _n * 37 // 4), 11)
    SYNTH_CASES["items%d" % _n] = (37, _n, max(1, _n * 37 // 4), 12)
SYNTH_CASES.update({
    "empty_rows": (5000, 7, 40, 13),
    "one_item": (300, 1, 150, 14),
    "one_user": (1, 300, 150, 15),
    # the radix sort's end_bit: space 2¹³, 2¹² − 1, 2¹² + 1 and 1.4995·2¹² (83·74: a third of the
    # keys have bit 12 set); 63·65, 17·241 and 83·74 are coprime pairs
    "space_pow2": (64, 128, 2730, 16),
    "space_pow2_minus1": (63, 65, 1365, 17),
    "space_pow2_plus1": (17, 241, 1365, 18),
    "space_1p5_pow2": (83, 74, 2047, 19),
    # key space 5.2e9 > 2³²: the product's high word, the sort, 64-bit / and %
    "space_gt32_users": ((1 << 20) + 3, 5003, 20000, 20),
    "space_gt32_items": (5003, (1 << 20) + 3, 20000, 21),
    # nnz = space / 2, the most the call takes: many repeated draws
    "collisions": (31, 33, 31 * 33 // 2, 22),
    "seed0": (257, 129, 5000, 0),
    "seed_max": (257, 129, 5000, SEED_MAX),
    "seed_wrap": (257, 129, 5000, SEED_WRAP),
})
# (nusers, nitems, ndraws, seed, s); at nitems ≤ 2 the draws outnumber the pairs there are
ZIPF_S = (0.5, 1.0, 2.0, 8.0)
ZIPF_CASES = {}
for _j, (_nu, _ni, _nd) in enumerate(((300, 1, 2000), (300, 2, 2000), (777, 1000, 50000),
                                      (1237, 5003, 100000))):
    for _s in ZIPF_S:
        ZIPF_CASES["items%d-s%g" % (_ni, _s)] = (_nu, _ni, _nd, 100 + 10 * _j + int(_s), _s)
