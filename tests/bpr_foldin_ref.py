"""The numpy reference of qmfx_bpr_fold_in (include/qmfx.h): the negative draws restated from
helpers.mix64 / helpers.fmix32, the schedule, and a step that is the oracle's BPREngine::update
on one triplet with throw-away copies of the two item rows and biases, of which only the user
row is kept.  The user line of that update reads the old item rows, so it is exactly the
frozen-item step.  Shared by tests/test_bpr_foldin.py (CPU) and tests/test_bpr_foldin_gpu.py."""
import functools

import numpy as np

import pyoracle as po
from helpers import M32, fmix32, mix64

SEED_SALT = 0xB5AD4ECEDA1CE2A9
CAP = 4096
LR, DECAY, USER_LAMBDA = 0.05, 0.9, 0.025


def _candidates(fk, j, t0, t1, nitems):
    """cand of attempts t0 .. t1 - 1 of draw j, vectorised (uint64 arithmetic, no wrap: every
    product is below 2^64)."""
    ctr = (np.uint64(4099 * j) + np.arange(t0, t1, dtype=np.uint64)) & np.uint64(M32)
    x = (np.uint64(fk) + ctr * np.uint64(0x9E3779B9)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return (x * np.uint64(nitems)) >> np.uint64(32)


def draw(fk, j, positives, pos_array, nitems):
    """(negative, attempts rejected) of draw j under the folded key fk: the first attempt
    t = 0, 1, ... whose candidate is not a positive, or attempt 4096 as drawn."""
    for t in range(8):  # most draws end here; the scalar form is helpers.triplets'
        cand = (fmix32((fk + (4099 * j + t) * 0x9E3779B9) & M32) * nitems) >> 32
        if cand not in positives:
            return cand, t
    c = _candidates(fk, j, 8, CAP + 1, nitems)
    free = np.nonzero(~np.isin(c, pos_array))[0]
    t = int(free[0]) if len(free) else CAP - 8
    return int(c[t]), t + 8


def draws(rowptr, col, nitems, seed, nepochs, num_neg):
    """Every step of the call in step order, per row: out[r] = [(e, i, j, n, t)], n the
    negative of draw j of positive i in pass e and t the attempts rejected before it (t == 4096:
    the draw was capped and n may be a positive, c_i included)."""
    seed_key = mix64(seed ^ SEED_SALT)
    out = []
    for r in range(len(rowptr) - 1):
        b, e1 = int(rowptr[r]), int(rowptr[r + 1])
        pos_array = np.asarray(col[b:e1], np.uint64)
        positives = set(int(x) for x in col[b:e1])
        steps = []
        for e in range(nepochs):
            ekey = mix64(seed_key ^ e)
            for i in range(e1 - b):
                pkey = mix64(ekey ^ (b + i))
                fk = (pkey & M32) ^ (pkey >> 32)
                for j in range(num_neg):
                    n, t = draw(fk, j, positives, pos_array, nitems)
                    steps.append((e, i, j, n, t))
        out.append(steps)
    return out


def rates(lr, decay, nepochs, precision):
    """lr_e: BPREngine::optimize's rule in double, each rounded once to the precision."""
    out, x = [], float(lr)
    for _ in range(nepochs):
        out.append(float(np.float32(x)) if precision == 32 else x)
        x *= decay
    return out


def oracle_step(p, qp, qn, bp, bn, lr, user_lambda, use_biases):
    """(new p, x, ok): the oracle's update on (0, 0, 1) over copies; x before the update."""
    U = np.ascontiguousarray(p[None, :], np.float64).copy()
    I2 = np.ascontiguousarray(np.stack([qp, qn]), np.float64)
    b2 = np.array([bp, bn], np.float64)
    x = po.bpr_predict_difference(U, I2, b2, 0, 0, 1, use_biases)
    try:
        po.bpr_update_seq(U, I2, b2, [[0, 0, 1]], lr, 0.0, user_lambda, 0.0, use_biases)
    except FloatingPointError:
        return p, x, False
    return U[0], x, True


def numpy_step(p, qp, qn, bp, bn, lr, user_lambda, use_biases):
    """The frozen step in plain numpy, the sum of x in factor order."""
    d = qp - qn
    x = 0.0
    for f in range(len(p)):
        x += p[f] * d[f]
    if use_biases:
        x += bp - bn
    eg = 1.0 / (1.0 + np.exp(x))
    if not np.isfinite(eg):
        return p, x, False
    return p + lr * (eg * d - user_lambda * p), x, True


def fold_in_reference(rowptr, col, I, bias, steps, nepochs, lr, decay, user_lambda, use_biases,
                      init=None, precision=64, step=oracle_step):
    """(P[n, k], losses[n], flagged[n]) of the call whose draws are `steps` (draws()): row r
    starts from init[r] (0 without), takes the steps in order at its pass's rate, and its loss
    sums log(1 + exp(-x)) over the last pass.  flagged[r]: some step of the row was not finite
    and was skipped.  user_lambda is rounded to the precision as the rates are."""
    n, k = len(rowptr) - 1, I.shape[1]
    lrs = rates(lr, decay, nepochs, precision)
    ul = float(np.float32(user_lambda)) if precision == 32 else user_lambda
    P = np.zeros((n, k)) if init is None else np.array(init, np.float64)
    losses, flagged = np.zeros(n), np.zeros(n, bool)
    for r in range(n):
        c = col[int(rowptr[r]):int(rowptr[r + 1])]
        p = P[r].copy()
        for e, i, _, neg, _ in steps[r]:
            ci = int(c[i])
            p, x, ok = step(p, I[ci], I[neg], bias[ci], bias[neg], lrs[e], ul, use_biases)
            flagged[r] |= not ok
            if ok and e == nepochs - 1:
                losses[r] += np.log(1.0 + np.exp(-x))
        P[r] = p
    return P, losses, flagged


# ---- the two batches of tests/test_bpr_foldin_gpu.py
EDGE_COUNTS = (0, 1, 63, 64, 65, 128, 129)  # the edges of the 64-lane staging


@functools.lru_cache(maxsize=None)
def batch(name):
    """(nitems, rowptr, col).  "edges": 300 items; rows of exactly 0, 1, 63, 64, 65, 128 and 129
    positives, then a dozen short rows (1..8).  "all_items": 40 items; row 0 holds all 40, so
    every draw of it is capped; then four short rows.  Columns strictly ascending."""
    rng = np.random.default_rng(17)
    if name == "edges":
        ni, counts = 300, EDGE_COUNTS + tuple(int(x) for x in rng.integers(1, 9, 12))
    else:
        ni, counts = 40, (40,) + tuple(int(x) for x in rng.integers(1, 9, 4))
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ni, c, replace=False)) for c in counts] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return ni, rowptr, col


# the seed of every call on a batch; tests/test_bpr_foldin.py asserts that "all_items" under it
# has a capped draw equal to its own positive
SEED = {"edges": 20240611, "all_items": 97}


@functools.lru_cache(maxsize=None)
def batch_draws(name, nepochs, num_neg):
    ni, rowptr, col = batch(name)
    return draws(rowptr, col, ni, SEED[name], nepochs, num_neg)


def rounded(a, precision):
    return a.astype(np.float32).astype(np.float64) if precision == 32 else a


@functools.lru_cache(maxsize=None)
def model(name, k, precision):
    """(I, bias) of a batch at k factors, as the device holds them; read-only."""
    ni = batch(name)[0]
    rng = np.random.default_rng(1000 * k + ni)
    I = rounded(rng.normal(0, 0.1, (ni, k)), precision)
    b = rounded(rng.normal(0, 0.1, ni), precision)
    I.setflags(write=False)
    b.setflags(write=False)
    return I, b


@functools.lru_cache(maxsize=None)
def start(name, k, precision):
    """Random start rows rounded to the precision; read-only."""
    n = len(batch(name)[1]) - 1
    x = rounded(np.random.default_rng(k + 5).normal(0, 0.1, (n, k)), precision)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_reference(name, k, num_neg, nepochs, precision, use_biases, with_init=False):
    """fold_in_reference of a batch's call at (LR, DECAY, USER_LAMBDA); computed once per
    session and shared; read-only."""
    _, rowptr, col = batch(name)
    I, b = model(name, k, precision)
    out = fold_in_reference(rowptr, col, I, b, batch_draws(name, nepochs, num_neg), nepochs, LR,
                            DECAY, USER_LAMBDA, use_biases,
                            init=start(name, k, precision) if with_init else None,
                            precision=precision)
    for a in out:
        a.setflags(write=False)
    return out
