"""numpy restatement of qmfx_wals_half_cg's contract (include/qmfx.h), the tolerance rule of its
tests, and the test cases the CPU and the GPU tests share.

cg_half takes the values the device holds (an fp32 context's rounded to float32 first), widened
to `dtype`, and does every operation in `dtype`: np.longdouble is the yardstick, np.float64 /
np.float32 measure what the context's own precision costs (δ below).
"""
import numpy as np

ALPHA, LAM = 1.25, 0.75  # exact in float32

# the wrong variants the tolerance rule has to reject (tests/test_wals_cg.py)
VARIANTS = ("beta0", "nolambda", "coldstart", "swapcw")


def cg_half(rowptr, col, val, Y, X0, alpha, lam, steps, dtype, variant=None):
    """-> (X, loss terms, loss scales, flags).  scale = Σc + 2|xᵀb| + |xᵀ(A−λI)x| + λ‖x‖², the
    magnitude of the sums behind a loss term (a rounding error is relative to it, not to the
    term, which cancels)."""
    assert variant is None or variant in VARIANTS
    Y = np.asarray(Y).astype(dtype)
    X = np.asarray(X0).astype(dtype).copy()
    val = np.asarray(val).astype(dtype)
    alpha, lam = dtype(alpha), dtype(lam)
    one = dtype(1)
    G = Y.T @ Y
    nrows = len(rowptr) - 1
    loss = np.zeros(nrows, dtype)
    scale = np.zeros(nrows, dtype)
    flags = np.zeros(nrows, bool)
    lam_op = dtype(0) if variant == "nolambda" else lam
    for r in range(nrows):
        beg, end = rowptr[r], rowptr[r + 1]
        if end == beg:
            X[r] = 0
            continue
        y = Y[col[beg:end]]
        w = alpha * val[beg:end]
        c = one + w

        def A(v):
            return G @ v + y.T @ (w * (y @ v)) + lam_op * v

        b = y.T @ (w if variant == "swapcw" else c)
        x = np.zeros_like(X[r]) if variant == "coldstart" else X[r].copy()
        res = b - A(x)
        p = res.copy()
        rho = res @ res
        for _ in range(steps):
            if rho == 0:
                break
            q = A(p)
            d = p @ q
            if not d > 0:
                flags[r] = True
                break
            a = rho / d
            x = x + a * p
            res = res - a * q
            rho1 = res @ res
            p = res + (dtype(0) if variant == "beta0" else rho1 / rho) * p
            rho = rho1
        X[r] = x
        # A·x = b − res, so xᵀ(A−λI)x = xᵀ(b − res) − λxᵀx
        xb, xr, xx, cs = x @ b, x @ res, x @ x, c.sum()
        loss[r] = cs + (xb - xr - lam * xx) - 2 * xb
        scale[r] = abs(cs) + 2 * abs(xb) + abs(xb - xr - lam * xx) + lam * xx
    return X, loss, scale, flags


def row_err(X, Xref):
    """max over rows and factors of |X − Xref| / the row's ‖Xref‖∞ (rows of zeros left out)."""
    Xref = np.asarray(Xref, np.longdouble)
    nrm = np.abs(Xref).max(axis=1)
    keep = nrm > 0
    if not keep.any():
        return 0.0
    diff = np.abs(np.asarray(X, np.longdouble) - Xref).max(axis=1)
    return float((diff[keep] / nrm[keep]).max())


def loss_err(loss, ref, scale):
    """max over rows of |loss − ref| / scale (rows without signals left out)."""
    scale = np.asarray(scale, np.longdouble)
    keep = scale > 0
    if not keep.any():
        return 0.0
    diff = np.abs(np.asarray(loss, np.longdouble) - np.asarray(ref, np.longdouble))
    return float((diff[keep] / scale[keep]).max())


# Row lengths at which the kernel can go wrong: none, one, a partial pass of 4 signals, around
# the 64 lanes of a wave, and 129 (33 passes with a ragged last one; the kernel stages 4 signals
# at once, so every row past 4 is "longer than what is staged").
LENGTHS = (65, 0, 1, 2, 63, 64, 129)
BLOCK = 16  # kCgRows: rows of a workgroup

# (k, fixed-side rows, rows, steps)
CASES = (
    [(k, 17, 2 * BLOCK + 3, 1 + i % 3) for i, k in enumerate((1, 8, 16, 17, 64, 100, 128, 129, 256))]
    + [(64, 17, n, 2) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    + [(16, 1, 2 * BLOCK + 3, 1), (128, 1, BLOCK + 1, 1)]
    + [(8, 17, 2 * BLOCK + 3, 8)]
)


def make_case(k, ny, nrows, precision, seed=0):
    """A well-conditioned system: fixed-side entries of order 1/√k, values in 1..5, x₀ random of
    the solution's size (row 3, when there is one, starts at its solution).  Everything is
    rounded to the context precision, so it is what the device holds.  -> rowptr, col, val, Y, X0"""
    rng = np.random.default_rng([k, ny, nrows, seed])
    store = np.float32 if precision == 32 else np.float64
    lens = np.array([LENGTHS[i % len(LENGTHS)] for i in range(nrows)])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, ny, rowptr[-1]).astype(np.int32)
    val = rng.integers(1, 6, rowptr[-1]).astype(np.float64)
    Y = (rng.standard_normal((ny, k)) / np.sqrt(k)).astype(store).astype(np.float64)
    G = Y.T @ Y
    X0 = np.zeros((nrows, k))
    for r in range(nrows):
        if lens[r] == 0:
            X0[r] = rng.standard_normal(k)  # an empty row's old value must not survive
            continue
        y = Y[col[rowptr[r]:rowptr[r + 1]]]
        w = ALPHA * val[rowptr[r]:rowptr[r + 1]]
        sol = np.linalg.solve(G + (y.T * w) @ y + LAM * np.eye(k), y.T @ (1 + w))
        X0[r] = sol if r == 3 else np.sqrt(np.mean(sol * sol)) * rng.standard_normal(k)
    return rowptr, col, val, Y, X0.astype(store).astype(np.float64)


def ctx_dtype(precision):
    return np.float32 if precision == 32 else np.float64


def references(case, precision, steps, alpha=ALPHA, lam=LAM):
    """The longdouble result, the context dtype's result, and δ for x and for the losses."""
    rowptr, col, val, Y, X0 = case
    ld = cg_half(rowptr, col, val, Y, X0, alpha, lam, steps, np.longdouble)
    dt = cg_half(rowptr, col, val, Y, X0, alpha, lam, steps, ctx_dtype(precision))
    return ld, dt, row_err(dt[0], ld[0]), loss_err(dt[1], ld[1], ld[2])
