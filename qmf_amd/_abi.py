"""ctypes bindings for libqmfx.so (include/qmfx.h)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QMFX_LIB") or os.path.join(_HERE, "_build", "libqmfx.so")

c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64
c_int = ctypes.c_int
c_dbl = ctypes.c_double
vp = ctypes.c_void_p
P_i64 = ctypes.POINTER(c_i64)
P_i32 = ctypes.POINTER(ctypes.c_int32)
P_f64 = ctypes.POINTER(c_dbl)
P_f32 = ctypes.POINTER(ctypes.c_float)
P_u8 = ctypes.POINTER(ctypes.c_uint8)
P_int = ctypes.POINTER(c_int)

# name -> argtypes (all return int status unless listed in _RESTYPE)
SIGNATURES = {
    "qmfx_last_error": [],
    "qmfx_version": [],
    "qmfx_device_count": [P_int],
    "qmfx_create": [ctypes.POINTER(vp), c_int, c_int, c_int],
    "qmfx_destroy": [vp],
    "qmfx_sync": [vp],
    "qmfx_set_shape": [vp, c_i64, c_i64],
    "qmfx_get_shape": [vp, P_i64, P_i64, P_i64],
    "qmfx_upload_csr": [vp, c_int, P_i64, P_i32, P_f64, c_i64],
    "qmfx_gen_synthetic": [vp, c_i64, c_i64, c_i64, c_u64, P_i64],
    "qmfx_gen_synthetic_zipf": [vp, c_i64, c_i64, c_i64, c_u64, c_dbl, P_i64],
    "qmfx_download_csr": [vp, c_int, P_i64, P_i32, P_f64],
    "qmfx_group_signals": [vp, vp, c_i64, P_i64, P_i64],
    "qmfx_get_ids": [vp, c_int, P_i64],
    "qmfx_import_signals": [vp, vp],
    "qmfx_set_factors": [vp, c_int, P_f64],
    "qmfx_get_factors": [vp, c_int, P_f64],
    "qmfx_fill_uniform": [vp, c_int, c_dbl, c_u64],
    "qmfx_wals_half": [vp, c_int, c_dbl, c_dbl, P_f64],
    "qmfx_wals_half_cg": [vp, c_int, c_dbl, c_dbl, c_int, P_f64],
    "qmfx_wals_failed_rows": [vp, P_i64, c_i64, P_i64],
    "qmfx_wals_row_losses": [vp, P_f64],
    "qmfx_row_classes": [vp, c_int, P_i64],
    "qmfx_wals_row_system": [vp, c_int, c_i64, c_dbl, c_dbl, P_f64, P_f64, P_f64],
    "qmfx_wals_set_row": [vp, c_int, c_i64, P_f64],
    "qmfx_bpr_set_positives": [vp, P_i64, P_i64, c_i64],
    "qmfx_bpr_set_biases": [vp, P_f64],
    "qmfx_bpr_get_biases": [vp, P_f64],
    "qmfx_bpr_epoch": [vp, c_u64, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_int],
    "qmfx_bpr_apply": [vp, P_i64, c_i64, c_dbl, c_dbl, c_dbl, c_dbl, c_int],
    "qmfx_bpr_eval": [vp, c_int, P_i64, c_i64, c_int, P_f64],
    "qmfx_eval_set_labels": [vp, c_i64, P_i64, P_i64, P_i64, P_f64],
    "qmfx_eval_ranks": [vp, c_int, P_f64, P_i64, P_f64],
    "qmfx_recommend": [vp, c_i64, P_i64, c_int, c_int, c_int, P_i64, P_f64, P_i32],
    "qmfx_recommend_without": [vp, c_i64, P_i64, c_i64, P_i64, c_int, c_int, c_int, P_i64, P_f64,
                               P_i32],
    "qmfx_recommend_candidates": [vp, c_i64, P_i64, P_i64, c_i64, P_i64, c_int, c_int, c_int,
                                  P_i64, P_f64, P_i32],
    "qmfx_recommend_screened": [vp, c_i64, P_i64, c_int, c_int, c_int, c_i64, c_i64, P_i64,
                                P_f64, P_i32],
    "qmfx_recommend_screen_stats": [vp, P_i64],
    "qmfx_recommend_screen_stage_ms": [vp, P_f64],
    "qmfx_factor_norms": [vp, c_int, P_f64],
    "qmfx_similar": [vp, c_int, c_i64, P_i64, c_int, c_int, c_int, P_i64, P_f64, P_i32],
    "qmfx_wals_fold_in": [vp, c_int, c_i64, P_i64, P_i32, P_f64, c_dbl, c_dbl, P_f64, P_f64, P_i64],
    "qmfx_fold_in_classes": [vp, P_i64],
    "qmfx_fold_in_order": [vp, P_i64],
    "qmfx_recommend_fold_in": [vp, c_i64, P_i64, P_i32, P_f64, c_dbl, c_dbl, c_int, c_int, P_i64,
                               P_f64, P_i32, P_f64],
    "qmfx_bpr_fold_in": [vp, c_i64, P_i64, P_i32, P_f64, c_u64, c_int, c_int, c_dbl, c_dbl, c_dbl,
                         c_int, P_f64, P_f64],
    "qmfx_bpr_recommend_fold_in": [vp, c_i64, P_i64, P_i32, P_f64, c_u64, c_int, c_int, c_dbl,
                                   c_dbl, c_dbl, c_int, c_int, c_int, P_i64, P_f64, P_i32, P_f64],
    "qmfx_wals_explain": [vp, c_int, c_i64, P_i64, P_i64, P_i64, c_dbl, c_dbl, c_int, P_i64, P_i64,
                          P_f64, P_i32, P_f64, P_f64],
    "qmfx_wals_explain_rows": [vp, c_int, c_i64, P_i64, P_i32, P_f64, P_i64, P_i64, c_dbl, c_dbl,
                               c_int, P_i64, P_i64, P_f64, P_i32, P_f64, P_f64],
    "qmfx_row_lengths": [vp, c_int, c_i64, P_i64, P_i64],
    "qmfx_rccl_unique_id": [P_u8],
    "qmfx_dist_init": [vp, c_int, c_int, P_u8],
    "qmfx_partition_rows": [P_i64, c_i64, c_int, c_int, P_i64, P_i64],
    "qmfx_dist_plan": [P_i64, c_i64, c_int, c_int, P_i64],
    "qmfx_dist_init_all": [ctypes.POINTER(vp), c_int],
    "qmfx_wals_half_multi": [ctypes.POINTER(vp), c_int, c_int, c_dbl, c_dbl, P_f64],
    "qmfx_solve_kernel_stats": [vp, P_f64, P_i64, P_f64, P_f64],
    "qmfx_kernel_stats": [vp, c_int, P_f64, P_i64, P_f64, P_f64],
    "qmfx_kernel_stats_side": [vp, c_int, c_int, P_f64, P_i64, P_f64, P_f64],
    "qmfx_reset_stats": [vp],
    "qmfx_exchange_stats": [vp, c_int, P_f64, P_f64, P_f64, P_i64],
    "qmfx_bpr_plan": [vp, P_int, P_int],
    "qmfx_build_variant": [],
    "qmfx_selftest_mfma": [c_int, c_int, P_f64, P_f64, P_f64],
}
QMFX_SIM_DOT = 0
QMFX_SIM_COSINE = 1

_RESTYPE = {"qmfx_last_error": ctypes.c_char_p, "qmfx_build_variant": ctypes.c_char_p}

_lib = None


class QmfxError(RuntimeError):
    pass


def build():
    subprocess.run(["make", "-s", "-C", _HERE, "-j8"], check=True)


def lib():
    """Loads libqmfx.so.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QmfxError("libqmfx.so not built (%s): run `make -C qmf_amd` or "
                            "__graft_entry__.build()" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, argt in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = _RESTYPE.get(name, c_int)
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise QmfxError("qmfx error %d: %s" % (rc, lib().qmfx_last_error().decode()))


def _p(a, t):
    return a.ctypes.data_as(t)


def version():
    return lib().qmfx_version()


def build_variant():
    """'' for the product library; the compile flags of a timing-variant build."""
    return lib().qmfx_build_variant().decode()


def selftest_mfma(precision, A, B, device=0):
    A = np.ascontiguousarray(A, np.float64)
    B = np.ascontiguousarray(B, np.float64)
    C = np.zeros((16, 16), np.float64)
    _check(lib().qmfx_selftest_mfma(device, precision, _p(A, P_f64), _p(B, P_f64), _p(C, P_f64)))
    return C


def device_count():
    """Visible HIP devices (initialises the HIP runtime in this process)."""
    n = c_int(0)
    _check(lib().qmfx_device_count(ctypes.byref(n)))
    return n.value


def rccl_unique_id():
    buf = (ctypes.c_uint8 * 128)()
    _check(lib().qmfx_rccl_unique_id(buf))
    return bytes(buf)


def partition_rows(rowptr, world, rank):
    rp = np.ascontiguousarray(rowptr, np.int64)
    b = c_i64(0)
    e = c_i64(0)
    _check(lib().qmfx_partition_rows(_p(rp, P_i64), len(rp) - 1, world, rank, ctypes.byref(b),
                                     ctypes.byref(e)))
    return b.value, e.value


def dist_plan(rowptr, world, npieces):
    """[world][npieces + 1] piece boundaries of the half-epoch all-gather schedule."""
    rp = np.ascontiguousarray(rowptr, np.int64)
    out = np.zeros((world, npieces + 1), np.int64)
    _check(lib().qmfx_dist_plan(_p(rp, P_i64), len(rp) - 1, world, npieces, _p(out, P_i64)))
    return out


def dist_init_all(ctxs):
    """One process, several GPUs: the contexts (one per device, rank order) become one RCCL
    clique (qmfx_dist_init_all)."""
    arr = (vp * len(ctxs))(*[c.h for c in ctxs])
    _check(lib().qmfx_dist_init_all(arr, len(ctxs)))


def wals_half_multi(ctxs, side, alpha, lam):
    """qmfx_wals_half over every context of one dist_init_all; returns the global loss sum."""
    arr = (vp * len(ctxs))(*[c.h for c in ctxs])
    out = c_dbl(0)
    _check(lib().qmfx_wals_half_multi(arr, len(ctxs), side, alpha, lam, ctypes.byref(out)))
    return out.value


class Context:
    """One device context (one GPU).  Mirrors the device state of a WALSEngine/BPREngine."""

    def __init__(self, nfactors, precision=64, device=0):
        L = lib()
        h = vp()
        _check(L.qmfx_create(ctypes.byref(h), device, precision, nfactors))
        self.h = h
        self.k = nfactors
        self.precision = precision
        self.nusers = 0
        self.nitems = 0

    def close(self):
        if getattr(self, "h", None):
            lib().qmfx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- data
    def set_shape(self, nusers, nitems):
        _check(lib().qmfx_set_shape(self.h, nusers, nitems))
        self.nusers, self.nitems = nusers, nitems

    def upload_csr(self, side, rowptr, colidx, values):
        rp = np.ascontiguousarray(rowptr, np.int64)
        col = np.ascontiguousarray(colidx, np.int32)
        val = np.ascontiguousarray(values, np.float64)
        _check(lib().qmfx_upload_csr(self.h, side, _p(rp, P_i64), _p(col, P_i32), _p(val, P_f64),
                                     len(col)))

    def gen_synthetic(self, nusers, nitems, nnz, seed):
        out = c_i64(0)
        _check(lib().qmfx_gen_synthetic(self.h, nusers, nitems, nnz, seed, ctypes.byref(out)))
        self.nusers, self.nitems = nusers, nitems
        return out.value

    def gen_synthetic_zipf(self, nusers, nitems, ndraws, seed, zipf_s):
        """Power-law item popularity (qmfx_gen_synthetic_zipf); returns the unique nnz."""
        out = c_i64(0)
        _check(lib().qmfx_gen_synthetic_zipf(self.h, nusers, nitems, ndraws, seed, float(zipf_s),
                                             ctypes.byref(out)))
        self.nusers, self.nitems = nusers, nitems
        return out.value

    def group_signals(self, users, items, values):
        """Device ingest (qmfx_group_signals) of raw (user id, item id, value) triples in
        file order; returns (user ids, item ids), ascending."""
        rec = np.empty(len(users), dtype=np.dtype([("u", "<i8"), ("i", "<i8"), ("v", "<f8")]))
        rec["u"], rec["i"], rec["v"] = users, items, values
        nu, ni = c_i64(0), c_i64(0)
        _check(lib().qmfx_group_signals(self.h, rec.ctypes.data_as(vp), len(rec),
                                        ctypes.byref(nu), ctypes.byref(ni)))
        self.nusers, self.nitems = nu.value, ni.value
        return self.ids(0), self.ids(1)

    def import_signals(self, src):
        """Take src's shape, ids and both CSRs device to device (qmfx_import_signals)."""
        _check(lib().qmfx_import_signals(self.h, src.h))
        self.nusers, self.nitems, _ = self.shape()

    def ids(self, side):
        out = np.empty(self.nusers if side == 0 else self.nitems, np.int64)
        _check(lib().qmfx_get_ids(self.h, side, _p(out, P_i64)))
        return out

    def shape(self):
        a, b, c = c_i64(), c_i64(), c_i64()
        _check(lib().qmfx_get_shape(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def download_csr(self, side):
        nu, ni, nnz = self.shape()
        n = nu if side == 0 else ni
        rp = np.empty(n + 1, np.int64)
        col = np.empty(max(nnz, 1), np.int32)
        val = np.empty(max(nnz, 1), np.float64)  # exactly the device's values (fp32 widened)
        _check(lib().qmfx_download_csr(self.h, side, _p(rp, P_i64), _p(col, P_i32), _p(val, P_f64)))
        return rp, col[:nnz], val[:nnz]

    # ---- factors
    def _n(self, side):
        return self.nusers if side == 0 else self.nitems

    def set_factors(self, side, F):
        F = np.ascontiguousarray(F, np.float64)
        assert F.shape == (self._n(side), self.k), F.shape
        _check(lib().qmfx_set_factors(self.h, side, _p(F, P_f64)))

    def factors(self, side):
        out = np.empty((self._n(side), self.k), np.float64)
        _check(lib().qmfx_get_factors(self.h, side, _p(out, P_f64)))
        return out

    def fill_uniform(self, side, bound, seed):
        _check(lib().qmfx_fill_uniform(self.h, side, bound, seed))

    # ---- WALS
    def wals_half(self, side, alpha, lam):
        out = c_dbl(0)
        _check(lib().qmfx_wals_half(self.h, side, alpha, lam, ctypes.byref(out)))
        return out.value

    def wals_half_cg(self, side, alpha, lam, steps):
        """One half by `steps` conjugate-gradient steps per row from the side's current factors."""
        out = c_dbl(0)
        _check(lib().qmfx_wals_half_cg(self.h, side, alpha, lam, steps, ctypes.byref(out)))
        return out.value

    def row_classes(self, side):
        """Row plan of a side: {'whitened': [8 bucket counts], 'direct', 'heavy', 'segments'}."""
        out = np.zeros(11, np.int64)
        _check(lib().qmfx_row_classes(self.h, side, _p(out, P_i64)))
        return {"whitened": out[:8].tolist(), "direct": int(out[8]), "heavy": int(out[9]),
                "segments": int(out[10])}

    def row_losses(self, side):
        out = np.empty(self._n(side), np.float64)
        _check(lib().qmfx_wals_row_losses(self.h, _p(out, P_f64)))
        return out

    def failed_rows(self):
        cnt = c_i64(0)
        _check(lib().qmfx_wals_failed_rows(self.h, None, 0, ctypes.byref(cnt)))
        rows = np.empty(max(cnt.value, 1), np.int64)
        _check(lib().qmfx_wals_failed_rows(self.h, _p(rows, P_i64), cnt.value, ctypes.byref(cnt)))
        return rows[: cnt.value]

    def row_system(self, side, row, alpha, lam):
        """(A, b, Σc) of one row's k×k system, built on the device."""
        k = self.k
        A = np.empty((k, k), np.float64)
        b = np.empty(k, np.float64)
        cs = np.zeros(1, np.float64)
        _check(lib().qmfx_wals_row_system(self.h, side, int(row), float(alpha), float(lam),
                                          _p(A, P_f64), _p(b, P_f64), _p(cs, P_f64)))
        return A, b, float(cs[0])

    def sync(self):
        _check(lib().qmfx_sync(self.h))

    # ---- BPR
    def bpr_set_positives(self, users, items):
        u = np.ascontiguousarray(users, np.int64)
        i = np.ascontiguousarray(items, np.int64)
        _check(lib().qmfx_bpr_set_positives(self.h, _p(u, P_i64), _p(i, P_i64), len(u)))

    def bpr_set_biases(self, b):
        b = np.ascontiguousarray(b, np.float64)
        _check(lib().qmfx_bpr_set_biases(self.h, _p(b, P_f64)))

    def bpr_biases(self):
        out = np.empty(self.nitems, np.float64)
        _check(lib().qmfx_bpr_get_biases(self.h, _p(out, P_f64)))
        return out

    def bpr_epoch(self, seed, num_neg, lr, bias_lambda, user_lambda, item_lambda, use_biases,
                  shuffle=True):
        _check(lib().qmfx_bpr_epoch(self.h, seed, num_neg, lr, bias_lambda, user_lambda,
                                    item_lambda, int(use_biases), int(shuffle)))

    def bpr_apply(self, triplets, lr, bias_lambda, user_lambda, item_lambda, use_biases):
        t = np.ascontiguousarray(triplets, np.int64).reshape(-1, 3)
        _check(lib().qmfx_bpr_apply(self.h, _p(t, P_i64), len(t), lr, bias_lambda, user_lambda,
                                    item_lambda, int(use_biases)))

    def bpr_eval(self, slot, triplets, use_biases):
        t = np.ascontiguousarray(triplets, np.int64).reshape(-1, 3)
        self._keep_trip = getattr(self, "_keep_trip", {})
        self._keep_trip[slot] = t
        out = c_dbl(0)
        _check(lib().qmfx_bpr_eval(self.h, slot, _p(t, P_i64), len(t), int(use_biases),
                                   ctypes.byref(out)))
        return out.value

    # ---- test-set evaluation (Engine.cpp:73-96, Metrics.cpp:27-164)
    def eval_set_labels(self, users, rowptr, items, values):
        """Test users (user idx) and their labelled items as a CSR over the test slots."""
        users = np.ascontiguousarray(users, np.int64)
        rowptr = np.ascontiguousarray(rowptr, np.int64)
        items = np.ascontiguousarray(items, np.int64)
        values = np.ascontiguousarray(values, np.float64)
        if len(rowptr) != len(users) + 1 or len(items) != rowptr[-1] or len(values) != len(items):
            raise QmfxError("label CSR shape mismatch")
        _check(lib().qmfx_eval_set_labels(self.h, len(users), _p(users, P_i64), _p(rowptr, P_i64),
                                          _p(items, P_i64), _p(values, P_f64)))
        self._ev = (len(users), int(rowptr[-1]), int(np.count_nonzero(values > 0)))

    def eval_ranks(self, use_biases=False):
        """(label_scores, above, sq_sum): see include/qmfx.h qmfx_eval_ranks."""
        nt, nl, npos = self._ev
        ls, ab, sq = np.empty(nl), np.empty(npos, np.int64), np.empty(nt)
        _check(lib().qmfx_eval_ranks(self.h, int(use_biases), _p(ls, P_f64), _p(ab, P_i64),
                                     _p(sq, P_f64)))
        return ls, ab, sq

    # ---- top-N recommendations
    def recommend(self, users, topn, exclude=0, use_biases=False):
        """(items[n, topn], scores[n, topn], counts[n]) for the user indices `users`: see
        include/qmfx.h qmfx_recommend (exclude: 0 all items, 1 minus the side-0 CSR row,
        2 minus the BPR positives)."""
        users = np.ascontiguousarray(users, np.int64)
        n, w = len(users), max(int(topn), 0)
        items = np.empty((n, w), np.int64)
        scores = np.empty((n, w), np.float64)
        counts = np.empty(n, np.int32)
        _check(lib().qmfx_recommend(self.h, n, _p(users, P_i64), int(topn), int(exclude),
                                    int(use_biases), _p(items, P_i64), _p(scores, P_f64),
                                    _p(counts, P_i32)))
        return items, scores, counts

    def recommend_screened(self, users, topn, exclude=0, use_biases=False, sample=0, cap=0):
        """recommend(), bit for bit, through an f32 screen of the catalogue and an exact re-rank
        of what it keeps: see include/qmfx.h qmfx_recommend_screened (sample, cap: 0 = auto)."""
        users = np.ascontiguousarray(users, np.int64)
        items, scores, counts = self._topn_out(len(users), topn)
        _check(lib().qmfx_recommend_screened(self.h, len(users), _p(users, P_i64), int(topn),
                                             int(exclude), int(use_biases), int(sample), int(cap),
                                             _p(items, P_i64), _p(scores, P_f64),
                                             _p(counts, P_i32)))
        return items, scores, counts

    def screen_stats(self):
        """Of the last recommend_screened: [users through the screen, users through the exact
        scan, candidates kept, longest kept list]."""
        out = np.zeros(4, np.int64)
        _check(lib().qmfx_recommend_screen_stats(self.h, _p(out, P_i64)))
        return out

    def screen_stage_ms(self):
        """Of the last recommend_screened: device milliseconds of [sample, rows / norms / f32
        copies, screen, counters + sort, re-rank, exact scan]."""
        out = np.zeros(6, np.float64)
        _check(lib().qmfx_recommend_screen_stage_ms(self.h, _p(out, P_f64)))
        return out

    def _topn_out(self, n, topn):
        w = max(int(topn), 0)
        return np.empty((n, w), np.int64), np.empty((n, w), np.float64), np.empty(n, np.int32)

    def recommend_without(self, users, deny, topn, exclude=0, use_biases=False):
        """recommend() with the item indices `deny` (any order, repeats allowed) eligible for
        nobody: see include/qmfx.h qmfx_recommend_without."""
        users = np.ascontiguousarray(users, np.int64)
        deny = np.ascontiguousarray(deny, np.int64)
        items, scores, counts = self._topn_out(len(users), topn)
        _check(lib().qmfx_recommend_without(self.h, len(users), _p(users, P_i64), len(deny),
                                            _p(deny, P_i64), int(topn), int(exclude),
                                            int(use_biases), _p(items, P_i64), _p(scores, P_f64),
                                            _p(counts, P_i32)))
        return items, scores, counts

    def recommend_candidates(self, users, topn, cand, cptr=None, exclude=0, use_biases=False):
        """recommend() within candidate lists: `cand` is one strictly ascending list of item
        indices shared by all users, or with cptr (len(users) + 1 offsets) user t's list is
        cand[cptr[t]:cptr[t + 1]]: see include/qmfx.h qmfx_recommend_candidates.  The lists are
        passed through as given, neither sorted nor deduplicated."""
        users = np.ascontiguousarray(users, np.int64)
        cand = np.ascontiguousarray(cand, np.int64)
        ncand = len(cand)
        if cptr is not None:
            cptr = np.ascontiguousarray(cptr, np.int64)
            if len(cptr) != len(users) + 1 or (len(cptr) and cptr.max() > ncand):
                raise QmfxError("candidate list shape mismatch")
        items, scores, counts = self._topn_out(len(users), topn)
        _check(lib().qmfx_recommend_candidates(
            self.h, len(users), _p(users, P_i64), None if cptr is None else _p(cptr, P_i64),
            ncand, _p(cand, P_i64), int(topn), int(exclude), int(use_biases), _p(items, P_i64),
            _p(scores, P_f64), _p(counts, P_i32)))
        return items, scores, counts

    # ---- similar rows
    def factor_norms(self, side):
        """The norm of every row of `side`: sqrt of the sequential, unfused sum of squares
        (include/qmfx.h qmfx_factor_norms)."""
        out = np.empty(self._n(side), np.float64)
        _check(lib().qmfx_factor_norms(self.h, int(side), _p(out, P_f64)))
        return out

    def similar(self, side, rows, topn, metric=QMFX_SIM_COSINE, exclude_self=True):
        """(neighbours[n, topn], scores[n, topn], counts[n]) for the row indices `rows` of
        `side`, ranked among the rows of the same side: see include/qmfx.h qmfx_similar
        (metric: QMFX_SIM_DOT or QMFX_SIM_COSINE)."""
        rows = np.ascontiguousarray(rows, np.int64)
        n, w = len(rows), max(int(topn), 0)
        neighbours = np.empty((n, w), np.int64)
        scores = np.empty((n, w), np.float64)
        counts = np.empty(n, np.int32)
        _check(lib().qmfx_similar(self.h, int(side), n, _p(rows, P_i64), int(topn), int(metric),
                                  int(bool(exclude_self)), _p(neighbours, P_i64),
                                  _p(scores, P_f64), _p(counts, P_i32)))
        return neighbours, scores, counts

    # ---- fold-in
    @staticmethod
    def _rows(rowptr, colidx, values):
        rp = np.ascontiguousarray(rowptr, np.int64)
        col = np.ascontiguousarray(colidx, np.int32)
        val = np.ascontiguousarray(values, np.float64)
        if len(rp) < 1 or len(col) != len(val):
            raise QmfxError("fold-in CSR shape mismatch")
        return rp, col, val

    def wals_fold_in(self, side, rowptr, colidx, values, alpha, lam):
        """(factors[n, k], losses[n], pivoted) of the n = len(rowptr) - 1 new rows of `side`
        given as a CSR of their own: see include/qmfx.h qmfx_wals_fold_in."""
        rp, col, val = self._rows(rowptr, colidx, values)
        n = len(rp) - 1
        F = np.empty((n, self.k), np.float64)
        losses = np.empty(n, np.float64)
        piv = c_i64(0)
        _check(lib().qmfx_wals_fold_in(self.h, int(side), n, _p(rp, P_i64), _p(col, P_i32),
                                       _p(val, P_f64), float(alpha), float(lam), _p(F, P_f64),
                                       _p(losses, P_f64), ctypes.byref(piv)))
        return F, losses, piv.value

    def fold_in_classes(self):
        """The last fold-in's row plan, as row_classes reports a side's."""
        out = np.zeros(11, np.int64)
        _check(lib().qmfx_fold_in_classes(self.h, _p(out, P_i64)))
        return {"whitened": out[:8].tolist(), "direct": int(out[8]), "heavy": int(out[9]),
                "segments": int(out[10])}

    def fold_in_order(self, nrows):
        """The last fold-in's processing order (its nrows row indices)."""
        out = np.empty(nrows, np.int64)
        _check(lib().qmfx_fold_in_order(self.h, _p(out, P_i64)))
        return out

    def recommend_fold_in(self, rowptr, colidx, values, alpha, lam, topn, exclude_seen=True):
        """(items[n, topn], scores[n, topn], counts[n], factors[n, k]) of n new users: see
        include/qmfx.h qmfx_recommend_fold_in."""
        rp, col, val = self._rows(rowptr, colidx, values)
        n, w = len(rp) - 1, max(int(topn), 0)
        items = np.empty((n, w), np.int64)
        scores = np.empty((n, w), np.float64)
        counts = np.empty(n, np.int32)
        F = np.empty((n, self.k), np.float64)
        _check(lib().qmfx_recommend_fold_in(self.h, n, _p(rp, P_i64), _p(col, P_i32),
                                            _p(val, P_f64), float(alpha), float(lam), int(topn),
                                            int(bool(exclude_seen)), _p(items, P_i64),
                                            _p(scores, P_f64), _p(counts, P_i32), _p(F, P_f64)))
        return items, scores, counts, F

    # ---- BPR fold-in
    def _bpr_rows(self, rowptr, colidx, init):
        rp = np.ascontiguousarray(rowptr, np.int64)
        col = np.ascontiguousarray(colidx, np.int32)
        if len(rp) < 1:
            raise QmfxError("fold-in CSR shape mismatch")
        if init is not None:
            init = np.ascontiguousarray(init, np.float64)
            if init.shape != (len(rp) - 1, self.k):
                raise QmfxError("init must be one row of nfactors per new row")
        return rp, col, init

    def bpr_fold_in(self, rowptr, colidx, seed, nepochs, num_neg, lr, decay, user_lambda,
                    use_biases=False, init=None):
        """(factors[n, k], losses[n]) of the n = len(rowptr) - 1 new users whose positive items
        are the rows of the CSR (strictly ascending item indices), fitted by SGD against the
        frozen item factors: see include/qmfx.h qmfx_bpr_fold_in."""
        rp, col, init = self._bpr_rows(rowptr, colidx, init)
        n = len(rp) - 1
        F = np.empty((n, self.k), np.float64)
        losses = np.empty(n, np.float64)
        _check(lib().qmfx_bpr_fold_in(self.h, n, _p(rp, P_i64), _p(col, P_i32),
                                      None if init is None else _p(init, P_f64), int(seed),
                                      int(nepochs), int(num_neg), float(lr), float(decay),
                                      float(user_lambda), int(bool(use_biases)), _p(F, P_f64),
                                      _p(losses, P_f64)))
        return F, losses

    def bpr_recommend_fold_in(self, rowptr, colidx, seed, nepochs, num_neg, lr, decay,
                              user_lambda, topn, use_biases=False, init=None, exclude_seen=True):
        """(items[n, topn], scores[n, topn], counts[n], factors[n, k]) of n new users: see
        include/qmfx.h qmfx_bpr_recommend_fold_in."""
        rp, col, init = self._bpr_rows(rowptr, colidx, init)
        n = len(rp) - 1
        items, scores, counts = self._topn_out(n, topn)
        F = np.empty((n, self.k), np.float64)
        _check(lib().qmfx_bpr_recommend_fold_in(
            self.h, n, _p(rp, P_i64), _p(col, P_i32), None if init is None else _p(init, P_f64),
            int(seed), int(nepochs), int(num_neg), float(lr), float(decay), float(user_lambda),
            int(bool(use_biases)), int(topn), int(bool(exclude_seen)), _p(items, P_i64),
            _p(scores, P_f64), _p(counts, P_i32), _p(F, P_f64)))
        return items, scores, counts, F

    # ---- explanations
    def row_lengths(self, side, rows):
        """The signal counts of rows of the context's CSR of `side`."""
        rows = np.ascontiguousarray(rows, np.int64)
        out = np.empty(len(rows), np.int64)
        _check(lib().qmfx_row_lengths(self.h, int(side), len(rows), _p(rows, P_i64),
                                      _p(out, P_i64)))
        return out

    @staticmethod
    def _explain_out(qptr, targets, lengths, topm, full):
        """The output arrays of an explain call: lengths[q] = signals of query q's row."""
        qptr = np.ascontiguousarray(qptr, np.int64)
        targets = np.ascontiguousarray(targets, np.int64)
        if len(qptr) != len(lengths) + 1 or (len(qptr) > 1 and qptr[-1] != len(targets)):
            raise QmfxError("explain query shape mismatch")
        npairs, w = len(targets), max(int(topm), 0)
        out = [np.empty((npairs, w), np.int64), np.empty((npairs, w), np.int64),
               np.empty((npairs, w), np.float64), np.empty(npairs, np.int32),
               np.empty(npairs, np.float64)]
        allv = allptr = None
        if full:
            per_pair = np.repeat(np.asarray(lengths, np.int64), np.maximum(np.diff(qptr), 0))
            allptr = np.concatenate([[0], np.cumsum(per_pair)]).astype(np.int64)
            allv = np.empty(int(allptr[-1]), np.float64)
        return qptr, targets, out, allv, allptr

    def wals_explain(self, side, rows, qptr, targets, alpha, lam, topm, full=False):
        """Why is target t recommended to row r?  (sources[np, topm], positions[np, topm],
        contribs[np, topm], counts[np], totals[np], full) for the pairs (rows[q], t), t in
        targets[qptr[q]:qptr[q + 1]]: see include/qmfx.h qmfx_wals_explain.  full is None, or
        with full=True (values, ptr): pair p's contributions in CSR order are
        values[ptr[p]:ptr[p + 1]].  For a trained row the total is not recommend()'s score (the
        stored row was solved against older factors of the other side)."""
        rows = np.ascontiguousarray(rows, np.int64)
        lengths = self.row_lengths(side, rows) if full else np.zeros(len(rows), np.int64)
        qptr, targets, out, allv, allptr = self._explain_out(qptr, targets, lengths, topm, full)
        _check(lib().qmfx_wals_explain(
            self.h, int(side), len(rows), _p(rows, P_i64), _p(qptr, P_i64), _p(targets, P_i64),
            float(alpha), float(lam), int(topm), _p(out[0], P_i64), _p(out[1], P_i64),
            _p(out[2], P_f64), _p(out[3], P_i32), _p(out[4], P_f64),
            _p(allv, P_f64) if full else None))
        return (*out, (allv, allptr) if full else None)

    def wals_explain_rows(self, side, rowptr, colidx, values, qptr, targets, alpha, lam, topm,
                          full=False):
        """wals_explain for rows given as a CSR of their own (wals_fold_in's): query q is row q.
        For these rows the total is recommend_fold_in's score, to rounding."""
        rp, col, val = self._rows(rowptr, colidx, values)
        qptr, targets, out, allv, allptr = self._explain_out(qptr, targets, np.diff(rp), topm, full)
        _check(lib().qmfx_wals_explain_rows(
            self.h, int(side), len(rp) - 1, _p(rp, P_i64), _p(col, P_i32), _p(val, P_f64),
            _p(qptr, P_i64), _p(targets, P_i64), float(alpha), float(lam), int(topm),
            _p(out[0], P_i64), _p(out[1], P_i64), _p(out[2], P_f64), _p(out[3], P_i32),
            _p(out[4], P_f64), _p(allv, P_f64) if full else None))
        return (*out, (allv, allptr) if full else None)

    # ---- dist / stats
    def dist_init(self, rank, world, uid):
        """uid = rank 0's rccl_unique_id(), or None: partition and shard without a
        communicator (each half solves only this rank's rows)."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid) if uid is not None else None
        _check(lib().qmfx_dist_init(self.h, rank, world, buf))

    def solve_stats(self):
        ms, n, fl, by = c_dbl(), c_i64(), c_dbl(), c_dbl()
        _check(lib().qmfx_solve_kernel_stats(self.h, ctypes.byref(ms), ctypes.byref(n),
                                             ctypes.byref(fl), ctypes.byref(by)))
        return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)

    def kernel_stats(self, cls):
        ms, n, fl, by = c_dbl(), c_i64(), c_dbl(), c_dbl()
        _check(lib().qmfx_kernel_stats(self.h, cls, ctypes.byref(ms), ctypes.byref(n),
                                       ctypes.byref(fl), ctypes.byref(by)))
        return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)

    def kernel_stats_side(self, cls, side):
        """kernel_stats(cls) over the halves that solved `side` only."""
        ms, n, fl, by = c_dbl(), c_i64(), c_dbl(), c_dbl()
        _check(lib().qmfx_kernel_stats_side(self.h, cls, side, ctypes.byref(ms), ctypes.byref(n),
                                            ctypes.byref(fl), ctypes.byref(by)))
        return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)

    def reset_stats(self):
        _check(lib().qmfx_reset_stats(self.h))

    def exchange_stats(self, side):
        """Multi-rank halves that solved `side` since reset (include/qmfx.h
        qmfx_exchange_stats): exchange_ms, exposed_ms, solve_ms (sums) and halves."""
        x, t, sv, n = c_dbl(), c_dbl(), c_dbl(), c_i64()
        _check(lib().qmfx_exchange_stats(self.h, side, ctypes.byref(x), ctypes.byref(t),
                                         ctypes.byref(sv), ctypes.byref(n)))
        return dict(exchange_ms=x.value, exposed_ms=t.value, solve_ms=sv.value, halves=n.value)

    def bpr_plan(self):
        """(waves, atomic_user) of the last bpr_epoch."""
        w, a = c_int(), c_int()
        _check(lib().qmfx_bpr_plan(self.h, ctypes.byref(w), ctypes.byref(a)))
        return w.value, a.value
