"""CPU-side checks of the screened recommend call (include/qmfx.h qmfx_recommend_screened): the
header declares the calls, the ctypes table types them, the tile constants the GPU tests size
their cases by are the kernel's, the slack constants restated here are the kernel's, the numpy
restatement of the screen's bound on a hand-computed case, and the CLI's flag check.

screen_bound_counts restates the header: the sample, the threshold L_u, the slack ε(u, i).  A
conforming screen passes item i only when a + b_i ≥ L_u − ε, and |a + b_i − score| ≤ ε, so every
passing item has score ≥ L_u − 2ε: the count of those is an upper bound of any conforming
filter's list.  The GPU tests use it to prove, before they call the device, that a case's `cap`
cannot overflow: a screen that falls back to the exact scan there is a broken screen."""
import os
import re
import subprocess

import numpy as np
import pytest

import qmf_amd
from helpers import ROOT

BIN = os.path.join(ROOT, "qmf_amd", "bin")
TILE_USERS, TILE_ITEMS = 128, 128


def exact_scores(U, Q, b=None):
    """qmfx_recommend's scores: the bias (or 0.0), then one rounded multiply and one rounded
    add per factor, in factor order."""
    s = np.zeros((len(U), len(Q))) + (0.0 if b is None else np.asarray(b, np.float64)[None, :])
    for f in range(U.shape[1]):
        s = s + U[:, f, None] * Q[None, :, f]
    return s


def norms(F):
    """qmfx_factor_norms' values."""
    s = np.zeros(len(F))
    for f in range(F.shape[1]):
        s = s + F[:, f] * F[:, f]
    return np.sqrt(s)


def sample_items(ni, S):
    return (np.arange(S, dtype=np.int64) * ni) // S


def slack(U, Q, b=None):
    """ε(u, i) of the header."""
    k = U.shape[1]
    nu, nq = norms(U)[:, None], norms(Q)[None, :]
    ab = 0.0 if b is None else np.abs(np.asarray(b, np.float64))[None, :]
    return (k + 4) * 2.0 ** -23 * nu * nq + (k + 4) * 2.0 ** -52 * ab + 2.0 ** -116 * (1 + nu + nq)


def sample_eligible(seen, ni, S, n):
    """Per user, the sample's items the user has not seen."""
    smp = sample_items(ni, S)
    return np.array([len(smp) if seen is None else len(np.setdiff1d(smp, seen[t]))
                     for t in range(n)])


def screen_bound_counts(U, Q, b, seen, topn, S):
    """Per user (a row of U; seen[t]: the user's seen items, or seen = None), the number of
    items with exact score ≥ L_u − 2ε(u, i); 0 for a user whose sample is short (the screen
    passes nothing finite for them)."""
    s = exact_scores(U, Q, b)
    e = slack(U, Q, b)
    smp = sample_items(len(Q), S)
    out = np.zeros(len(U), np.int64)
    for t in range(len(U)):
        el = smp if seen is None else np.setdiff1d(smp, seen[t])
        if len(el) < topn:
            continue
        L = np.sort(s[t, el])[::-1][topn - 1]
        out[t] = np.count_nonzero(s[t] >= L - 2 * e[t])
    return out


def test_header_declares_the_screened_calls():
    h = open(os.path.join(ROOT, "include", "qmfx.h")).read()
    m = re.search(r"int qmfx_recommend_screened\(([^;]*)\);", h)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["ctx", "nusers", "users", "topn", "exclude", "use_biases", "sample", "cap",
                     "items", "scores", "counts"]
    assert re.search(r"int qmfx_recommend_screen_stats\(qmfx_ctx\* ctx, int64_t out\[4\]\);", h)
    # the header states what a test must be able to restate
    for word in ("floor(j * nitems / S)", "(k + 4) * 2^-23", "(k + 4) * 2^-52", "2^-116",
                 "A non-finite a always passes"):
        assert word in h, word


def test_signature_table_types_the_screened_calls():
    import ctypes
    S = qmf_amd._abi.SIGNATURES
    rec, scr = S["qmfx_recommend"], S["qmfx_recommend_screened"]
    # qmfx_recommend's arguments with sample and cap (int64) before the outputs
    assert scr == rec[:6] + [ctypes.c_int64, ctypes.c_int64] + rec[6:]
    assert len(S["qmfx_recommend_screen_stats"]) == 2
    assert hasattr(qmf_amd.lib(), "qmfx_recommend_screened")
    assert hasattr(qmf_amd.lib(), "qmfx_recommend_screen_stats")
    assert callable(qmf_amd.Context.recommend_screened)
    assert callable(qmf_amd.Context.screen_stats)


def test_tile_and_slack_constants_are_the_kernel_s():
    kh = open(os.path.join(ROOT, "qmf_amd", "csrc", "kernels.h")).read()
    assert re.search(r"constexpr int kScreenTileUsers = %d, kScreenTileItems = %d;"
                     % (TILE_USERS, TILE_ITEMS), kh)
    src = open(os.path.join(ROOT, "qmf_amd", "csrc", "screen.hip")).read()
    assert "return (double)(k + 4) * 0x1p-23;" in src
    assert "return (double)(k + 4) * 0x1p-52;" in src
    assert "constexpr double SC_ABS = 0x1p-116;" in src


def test_bound_counts_on_a_hand_computed_case():
    # k = 1, user 0 = [1], user 1 = [-1]; items 1, 2, 3, 4: scores are ± the item's value
    U = np.array([[1.0], [-1.0]])
    Q = np.array([[1.0], [2.0], [3.0], [4.0]])
    assert sample_items(4, 2).tolist() == [0, 2]
    assert sample_items(3001, 256)[[0, 1, 255]].tolist() == [0, 11, 2989]
    # topn = 1: L = 3 and -1; items at or above: {2, 3} and {0}
    assert screen_bound_counts(U, Q, None, None, 1, 2).tolist() == [2, 1]
    # topn = 2: L = 1 and -3
    assert screen_bound_counts(U, Q, None, None, 2, 2).tolist() == [4, 3]
    # user 0 has seen item 2: the sample leaves item 0, L = 1; topn = 2: the sample is short
    seen = [np.array([2]), np.array([], np.int64)]
    assert screen_bound_counts(U, Q, None, seen, 1, 2).tolist() == [4, 1]
    assert screen_bound_counts(U, Q, None, seen, 2, 2).tolist() == [0, 3]
    assert sample_eligible(seen, 4, 2, 2).tolist() == [1, 2]
    # the slack: ε(u0, item 3) = 5·2^-23·4 (+ 2^-116·6) ≈ 2.4e-6; an item 3e-6 below L = 4 is
    # within 2ε and counts, one 1e-5 below does not
    eps = slack(U, Q)[0, 3]
    assert abs(eps - 5 * 2.0 ** -23 * 4) < 1e-30
    Q2 = np.array([[4.0], [4.0 - 3e-6], [4.0 - 1e-5], [1.0]])
    assert screen_bound_counts(U[:1], Q2, None, None, 1, 1).tolist() == [2]
    # a bias enters the score, and |b| the slack
    b = np.array([0.0, 0.0, 0.0, 10.0])
    assert screen_bound_counts(U[:1], Q2, b, None, 1, 1).tolist() == [3]     # sample = item 0, L = 4
    assert screen_bound_counts(U[:1], Q2, b, None, 1, 4).tolist() == [1]     # L = 11
    assert abs(slack(U[:1], Q2, b)[0, 3] - slack(U[:1], Q2)[0, 3] - 5 * 2.0 ** -52 * 10) < 1e-20


SCOPES = ("--recommend_exclude_items", "--recommend_items", "--recommend_candidates")


@pytest.mark.parametrize("exe", ["wals", "bpr"])
@pytest.mark.parametrize("scope", SCOPES)
def test_cli_rejects_the_screen_with_a_scope_flag(tmp_path, exe, scope):
    """The check stands before the device is touched and before the training file is read (it
    does not exist), so this runs without a GPU."""
    r = subprocess.run([os.path.join(BIN, exe), "--train_dataset=" + str(tmp_path / "none"),
                        "--nfactors=8", "--nepochs=1",
                        "--user_recommendations=" + str(tmp_path / "R"), "--recommend_screen",
                        scope + "=" + str(tmp_path / "F")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, r.stderr[-2000:]
    assert "--recommend_screen scans the whole catalogue" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "R")
