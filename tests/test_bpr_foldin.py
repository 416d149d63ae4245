"""CPU-side checks of the BPR fold-in (include/qmfx.h qmfx_bpr_fold_in,
qmfx_bpr_recommend_fold_in): the reference the GPU tests compare against
(tests/bpr_foldin_ref.py) is anchored on the oracle and on its own draws, the header and the
ctypes table agree, and the `bpr` CLI rejects a fold-in output without its dataset before it
touches a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import qmf_amd
from bpr_foldin_ref import (CAP, SEED, batch, batch_draws, draws, fold_in_reference, numpy_step,
                            oracle_step, rates)
from helpers import ROOT, triplets
from test_foldin import _CTYPES, _declared

BIN = os.path.join(ROOT, "qmf_amd", "bin")
_CTYPES = dict(_CTYPES, uint64_t=ctypes.c_uint64)


@pytest.mark.parametrize("use_biases", [False, True])
@pytest.mark.parametrize("k", [10, 130])
def test_numpy_step_equals_the_oracle_step(k, use_biases):
    """The oracle's update over copies, user row kept, is the frozen step: 1e-15 of max|p|."""
    rng = np.random.default_rng(k)
    worst = 0.0
    for _ in range(200):
        p, qp, qn = rng.normal(0, 0.1, (3, k))
        bp, bn = rng.normal(0, 0.1, 2)
        a, xa, oka = oracle_step(p, qp, qn, bp, bn, 0.05, 0.025, use_biases)
        b, xb, okb = numpy_step(p, qp, qn, bp, bn, 0.05, 0.025, use_biases)
        assert oka and okb
        worst = max(worst, np.max(np.abs(a - b)) / np.max(np.abs(a)), abs(xa - xb) / max(abs(xa), 1))
    print("frozen step k=%d biases=%d: numpy vs oracle %.3g" % (k, use_biases, worst))
    assert worst <= 1e-15
    # the same row for p == n: the difference is exactly 0, only the regularisation moves p
    a, x, ok = oracle_step(p, qp, qp, bp, bp, 0.05, 0.025, use_biases)
    assert ok and x == 0.0 and np.array_equal(a, p + 0.05 * (-0.025 * p))


def test_a_non_finite_step_is_skipped_and_flagged():
    p, q = np.ones(4), np.full(4, np.nan)
    for step in (oracle_step, numpy_step):
        out, _, ok = step(p, q, np.zeros(4), 0.0, 0.0, 0.05, 0.025, False)
        assert not ok and np.array_equal(out, p)


def test_rates_follow_optimize():
    assert rates(0.05, 0.9, 3, 64) == [0.05, 0.05 * 0.9, 0.05 * 0.9 * 0.9]
    assert rates(0.05, 0.9, 2, 32) == [float(np.float32(0.05)), float(np.float32(0.05 * 0.9))]


def test_all_items_row_draws_its_own_positive_when_capped():
    """Row 0 of "all_items" holds every item: each of its draws is capped, is used as drawn, and
    under SEED at least one equals the step's own positive c_i."""
    ni, rowptr, col = batch("all_items")
    assert rowptr[1] == ni == 40
    for nepochs, num_neg in ((1, 9), (3, 5), (3, 4), (3, 1)):
        steps = batch_draws("all_items", nepochs, num_neg)[0]
        assert len(steps) == nepochs * 40 * num_neg
        assert all(t == CAP for *_, t in steps)
        own = sum(1 for e, i, j, n, t in steps if n == col[i])
        print("all_items nepochs=%d num_neg=%d: %d capped draws equal c_i" % (nepochs, num_neg, own))
        assert own >= 1


@pytest.mark.parametrize("name", ["edges", "all_items"])
def test_draws_avoid_the_rows_positives_unless_capped(name):
    """Rows of <= 64 and > 64 positives: an accepted draw is no positive of the row; only a
    capped one may be."""
    ni, rowptr, col = batch(name)
    counts = np.diff(rowptr)
    if name == "edges":
        assert tuple(counts[:7]) == (0, 1, 63, 64, 65, 128, 129)
    steps = batch_draws(name, 3, 5)
    for r, row in enumerate(steps):
        pos = set(col[rowptr[r]:rowptr[r + 1]].tolist())
        assert len(row) == 3 * counts[r] * 5
        assert [(e, i, j) for e, i, j, _, _ in row] == \
            [(e, i, j) for e in range(3) for i in range(counts[r]) for j in range(5)]
        for e, i, j, n, t in row:
            assert 0 <= n < ni and 0 <= t <= CAP
            assert (n not in pos) or t == CAP, (r, e, i, j, n, t)
        if counts[r] < ni:
            assert all(t < CAP for *_, t in row)


def test_draws_are_the_epoch_samplers_with_a_pass_key():
    """draws() against helpers.triplets (the epoch kernel's restated sampler): pass e of the
    fold-in is the identity-order epoch whose seed_key is mix64(seed_key ^ e), so with the keys
    lined up by hand the negatives agree."""
    import bpr_foldin_ref as ref
    from helpers import mix64
    rng = np.random.default_rng(3)
    ni, counts = 50, (3, 0, 7, 12)
    rowptr = np.concatenate([[0], np.cumsum(counts)])
    col = np.concatenate([np.sort(rng.choice(ni, c, replace=False)) for c in counts])
    users = np.repeat(np.arange(len(counts)), counts)
    seed, e = 1234, 2
    got = draws(rowptr, col, ni, seed, e + 1, 4)
    # helpers.triplets derives seed_key = mix64(s ^ SALT); ask for the s that yields pass e's key
    want = {}
    orig = ref.mix64
    pass_key = mix64(mix64(seed ^ ref.SEED_SALT) ^ e)
    import helpers
    try:
        helpers.mix64 = lambda x, _o=orig: pass_key if x == (0 ^ ref.SEED_SALT) else _o(x)
        trip = triplets(users, col, ni, 0, 4, False)
    finally:
        helpers.mix64 = orig
    for u, p, n in trip:
        want.setdefault(int(u), []).append(int(n))
    for r in range(len(counts)):
        assert [n for ee, _, _, n, _ in got[r] if ee == e] == want.get(r, [])


def test_reference_schedule_on_a_hand_case():
    """One row, one positive, one negative per pass, two passes: two frozen steps at lr and
    lr * decay, the loss from the second."""
    I = np.array([[0.3, -0.2], [0.1, 0.4], [-0.5, 0.2]])
    b = np.zeros(3)
    rowptr, col = np.array([0, 1]), np.array([1])
    steps = [[(0, 0, 0, 2, 0), (1, 0, 0, 0, 0)]]
    P, loss, flagged = fold_in_reference(rowptr, col, I, b, steps, 2, 0.1, 0.5, 0.01, False,
                                         step=numpy_step)
    p = np.zeros(2)
    d = I[1] - I[2]
    p = p + 0.1 * (0.5 * d - 0.01 * p)
    d = I[1] - I[0]
    x = p @ d
    p2 = p + 0.05 * (d / (1 + np.exp(x)) - 0.01 * p)
    assert np.allclose(P[0], p2, rtol=1e-15, atol=0) and not flagged[0]
    assert abs(loss[0] - np.log(1 + np.exp(-x))) <= 1e-15


def test_abi_table_matches_the_header():
    for name, nargs in (("qmfx_bpr_fold_in", 14), ("qmfx_bpr_recommend_fold_in", 18)):
        types = _declared(name)
        assert len(types) == nargs, (name, types)
        sig = qmf_amd._abi.SIGNATURES[name]
        assert len(sig) == nargs, name
        for i, (t, s) in enumerate(zip(types, sig)):
            assert _CTYPES[t] is s, (name, i, t, s)
        assert hasattr(qmf_amd.lib(), name)
    for m in ("bpr_fold_in", "bpr_recommend_fold_in"):
        assert callable(getattr(qmf_amd.Context, m))


@pytest.mark.parametrize("flag", ["--fold_in_user_factors", "--fold_in_recommendations"])
def test_cli_fold_in_outputs_need_the_dataset(tmp_path, flag):
    """The CHECK fires while the flags are read: no dataset is opened, no device created."""
    r = subprocess.run([os.path.join(BIN, "bpr"), "--train_dataset=" + str(tmp_path / "absent"),
                        "--nfactors=8", "--nepochs=1", flag + "=" + str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "need --fold_in_dataset" in r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_cli_fold_in_recommendation_count_is_checked(tmp_path):
    r = subprocess.run([os.path.join(BIN, "bpr"), "--train_dataset=" + str(tmp_path / "absent"),
                        "--fold_in_dataset=" + str(tmp_path / "absent2"),
                        "--fold_in_recommendations=" + str(tmp_path / "out"),
                        "--num_recommendations=129"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--num_recommendations must be in 1..128" in r.stderr
