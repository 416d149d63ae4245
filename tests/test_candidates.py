"""CPU-side checks of recommending within candidate sets (include/qmfx.h qmfx_recommend_without,
qmfx_recommend_candidates): the header declares both calls, the ctypes table carries them with
the right output types, the numpy reference that the GPU tests compare against (the complement
of a list as the seen set) gives the hand-computed answer on a small case with a tie, and both
CLIs reject the wrong combinations of the scope flags before they touch the device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import qmf_amd
from helpers import ROOT
from test_recommend import topn_reference

BIN = os.path.join(ROOT, "qmf_amd", "bin")
# candidates per chunk of a list (RC_CHUNK of csrc/recommend.hip); the GPU tests place their
# list lengths around it
CHUNK = 512


def candidate_seen(ni, lists, seen=None):
    """The reference's seen sets of a candidate call: the complement of each user's list, united
    with the user's seen items."""
    out = []
    for t, l in enumerate(lists):
        s = np.setdiff1d(np.arange(ni), l)
        out.append(np.union1d(s, seen[t]) if seen is not None else s)
    return out


def deny_seen(deny, n, seen=None):
    """The reference's seen sets of a deny call: the deny items united with the seen items."""
    d = np.unique(np.asarray(deny, np.int64))
    return [np.union1d(d, seen[t]) if seen is not None else d for t in range(n)]


def test_header_declares_both_calls():
    src = open(os.path.join(ROOT, "include", "qmfx.h")).read()
    for name, extra in (("qmfx_recommend_without", ["int64_t ndeny", "const int64_t* deny"]),
                        ("qmfx_recommend_candidates", ["const int64_t* cptr", "int64_t ncand",
                                                       "const int64_t* cand"])):
        decl = re.search(r"int %s\(([^;]*)\);" % name, src)
        assert decl, name + " is not declared"
        args = decl.group(1)
        for a in extra + ["int topn", "int exclude", "int use_biases", "int64_t* items",
                          "double* scores", "int32_t* counts"]:
            assert a in args, (name, a)


def test_signature_table_types_the_outputs():
    S = qmf_amd._abi.SIGNATURES
    without, cands = S["qmfx_recommend_without"], S["qmfx_recommend_candidates"]
    assert len(without) == 11 and len(cands) == 12
    for sig in (without, cands):
        assert sig[1] is ctypes.c_int64 and sig[2] is ctypes.POINTER(ctypes.c_int64)
        assert sig[-3] is ctypes.POINTER(ctypes.c_int64)   # items
        assert sig[-2] is ctypes.POINTER(ctypes.c_double)  # scores
        assert sig[-1] is ctypes.POINTER(ctypes.c_int32)   # counts
    assert without[3] is ctypes.c_int64 and without[4] is ctypes.POINTER(ctypes.c_int64)
    assert cands[3] is ctypes.POINTER(ctypes.c_int64) and cands[4] is ctypes.c_int64
    assert cands[5] is ctypes.POINTER(ctypes.c_int64)
    assert hasattr(qmf_amd.lib(), "qmfx_recommend_without")
    assert hasattr(qmf_amd.lib(), "qmfx_recommend_candidates")
    assert callable(qmf_amd.Context.recommend_without)
    assert callable(qmf_amd.Context.recommend_candidates)


def test_chunk_constant_is_the_kernel_s():
    src = open(os.path.join(ROOT, "qmf_amd", "csrc", "recommend.hip")).read()
    assert re.search(r"constexpr int RC_CHUNK = %d;" % CHUNK, src)


def test_numpy_reference_on_a_hand_computed_case():
    # 3 users × 6 items; user 0 has a three-way tie at 2.0 (items 1, 3, 4)
    S = np.array([[1.0, 2.0, 0.5, 2.0, 2.0, 3.0],
                  [-0.0, 0.0, -1.0, 5.0, 0.0, -0.0],
                  [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    lists = [np.array([0, 1, 3, 4]), np.array([0, 2, 5]), np.array([], np.int64)]
    items, scores, counts = topn_reference(S, 3, candidate_seen(6, lists))
    assert items.tolist() == [[1, 3, 4], [0, 5, 2], [-1, -1, -1]]
    assert scores.tolist() == [[2.0, 2.0, 2.0], [-0.0, -0.0, -1.0], [0.0, 0.0, 0.0]]
    assert counts.tolist() == [3, 3, 0]
    # ... and with seen lists on top: user 0 has seen 3, user 1 items 0 and 5
    seen = [np.array([3]), np.array([0, 5]), np.array([1])]
    items, scores, counts = topn_reference(S, 3, candidate_seen(6, lists, seen))
    assert items.tolist() == [[1, 4, 0], [2, -1, -1], [-1, -1, -1]]
    assert counts.tolist() == [3, 1, 0]
    # a deny list: items 5 and 3 (given twice) for everybody
    items, scores, counts = topn_reference(S, 3, deny_seen([5, 3, 5], 3, seen))
    assert items.tolist() == [[1, 4, 0], [1, 4, 2], [4, 2, 0]]
    assert scores[0].tolist() == [2.0, 2.0, 1.0]
    assert counts.tolist() == [3, 3, 3]


SCOPES = ("--recommend_exclude_items", "--recommend_items", "--recommend_candidates")
EXCLUSIVE = "--recommend_exclude_items, --recommend_items and --recommend_candidates are mutually exclusive"


@pytest.mark.parametrize("exe", ["wals", "bpr"])
@pytest.mark.parametrize("flags, message", [
    (("--user_recommendations=R", SCOPES[0] + "=F", SCOPES[1] + "=F"), EXCLUSIVE),
    (("--user_recommendations=R", SCOPES[1] + "=F", SCOPES[2] + "=F"), EXCLUSIVE),
    (("--user_recommendations=R", SCOPES[0] + "=F", SCOPES[2] + "=F"), EXCLUSIVE),
    (("--user_recommendations=R", SCOPES[2] + "=F", "--recommend_users=F"),
     "--recommend_candidates and --recommend_users are mutually exclusive"),
    ((SCOPES[0] + "=F",), "--recommend_candidates need --user_recommendations"),
    ((SCOPES[1] + "=F",), "--recommend_candidates need --user_recommendations"),
    ((SCOPES[2] + "=F",), "--recommend_candidates need --user_recommendations"),
])
def test_cli_rejects_wrong_scope_flag_combinations(tmp_path, exe, flags, message):
    """The checks stand before the device is touched (and before the training file is read:
    it does not exist), so this runs without a GPU."""
    flags = [f.replace("=F", "=" + str(tmp_path / "F")).replace("=R", "=" + str(tmp_path / "R"))
             for f in flags]
    r = subprocess.run([os.path.join(BIN, exe), "--train_dataset=" + str(tmp_path / "none"),
                        "--nfactors=8", "--nepochs=1"] + flags,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "R")
