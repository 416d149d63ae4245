"""The conjugate-gradient half's reference and tolerance rule, and the `wals` flags, without a GPU.

The GPU tests (test_wals_cg_gpu.py) accept the device within 16·δ of the longdouble reference,
δ being what the context's own precision costs the same algorithm in numpy.  Here: the reference
converges to the direct solution, and the rule is tight enough to reject four plausible wrong
implementations on every test case where mathematics lets them differ at all.
"""
import os
import subprocess

import numpy as np
import pytest

import wals_cg_ref as ref
from wals_cg_ref import ALPHA, LAM, CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALS = os.path.join(ROOT, "qmf_amd", "bin", "wals")
TINY = os.path.join(ROOT, "tests", "golden", "tiny.txt")

# "Converged": CG's error bound.  After s steps ‖x_s − x*‖_A ≤ 2·((√κ−1)/(√κ+1))^s·‖x₀ − x*‖_A, κ the
# row's cond₂(A).  Termination after k steps holds in exact arithmetic only (float64 leaves up to
# 1e-3 at k = 16, where every eigenvalue is distinct), so the bound is the distance stated here;
# the GPU tests compare iterates step for step and never rely on convergence.
def case_id(c):
    return "k%d-ny%d-n%d-s%d" % c


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_converges_to_the_direct_solution(case):
    k, ny, nrows, _ = case
    rowptr, col, val, Y, X0 = ref.make_case(k, ny, nrows, 64)
    X, loss, _, flags = ref.cg_half(rowptr, col, val, Y, X0, ALPHA, LAM, k, np.float64)
    assert not flags.any()
    G = Y.T @ Y
    worst = 0.0
    for r in range(nrows):
        if rowptr[r + 1] == rowptr[r]:
            assert np.all(X[r] == 0) and loss[r] == 0
            continue
        y = Y[col[rowptr[r]:rowptr[r + 1]]]
        w = ALPHA * val[rowptr[r]:rowptr[r + 1]]
        A = G + (y.T * w) @ y + LAM * np.eye(k)
        b = y.T @ (1 + w)
        sol = np.linalg.solve(A, b)
        ev = np.linalg.eigvalsh(A)
        sk = np.sqrt(ev[-1] / ev[0])
        e0, ek = X0[r] - sol, X[r] - sol
        bound = 2 * ((sk - 1) / (sk + 1)) ** k * np.sqrt(e0 @ A @ e0)
        # a start at the solution (row 3) has e₀ of rounding size: allow float64's own residue
        floor = 1e-12 * np.sqrt(sol @ A @ sol)
        got = np.sqrt(ek @ A @ ek)
        worst = max(worst, got / (bound + floor))
        assert got <= bound + floor, r
        # the loss term is the quadratic's value at x: it exceeds the minimum by ‖x − x*‖²_A
        want = (1 + w).sum() + X[r] @ (A - LAM * np.eye(k)) @ X[r] - 2 * X[r] @ b
        assert abs(loss[r] - want) <= 1e-9 * ((1 + w).sum() + abs(want))
    print("steps = k: largest error / bound %.2e" % worst)


def separable(variant, k, ny, steps):
    """Whether mathematics lets the variant differ from the contract on this case.  β enters
    with the second step's direction, so one step is the same with β = 0.  A row's operator is
    λI plus a matrix whose range lies in the span of the fixed side's rows, so it has at most
    min(k, ny + 1) distinct eigenvalues: after that many steps CG has converged from any start,
    and x₀ no longer shows."""
    if variant == "beta0":
        return steps >= 2
    if variant == "coldstart":
        return steps < min(k, ny + 1)
    return True


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tolerance_rule_rejects_wrong_variants(case, precision):
    k, ny, nrows, steps = case
    data = ref.make_case(k, ny, nrows, precision)
    ld, _, dx, _ = ref.references(data, precision, steps)
    assert dx > 0
    tested = 0
    for variant in ref.VARIANTS:
        if not separable(variant, k, ny, steps):
            continue
        Xv = ref.cg_half(*data, ALPHA, LAM, steps, np.longdouble, variant=variant)[0]
        err = ref.row_err(Xv, ld[0])
        print("%s: δ %.2e, bound 16δ %.2e, variant error %.2e" % (variant, dx, 16 * dx, err))
        # far outside: four times the bound at the least
        assert err > 4 * 16 * dx, variant
        tested += 1
    assert tested >= 2


def test_every_variant_is_rejected_somewhere():
    """The exemptions of `separable` leave every variant tested at several cases."""
    for variant in ref.VARIANTS:
        assert sum(separable(variant, k, ny, s) for k, ny, _, s in CASES) >= 5, variant


@pytest.mark.parametrize("args,message", [
    (["--solver=lu"], "--solver must be exact or cg"),
    (["--solver=cg", "--cg_steps=0"], "--cg_steps must be at least 1"),
    (["--solver=cg", "--ngpus=2"], "--solver=cg runs on one GPU"),
])
def test_cli_rejects_before_touching_the_device(args, message, tmp_path):
    if not os.path.exists(WALS):
        pytest.fail("qmf_amd/bin/wals is not built")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([WALS, "--train_dataset=" + TINY, "--nepochs=1", "--nfactors=4",
                        "--user_factors=" + str(tmp_path / "u"),
                        "--item_factors=" + str(tmp_path / "i")] + args,
                       capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode != 0
    assert message in p.stderr + p.stdout
    assert not (tmp_path / "u").exists()
