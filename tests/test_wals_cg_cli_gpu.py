"""`wals --solver=cg` on the MI355X: the CLI's files and log against Context.wals_half_cg driven
in the same order, and --solver=exact against a run without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import qmf_amd
from helpers import GOLDEN, ROOT, factor_text, load_tiny

pytestmark = pytest.mark.gpu
WALS = os.path.join(ROOT, "qmf_amd", "bin", "wals")
TINY = os.path.join(GOLDEN, "tiny.txt")
K, NEPOCHS, STEPS, ALPHA, LAM = 8, 3, 2, 40.0, 0.05


def run(tmp_path, tag, *flags):
    uf, itf = str(tmp_path / (tag + "U.txt")), str(tmp_path / (tag + "I.txt"))
    r = subprocess.run([WALS, "--train_dataset=" + TINY, "--nfactors=%d" % K,
                        "--nepochs=%d" % NEPOCHS, "--regularization_lambda=%r" % LAM,
                        "--confidence_weight=%r" % ALPHA, "--user_factors=" + uf,
                        "--item_factors=" + itf] + list(flags),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr, open(uf).read(), open(itf).read()


def write_dist(tmp_path, nitems):
    init = np.random.default_rng(5).uniform(-0.01, 0.01, (nitems, K))
    text = ["%.9f" % x for x in np.ravel(init)]
    path = str(tmp_path / "dist.dat")
    with open(path, "w") as f:
        f.write("".join(t + "\n" for t in text))
    # what the CLI reads back from the file
    return path, np.array([float(t) for t in text]).reshape(nitems, K)


@pytest.mark.parametrize("precision", [64, 32])
def test_cli_cg_equals_the_python_sequence(tmp_path, precision):
    u, i, v = load_tiny()
    nitems = len(np.unique(i))
    dist, init = write_dist(tmp_path, nitems)
    log, utext, itext = run(tmp_path, "cg", "--solver=cg", "--cg_steps=%d" % STEPS,
                            "--distribution_file=" + dist, "--precision=%d" % precision)
    with qmf_amd.Context(K, precision) as c:
        uids, iids = c.group_signals(u, i, v)
        c.set_factors(0, np.zeros((len(uids), K)))
        c.set_factors(1, init)
        want = []
        for _ in range(NEPOCHS):
            c.wals_half_cg(0, ALPHA, LAM, STEPS)
            want.append(c.wals_half_cg(1, ALPHA, LAM, STEPS) / (len(uids) * len(iids)))
        U, I = c.factors(0), c.factors(1)
    assert utext == factor_text(uids, U)
    assert itext == factor_text(iids, I)
    got = re.findall(r"epoch \d+: train loss = ([-\d.e+]+)", log)
    # the log prints with ostream's default 6 significant digits
    assert got == ["%g" % x for x in want]


def test_cli_solver_exact_is_the_default(tmp_path):
    u, i, v = load_tiny()
    dist, _ = write_dist(tmp_path, len(np.unique(i)))
    plain = run(tmp_path, "a", "--distribution_file=" + dist)
    exact = run(tmp_path, "b", "--solver=exact", "--distribution_file=" + dist)
    assert plain[1:] == exact[1:]
    loss = r"epoch \d+: train loss = [-\d.e+]+"
    assert re.findall(loss, plain[0]) == re.findall(loss, exact[0])
