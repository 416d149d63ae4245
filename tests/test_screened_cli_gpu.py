"""--recommend_screen of the drop-in CLIs (`wals`, `bpr`): the recommendation file is byte for
byte the one written without the flag, on tests/golden/tiny.txt and on the ML-100K-shaped
fixture, with --recommend_users and --recommend_seen too.

The two files come from two runs, so the runs must train the same model.  `wals` does from one
--distribution_file (its initial factors are otherwise drawn afresh by every run).  A `bpr`
epoch is Hogwild SGD: reproducible only while it runs on one wave, which tiny.txt's 10 users
guarantee; on the ML-100K shape `bpr` therefore recommends from its seeded initial factors
(--nepochs=0), which exercises the same selection."""
import numpy as np
import pytest

from helpers import load_ml100k, load_tiny
from test_cli_gpu import run, write_dataset, write_dist

pytestmark = pytest.mark.gpu


def _data(case):
    if case == "tiny":
        return load_tiny(), 8
    d = load_ml100k()
    return (d["users"], d["items"], d["values"]), 16


@pytest.mark.parametrize("case", ["tiny", "ml100k"])
@pytest.mark.parametrize("exe", ["wals", "bpr"])
def test_cli_screened_files_are_byte_identical(tmp_path, exe, case):
    (u, i, v), k = _data(case)
    data = str(tmp_path / "train.txt")
    write_dataset(data, u, i, v)
    ufile = str(tmp_path / "users.txt")
    ids = np.unique(u)
    with open(ufile, "w") as f:
        f.write("".join("%d\n" % x for x in ids[::-3]))
    epochs = 0 if (exe, case) == ("bpr", "ml100k") else 2
    base = ["--train_dataset=" + data, "--nfactors=%d" % k, "--nepochs=%d" % epochs,
            "--num_recommendations=7"]
    if exe == "wals":
        dist = str(tmp_path / "dist.txt")
        write_dist(dist, np.random.default_rng(3).uniform(-0.01, 0.01, len(np.unique(i)) * k))
        base += ["--distribution_file=" + dist]
    else:
        base += ["--use_biases", "--init_distribution_bound=0.1", "--seed=5"]
    for n, extra in enumerate(((), ("--recommend_seen",), ("--recommend_users=" + ufile,))):
        files = []
        for screen in ((), ("--recommend_screen",)):
            rf = str(tmp_path / ("R%d%d.txt" % (n, len(screen))))
            run(exe, *base, "--user_recommendations=" + rf, *extra, *screen)
            files.append(open(rf, "rb").read())
        assert len(files[0]) > 0
        assert files[0] == files[1], (exe, case, extra)
