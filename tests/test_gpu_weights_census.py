"""Result census of the weight, temperature-search and importance-step kernels (csrc/asmc_weights.hip, asmc_search.hip,
asmc_is_weights.hip) against tests/golden/weights_census.json.

tests/test_gpu_weights.py judges these kernels within derived tolerances.  tools/record_weights_census.py ran the cases below
once, on the build of the commit before asmc_weights.hip was split and the search's repeated sequences were folded into helpers,
and wrote per case the profile's label -> launch count, the instantiation -> count, SHA-256 digests of every device output and
the host result vectors verbatim.  Here the same cases run on the tree under test and everything must be EQUAL: a refactor of
these files changes no launch, no instantiation and no bit of any result.

Grids - and with them the order of the additions - depend on the device's compute-unit count, which the file records: on a
device with another count the GPU test fails with that message (it does not skip)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_weights_census", os.path.join(ROOT, "tools", "record_weights_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _tool()
with open(R.GOLDEN) as _f:
    GOLD = json.load(_f)


def test_census_file_lists_every_case():
    """the recorded file and the tool's case list name the same cases (no GPU needed)"""
    assert sorted(GOLD["cases"]) == sorted(c["name"] for c in R.CASES)
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)
    assert GOLD["num_cu"] > 0
    for name, g in GOLD["cases"].items():
        assert sum(g["report"].values()) > 0 and sum(g["variants"].values()) == sum(g["report"].values()), name
        assert g["digests"] or g["host"], name


@pytest.fixture(scope="module")
def engines():
    es = R.make_engines()
    yield es
    for e in es:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_weights_census(engines, case):
    assert R.num_cu() == GOLD["num_cu"], (f"the census was recorded on {GOLD['num_cu']} compute units, this device has {R.num_cu()}: "
                                          "grids differ, the digests cannot be compared")
    gold = GOLD["cases"][case["name"]]
    got = R.run_case(engines, case)
    print(case["name"], got["report"], got["host"])
    assert got["report"] == gold["report"]
    assert got["variants"] == gold["variants"]
    assert got["host"] == gold["host"]
    assert got["digests"] == gold["digests"]
