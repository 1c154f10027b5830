"""Launch census of the mutation drivers (csrc/asmc_pcn_drive.hip) against tests/golden/mutation_census.json.

tests/test_gpu_pcn.py pins `asmc_pcn_mutate` launch by launch; `asmc_pcn_mutate_flow` was pinned by results within a tolerance
only.  tools/record_mutation_census.py ran the cases below once, on the build of the commit before the drivers moved to a file of
their own, and wrote per case the profile's label -> launch count, the instantiation -> count, SHA-256 digests of x, ll, lp, lq
(and of a chain target's slots), the accept counts, the step-size history and the final rho.  Here the same cases run on the tree
under test and everything must be EQUAL: a driver refactor changes no launch, no instantiation and no bit of any result.

The error table: single-fault calls of asmc_pcn_mutate_flow return the recorded code, launch nothing and leave x untouched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_mutation_census", os.path.join(ROOT, "tools", "record_mutation_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _tool()
with open(R.GOLDEN) as _f:
    GOLD = json.load(_f)


def test_census_file_lists_every_case():
    """the recorded file and the tool's case list name the same cases (no GPU needed)"""
    assert sorted(GOLD["cases"]) == sorted(c["name"] for c in R.CASES)
    assert sorted(GOLD["errors"]) == sorted(R.ERRORS)
    assert (GOLD["n"], GOLD["steps"]) == (R.N, R.STEPS)
    assert set(GOLD["unstable"]) <= set(GOLD["cases"])
    for name, g in GOLD["cases"].items():
        assert ("digests" in g) == (name not in GOLD["unstable"]), name
        assert sum(g["report"].values()) > 0 and sum(g["variants"].values()) == sum(g["report"].values()), name


@pytest.fixture(scope="module")
def eng():
    return R.make_engine()


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_mutation_census(eng, case):
    gold = GOLD["cases"][case["name"]]
    got = R.run_case(eng, case)
    print(case["name"], got["report"], got["n_accept"], got["rho"])
    assert got["report"] == gold["report"]
    assert got["variants"] == gold["variants"]
    assert got["n_accept"] == gold["n_accept"]
    assert got["rho_hist"] == gold["rho_hist"] and got["rho"] == gold["rho"]
    if "digests" in gold:
        assert got["digests"] == gold["digests"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.ERRORS)
def test_mutation_flow_single_fault_calls(eng, name):
    got = R.run_error(eng, name)
    print(name, got)
    assert got["rc"] == GOLD["errors"][name]["rc"] and got["rc"] != 0
    assert got["launched"] == {}, got["launched"]
    assert got["x_untouched"]
