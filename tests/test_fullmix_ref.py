"""The long-double restatement of GaussianMixture and its tolerances, without a GPU: numpy's own fp64 evaluation meets every
formula on every input generator the GPU test uses (tests/test_gpu_fullmix.py), and each planted mutation lands at least 100
tolerances out on at least one of them - so a kernel that passes the GPU test has none of these faults."""
import numpy as np
import pytest

import fullmix_ref as R


@pytest.fixture(scope="module")
def cases():
    """(config, target, meta, rows, reference) of the whole grid, once."""
    out = []
    for cfg in R.grid():
        d, C, cond, kind, bounds, dtype, n = cfg
        t, meta = R.make_target(d, C, cond, seed=7, kind=kind, bounds=bounds)
        x = np.concatenate([R.make_rows(t, n, seed=11, dtype=dtype), R.special_rows(t, dtype)])
        out.append((cfg, t, meta, x, R.reference(t, x)))
    return out


def test_grid_covers_every_axis():
    g = R.grid()
    assert {c[0] for c in g} == set(R.DIMS) and {c[1] for c in g} == set(R.COMPONENTS)
    for d in R.DIMS:
        mine = [c for c in g if c[0] == d]
        assert {c[2] for c in mine} == {1.0, 1e6} and {c[4] for c in mine} == {False, True} and len({c[5] for c in mine}) == 2
    assert {c[3] for c in g} == set(R.KINDS)


def test_numpy_fp64_meets_every_tolerance(cases):
    worst_v = worst_g = 0.0
    for cfg, t, meta, x, ref in cases:
        v, g = R.numpy_fp64(t, x)
        wv, wg = R.compare(ref, v, g)
        assert wv < 1.0 and wg < 1.0, (cfg, wv, wg)
        wv2, _ = R.compare(ref, t(x))  # the class's own __call__
        assert wv2 < 1.0, (cfg, wv2)
        worst_v, worst_g = max(worst_v, wv), max(worst_g, wg)
    print(f"numpy fp64: worst value error {worst_v:.3f} tol, worst gradient error {worst_g:.3f} tol")


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_mutation_is_at_least_100_tolerances_out_somewhere(cases, mutation):
    worst = 0.0
    for cfg, t, meta, x, ref in cases:
        if mutation == "rPr" and not (cfg[3] == "plain" and cfg[2] == 1e6):
            continue
        if mutation != "swapped_bound":  # finite rows inside the box only: the distance is then a number, not a pattern
            keep = np.isfinite(ref["value"])
            x, ref = x[keep], {k: a[keep] for k, a in ref.items()}
        v, g = R.numpy_fp64(t, x, mutate=mutation, meta=meta)
        wv, wg = R.compare(ref, v, g)
        worst = max(worst, wv, wg)
    print(f"{mutation}: worst {worst:.3g} tolerances out")
    assert worst >= 100.0, (mutation, worst)
