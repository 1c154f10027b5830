"""The host restatement of the preconditioning transforms (tests/transform_ref.py) pinned on three sides before the device tests
(tests/test_gpu_transforms.py) lean on it: the real reference's recorded outputs (tests/golden/ref_transforms.npz), the C oracle, and a
literal table of what non-finite inputs map to.  Runs without a GPU."""
import math

import numpy as np
import pytest

import transform_ref as R

LD = np.longdouble
FTS = [pytest.param(np.float64, id="fp64"), pytest.param(LD, id="mpmath")]


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the reference's recorded outputs ---------------------------------------------------------------------------------------------
GOLDEN_CASES = ("mixed_logit_affine", "probit", "default_periodic", "logit_affine_d32", "probit_affine_periodic")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_golden(golden, name, ft):
    """Both runs against CompositeTransform's own forward / inverse outputs, at the tolerances of
    test_gpu_parity.py::test_transform_kernels_match_reference_golden (2e-10 on the inverse log-Jacobian covers the reference's
    cancellation in log1p(-u) next to u = 1, which the high-precision run does not share)."""
    g = golden["ref_transforms"]
    assert set(g["names"]) == set(GOLDEN_CASES)
    affine = bool(int(g[f"{name}_affine"]))
    tab = dict(kind=g[f"{name}_kind"], periodic=g[f"{name}_periodic"], lower=g[f"{name}_lower"], upper=g[f"{name}_upper"],
               mean=g[f"{name}_mean"] if affine else None, std=g[f"{name}_std"] if affine else None, eps=1e-6)
    z, lj, _ = R.composite(g[f"{name}_x"], **tab, ft=ft)
    np.testing.assert_allclose(_f64(z), g[f"{name}_z"], rtol=1e-12, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(_f64(lj), g[f"{name}_lj"], rtol=1e-12, atol=1e-11, err_msg=name)
    x2, lj2, _ = R.composite(g[f"{name}_z2"], **tab, inverse=True, ft=ft)
    np.testing.assert_allclose(_f64(x2), g[f"{name}_x2"], rtol=1e-12, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(_f64(lj2), g[f"{name}_lj2"], rtol=1e-12, atol=2e-10, err_msg=name)
    if ft is np.float64 and not (tab["kind"] == 1).any():  # the reference's own arithmetic: the same bits where no libm-dependent
        np.testing.assert_array_equal(lj2, g[f"{name}_lj2"])  # log / log1p enters (probit's Jacobian is plain arithmetic)


# ---- the C oracle -----------------------------------------------------------------------------------------------------------------
TABLES = ("none", "affine", "periodic", "logit", "probit", "logit_affine", "probit_affine", "logit_mix", "probit_mix")


@pytest.mark.parametrize("d", [1, 3, 8, 33])
@pytest.mark.parametrize("name", TABLES)
def test_fp64_run_agrees_with_the_oracle_on_the_interior(oracle, name, d):
    """1e-13 relative, both directions: purely relative wherever the last stage that touches a coordinate cannot cancel (forward
    without the affine stage; coordinates the inverse leaves alone).  Where it can - (v - mean) / std forward, w u + lower,
    lower + mod(.) and v std + mean inverse - numpy's and libm's log differ by an ulp of the operand, which the difference keeps,
    so `relative` is there to the larger of the value and the operands of that subtraction or addition.  (Measured purely
    relative: at most 2.9e-14 without the affine forward stage; 1.2e-13, 3.2e-13 and 2.3e-12 for logit_affine, probit_mix and
    probit_affine forward.)"""
    tab = R.table(name, d)
    kind, per, lo, up, mean, std = tab
    for inverse in (False, True):
        x = R.interior_x(tab, 257, inverse)
        y, lj, _ = R.composite(x, *tab, R.EPS, inverse)
        yo, ljo = oracle.transform(x, *tab, R.EPS, inverse=inverse)
        scale = np.zeros(d)  # 0: purely relative
        if not inverse and mean is not None:
            scale = (1.0 + np.abs(mean)) / np.abs(std)
        elif inverse:
            scale = np.where((kind != 0) | (per != 0), np.maximum(np.abs(lo), np.abs(up)), 0.0 if mean is None else 1.0 + np.abs(mean))
        gap = np.abs(y - yo) / np.maximum(np.maximum(np.abs(yo), scale), 5e-324)
        assert np.all(gap <= 1e-13), float(gap.max())
        np.testing.assert_allclose(lj, ljo, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("d", [6, 8])
def test_edge_sets_have_the_oracles_nonfinite_pattern(oracle, d):
    """On every edge set of the device tests the fp64 run, the high-precision run and the oracle put NaN and +-inf in the same
    places (values and row Jacobians), so that any of the three can judge a kernel's non-finite pattern."""
    for name, (tab, x, inverse) in R.edge_cases(d).items():
        y, lj, _ = R.composite(x, *tab, R.EPS, inverse)
        yo, ljo = oracle.transform(x, *tab, R.EPS, inverse=inverse)
        assert R.same_nonfinite(y, yo) and R.same_nonfinite(lj, ljo), name
        if "nonfinite" in name:
            yh, ljh, _ = R.composite(x[:48], *tab, R.EPS, inverse, ft=LD)
            assert R.same_nonfinite(yh, y[:48]) and R.same_nonfinite(ljh, lj[:48]), name
            assert not np.isfinite(y).all(), name


def test_high_precision_run_is_close_to_the_fp64_run_where_the_expression_is_well_conditioned():
    """Interior points: the two runs differ by the rounding of a handful of fp64 operations, which also shows that the mpmath
    plumbing (long double <-> mpf) loses nothing."""
    for name in ("logit", "probit", "periodic", "affine"):
        tab = R.table(name, 4, bounds=((-3.0, 2.5),))  # (an interval at 1e6 would put x - lower's rounding at 1e-10 relative)
        for inverse in (False, True):
            x = R.interior_x(tab, 40, inverse)
            y, lj, t = R.composite(x, *tab, R.EPS, inverse)
            yh, ljh, th = R.composite(x, *tab, R.EPS, inverse, ft=LD)
            assert yh.dtype == LD and th.dtype == LD
            np.testing.assert_allclose(y, _f64(yh), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(lj, _f64(ljh), rtol=1e-13)
            # long double really carries more than fp64: the identity element of the check above
            assert np.any(yh != _f64(yh).astype(LD)) or name in ("periodic",)


# ---- non-finite inputs: the semantics, written down once ---------------------------------------------------------------------------
EPS = 1e-6
C_LO, C_HI = EPS, 1.0 - EPS  # the clamp ends, fp64
LOGIT_LO = math.log(C_LO) - math.log1p(-C_LO)  # -13.815509557963773
LOGIT_HI = math.log(C_HI) - math.log1p(-C_HI)
LOGIT_LJ_LO = math.log(C_LO) + math.log1p(-C_LO)  # the inverse's term at the clamped ends; the forward's is its negative
LOGIT_LJ_HI = math.log(C_HI) + math.log1p(-C_HI)
# sqrt(2) erfinv(y) at the clamp ends y = fl(2 fl(1 - eps) - 1) and fl(2 eps - 1): fp64 by definition (erfinv amplifies the rounding of
# 2 u - 1 next to -1 by 1e5: the true probit of eps is -4.7534243088229)
PROBIT_HI, PROBIT_LO = 4.753424308817088, -4.753424308828307
LO, UP = -3.0, 2.5
W = UP - LO
nan, inf = math.nan, math.inf


def _one(kind, periodic, v, inverse, mean=None, std=None, ft=np.float64):
    m, s = (None, None) if mean is None else ([mean], [std])
    y, lj, _ = R.composite([[v]], [kind], [periodic], [LO], [UP], m, s, EPS, inverse, ft=ft)
    return float(y[0, 0]), float(lj[0])


def _same(a, b, rtol=4e-16):
    return (math.isnan(a) and math.isnan(b)) or a == b or (math.isfinite(b) and abs(a - b) <= rtol * abs(b))


FORWARD = [
    # kind, periodic, mean, std, x -> value, row log|det J|
    (1, 0, None, None, nan, nan, nan),
    (2, 0, None, None, nan, nan, nan),
    (0, 1, None, None, nan, nan, 0.0),
    (0, 0, None, None, nan, nan, 0.0),
    (0, 0, 0.5, 2.0, nan, nan, -math.log(2.0)),
    (1, 0, None, None, inf, LOGIT_HI, -LOGIT_LJ_HI - math.log(W)),  # a bounded coordinate: the clamp end on the same side
    (1, 0, None, None, -inf, LOGIT_LO, -LOGIT_LJ_LO - math.log(W)),
    (2, 0, None, None, inf, PROBIT_HI, 0.5 * (math.log(2 * math.pi) + PROBIT_HI**2) - math.log(W)),
    (2, 0, None, None, -inf, PROBIT_LO, 0.5 * (math.log(2 * math.pi) + PROBIT_LO**2) - math.log(W)),
    (0, 1, None, None, inf, nan, 0.0),  # periodic: fmod(inf, w) is NaN
    (0, 1, None, None, -inf, nan, 0.0),
    (0, 0, 0.5, 2.0, inf, inf, -math.log(2.0)),  # untouched + affine: the sign follows std
    (0, 0, 0.5, -2.0, inf, -inf, -math.log(2.0)),
    (0, 0, 0.5, -2.0, -inf, inf, -math.log(2.0)),
    (0, 0, None, None, -inf, -inf, 0.0),
]
INVERSE = [
    (1, 0, None, None, nan, nan, nan),
    (2, 0, None, None, nan, nan, nan),
    (0, 1, None, None, nan, nan, 0.0),
    (0, 0, 0.5, 2.0, nan, nan, math.log(2.0)),
    (1, 0, None, None, inf, W * C_HI + LO, LOGIT_LJ_HI + math.log(W)),  # logit: the clamped end, with the clamp's Jacobian
    (1, 0, None, None, -inf, W * C_LO + LO, LOGIT_LJ_LO + math.log(W)),
    (2, 0, None, None, inf, UP, -inf),  # probit: erf reaches +-1, the density term is -inf
    (2, 0, None, None, -inf, LO, -inf),
    (1, 0, 0.5, -2.0, inf, W * C_LO + LO, LOGIT_LJ_LO + math.log(W) + math.log(2.0)),  # the affine stage in front flips the side
    (0, 1, None, None, inf, nan, 0.0),
    (0, 0, 0.5, -2.0, inf, -inf, math.log(2.0)),
]


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("inverse,row", [(False, r) for r in FORWARD] + [(True, r) for r in INVERSE])
def test_nonfinite_inputs_map_as_tabulated(inverse, row, ft):
    kind, periodic, mean, std, v, want, want_lj = row
    got, got_lj = _one(kind, periodic, v, inverse, mean, std, ft)
    rtol = 2e-15 if kind == 2 and not inverse else 4e-16  # (scipy's erfinv against mpmath's)
    assert _same(got, want, rtol) and _same(got_lj, want_lj, rtol), (row, got, got_lj)


def test_the_tabulated_constants():
    """The literals of the table above, from mpmath."""
    mp = R._MP
    assert LOGIT_LO == pytest.approx(-13.815509557963773, rel=1e-15)
    assert float(mp.sqrt(2) * mp.erfinv(1 - 2 * mp.mpf(EPS))) == pytest.approx(PROBIT_HI, rel=1e-9)
    # the two clamp ends carry different Jacobian constants: fl(1 - eps) is not 1 - eps
    u = mp.mpf(C_HI)
    assert float(mp.log(u) + mp.log1p(-u)) == pytest.approx(LOGIT_LJ_HI, rel=1e-15)
    assert abs(LOGIT_LJ_HI - LOGIT_LJ_LO) == pytest.approx(2.9e-11, rel=0.05)
