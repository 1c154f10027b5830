"""The restatement of tests/moments_ref.py and its tolerance formulas, without a GPU: for every input generator of
tests/test_gpu_moments_density.py numpy's own fp64 evaluation stays inside the formulas (a correct fp64 kernel can meet them), each of
five plausible mistakes lands at least 100 x outside (they have teeth), the jitter ladder's expected counts sit far from rounding, and
the C oracle agrees with the restatement, non-finite rules included."""
import math

import mpmath
import numpy as np
import pytest
from scipy.special import logsumexp

import moments_ref as M

LD = M.LD

# (n, d, kind): every generator call of the GPU module's Gram and column-sum cases (an offset view reads the rows of its shape)
GRAM_D = sorted({32, 64, 128} | {1, 2, 3, 12, 31, 33, 48, 65, 100, 127} | {2, 12, 32, 4} | {48, 64, 100, 128, 36} | {1, 3, 33, 63, 7, 62})
POPULATIONS = ([(5003, d, "bulk") for d in GRAM_D] + [(n, 32, "bulk") for n in (1, 3, 4, 5, 31, 32, 33, 63, 64, 65)]
               + [(70001, 32, "bulk"), (70001, 64, "bulk"), (20001, 128, "bulk"), (65, 128, "bulk"), (65, 65, "bulk")]
               + [(5003, d, "offset") for d in (32, 48, 128)]
               + [(n, d, "bulk") for d in (1, 3, 32, 100, 128, 129, 200, 256) for n in (1, 7)] + [(5003, d, "bulk") for d in (129, 200, 256)])
POPULATIONS = list(dict.fromkeys(POPULATIONS))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,kind", POPULATIONS)
def test_numpy_moments_meet_the_tolerances(n, d, kind, f32):
    x = M.population(n, d, kind, f32=f32)
    assert np.abs(x).min() >= 0.5
    s, sa = M.colsum(x)
    M.compare(x.sum(0), s, M.tol_colsum(n, sa), f"numpy colsum {n}x{d} {kind}")
    c = M.centre(x)
    g, mag, s1 = M.centered_gram(x, c)
    M.compare((x - c).T @ (x - c), g, M.tol_gram(n, mag), f"numpy gram {n}x{d} {kind}")
    # mean_gram: the implementation's own centre (here numpy's sum / n), against the restatement around ITS centre
    c_ref = (s / LD(n)).astype(np.float64)
    g2, mag2, s12 = M.centered_gram(x, c_ref)
    M.compare((x - c).T @ (x - c), g2, M.tol_mean_gram(n, n, mag2, s12, sa), f"numpy mean_gram {n}x{d} {kind}")


def _mixture_f64(x, logw, mu, prec, premap=None):
    with np.errstate(all="ignore"):
        t = x if premap is None else M.premap_t(x, premap)
        terms = np.stack([lw - 0.5 * ((t - m) ** 2 * p).sum(1) for lw, m, p in zip(logw, mu, prec)])
        r = terms[0] if len(logw) == 1 else logsumexp(terms, axis=0)
        return r if premap is None else r + (premap[4] * t * t).sum(1)


MIXTURES = [(d, C) for d in (1, 2, 7, 32, 100, 256) for C in (1, 2, 4, 8)]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("d,C", MIXTURES)
def test_numpy_mixture_meets_the_tolerance(d, C, f32):
    for zw in (None, "one", "all"):
        logw, mu, prec = M.mixture_params(d, C, zero_weight=zw)
        x, nan_rows = M.mixture_rows(257, d, mu, prec, f32=f32)
        ref, mag, _ = M.mixture_logpdf(x, logw, mu, prec)
        assert np.isnan(ref[nan_rows].astype(np.float64)).all() and len(nan_rows) == 5
        assert np.isnan(ref.astype(np.float64)).sum() == 5  # no other row
        if zw is None:
            assert np.isfinite(ref[2:4].astype(np.float64)).all() and np.all(ref[2:4] < -1e7)  # the far rows stay finite
            assert np.all(np.isneginf(ref[4:6].astype(np.float64)))  # +-inf coordinates
        if zw == "all":
            assert np.all(np.isneginf(np.delete(ref.astype(np.float64), nan_rows)))
        M.compare(_mixture_f64(x, logw, mu, prec), ref, M.tol_mixture(d, mag, ref), f"numpy mixture d={d} C={C} {zw}")


@pytest.mark.parametrize("zero_h", [False, True], ids=["h", "h0"])
@pytest.mark.parametrize("d,C,f32", [(2, 1, False), (8, 4, False), (32, 2, False), (128, 4, False), (4, 2, True), (32, 4, True), (256, 1, True)])
def test_numpy_premapped_mixture_meets_the_tolerance(d, C, f32, zero_h):
    logw, mu, prec = M.mixture_params(d, C)
    pm = M.premap_table(d, zero_h=zero_h)
    x, nan_rows = M.mixture_rows(257, d, mu, prec, f32=f32, premap=pm)
    ref, mag, sens = M.mixture_logpdf(x, logw, mu, prec, premap=pm)
    assert np.isnan(ref[nan_rows].astype(np.float64)).all() and len(nan_rows) == 7
    t = M.premap_t(x, pm)
    on_lo, on_hi = 2 + 9, 2 + 10  # mixture_rows: the rows exactly on the clamp ends, then just beyond them
    bounded = np.isfinite(pm[2])
    assert np.all(t[on_lo][bounded] == -1.5) and np.all(t[on_hi][bounded] == 2.25)
    assert np.all(x[on_lo][bounded] * pm[0][bounded] + pm[1][bounded] == -1.5)  # on the end before the clamp, not behind it
    assert np.all(t[on_lo + 2][bounded] == -1.5) and np.all(t[on_hi + 2][bounded] == 2.25)
    assert np.all((x[on_lo + 2] * pm[0] + pm[1])[bounded] < -1.5)
    got = _mixture_f64(x, logw, mu, prec, pm)
    fin = np.isfinite(ref.astype(np.float64))  # (an infinite unbounded coordinate times h = 0: NaN by IEEE rules in both)
    assert fin.sum() >= 257 - 9
    M.compare(got, ref, M.tol_mixture(d, mag, ref, sens), f"numpy premap mixture d={d} C={C}")


def test_long_double_log_sum_exp_agrees_with_mpmath():
    d, C = 7, 4
    logw, mu, prec = M.mixture_params(d, C)
    pm = M.premap_table(d)
    x, _ = M.mixture_rows(40, d, mu, prec, premap=pm)
    ref, _, _ = M.mixture_logpdf(x, logw, mu, prec, premap=pm)
    mp = mpmath.mp.clone()
    mp.dps = 40
    t = M.premap_t(x, pm)
    for i in np.flatnonzero(np.isfinite(ref.astype(np.float64))):
        terms = [mp.mpf(float(logw[c])) - sum((mp.mpf(float(t[i, j])) - mp.mpf(float(mu[c, j]))) ** 2 * mp.mpf(float(prec[c, j]))
                                             for j in range(d)) / 2 for c in range(C)]
        val = mp.log(sum(mp.exp(v) for v in terms)) if max(terms) > -11000 else max(terms) + mp.log(sum(mp.exp(v - max(terms)) for v in terms))
        val += sum(mp.mpf(float(pm[4][j])) * mp.mpf(float(t[i, j])) ** 2 for j in range(d))
        hi = float(ref[i])
        got = mp.mpf(hi) + mp.mpf(float(ref[i] - LD(hi)))
        assert abs(got - val) <= abs(val) * mp.mpf(2) ** -60, (i, got, val)


def test_gaussian_logq_restatement():
    g = np.random.default_rng(5)
    for d in (1, 5, 32, 256):
        mu, sigma = np.linspace(-1, 1, d), np.linspace(0.5, 2, d)
        x = mu + sigma * g.normal(size=(50, d))
        ref, mag = M.gaussian_logq(x, mu, sigma)
        z = (x - mu) / sigma
        f64 = -0.5 * (z * z).sum(1) - np.log(sigma).sum() - 0.5 * d * np.log(2 * np.pi)
        M.compare(f64, ref, M.tol_mixture(d, mag, ref), f"numpy gaussian logq d={d}")


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,kind", [(5003, 32, "bulk"), (70001, 64, "bulk"), (5003, 48, "offset"), (5, 32, "bulk")])
def test_moment_mistakes_land_100_tolerances_out(n, d, kind):
    x = M.population(n, d, kind)
    s, sa = M.colsum(x)
    c = M.centre(x)
    g, mag, _ = M.centered_gram(x, c)
    r = n // 2
    dropped, doubled = np.delete(x, r, axis=0), np.concatenate([x, x[r:r + 1]])
    for name, y in (("one row dropped", dropped), ("one row counted twice", doubled)):
        w = M.worst(np.abs(y.sum(0).astype(LD) - s).astype(np.float64), M.tol_colsum(n, sa))
        wg = M.worst(np.abs(((y - c).T @ (y - c)).astype(LD) - g).astype(np.float64), M.tol_gram(n, mag))
        print(f"TEETH {name} {n}x{d} {kind}: colsum {w:.3g}, gram {wg:.3g} tolerances")
        assert w >= 100 and wg >= 100
    if kind == "offset":
        unc = x.T @ x - n * np.outer(c, c)
        wu = M.worst(np.abs(unc.astype(LD) - g).astype(np.float64), M.tol_gram(n, mag))
        print(f"TEETH uncentred form {n}x{d}: {wu:.3g} tolerances")
        assert wu >= 100


@pytest.mark.parametrize("d,C", [(2, 2), (32, 4), (128, 2)])
def test_density_mistakes_land_100_tolerances_out(d, C):
    logw, mu, prec = M.mixture_params(d, C)
    pm = M.premap_table(d)
    x, _ = M.mixture_rows(257, d, mu, prec, premap=pm)
    ref, mag, sens = M.mixture_logpdf(x, logw, mu, prec, premap=pm)
    fin = np.isfinite(ref.astype(np.float64))
    tol = M.tol_mixture(d, mag, ref, sens)
    a, b, lo, hi, h = pm
    wrong_end = _mixture_f64(x, logw, mu, prec, (a, b, np.where(np.isfinite(lo), hi, lo), hi, h))
    ref0, mag0, _ = M.mixture_logpdf(x, logw, mu, prec)
    no_weight = _mixture_f64(x, logw[:-1], mu[:-1], prec[:-1])
    fin0 = np.isfinite(ref0.astype(np.float64))
    with np.errstate(all="ignore"):
        w1 = M.worst(np.abs(wrong_end.astype(LD) - ref).astype(np.float64)[fin], tol[fin])
        w2 = M.worst(np.abs(no_weight.astype(LD) - ref0).astype(np.float64)[fin0], M.tol_mixture(d, mag0, ref0)[fin0])
    print(f"TEETH d={d} C={C}: upper clamp end for the lower one {w1:.3g}, one weight left out {w2:.3g} tolerances")
    assert w1 >= 100 and w2 >= 100


# ---- the reference fit ----------------------------------------------------------------------------------------------------------------
FIT_DIMS, N_MEAN, N_COV = M.FIT_DIMS, M.N_MEAN, M.N_COV


@pytest.mark.parametrize("d", FIT_DIMS)
def test_reference_fit_restatement_and_ladder_margins(d):
    cov = M.spd_with_condition(d, 1e10)
    mu, L, Li, tries, a = M.reference_fit(np.arange(1.0, d + 1), cov * (N_COV - 1), N_MEAN, N_COV)
    assert tries == 0 and np.array_equal(a.astype(np.float64), cov) and np.array_equal(a, cov.astype(LD))
    EL, ELi = M.fit_gaps(a)
    print(f"FIT d={d}: condition 1e10, E_L={EL:.3g} E_Linv={ELi:.3g}")
    assert float(np.abs((L @ L.T - a)).max()) <= d * 2.0**-60 * float(np.abs(a).max())
    assert float(np.abs(Li @ L - np.eye(d)).max()) <= d * 2.0**-50 * float(np.linalg.norm(Li.astype(np.float64)) * np.linalg.norm(L.astype(np.float64)))
    for lowest, want in ((-3e-7, 4), (-3e-3, 6)):
        sym = M.with_lowest_eigenvalue(d, lowest, relative=d > 1)  # (d = 1: the 1 x 1 matrix (lowest), whose scale is 1)
        _, L, _, tries, a = M.reference_fit(np.zeros(d), sym * (N_COV - 1), N_MEAN, N_COV)
        assert tries == want
        scale = float(np.trace(sym)) / d if d > 1 else 1.0
        ev = np.linalg.eigvalsh(sym).min() / scale
        assert abs(ev - lowest) <= 1e-3 * abs(lowest)
        # the try before is short of the eigenvalue by a factor of 30, the one that works clears it by a factor of 3.3: rounding
        # (1e-16 of the entries) is ten orders of magnitude away from both
        assert M.JITTERS[want - 1] < abs(lowest) / 29 and M.JITTERS[want] > 3.3 * abs(lowest)
        assert np.linalg.eigvalsh(sym + M.JITTERS[want - 1] * scale * np.eye(d)).min() < -0.9 * abs(lowest) * scale
        assert np.linalg.eigvalsh(sym + M.JITTERS[want] * scale * np.eye(d)).min() > 2 * abs(lowest) * scale
        assert np.array_equal(a, sym.astype(LD) + LD(M.JITTERS[want]) * M.jitter_scale(sym.astype(LD)) * np.eye(d, dtype=LD))


@pytest.mark.parametrize("d", FIT_DIMS)
def test_reference_fit_scale_and_failures(d):
    sym = M.all_negative(d)  # every eigenvalue in [-3e-7, -1e-7]: mean(diag) < 0, the scale is 1
    assert np.trace(sym) < 0
    _, L, _, tries, a = M.reference_fit(np.zeros(d), sym * (N_COV - 1), N_MEAN, N_COV)
    assert tries == 4 and np.array_equal(a, sym.astype(LD) + LD(1e-6) * np.eye(d, dtype=LD))
    bad = M.with_lowest_eigenvalue(d, -1e9, relative=False)
    assert np.linalg.eigvalsh(bad).min() < -9e8 and np.trace(bad) < 0  # (mean(diag) < 0: the scale is 1 here too)
    assert M.reference_fit(np.ones(d), bad * (N_COV - 1), N_MEAN, N_COV)[3] == -1  # the largest jitter, 1e8 x 1, is short of it
    inf = M.spd_with_condition(d, 10.0)
    inf[(1, 0) if d > 1 else (0, 0)] = inf[(0, 1) if d > 1 else (0, 0)] = np.inf
    mu, L, Li, tries, _ = M.reference_fit(np.ones(d), inf * (N_COV - 1), N_MEAN, N_COV)
    assert tries == -1 and L is None and np.all(np.isfinite(mu.astype(np.float64)))


# ---- the C oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,kind", [(5003, 32, "bulk"), (257, 100, "bulk"), (5003, 48, "offset")])
def test_oracle_moments_agree_with_the_restatement(oracle, n, d, kind):
    """orc_moments at the tolerances test_gpu_parity.py::test_moments_vs_oracle uses (1e-12 on the mean, 1e-10 + 1e-12 on the
    covariance), and inside this module's own formulas."""
    x = M.population(n, d, kind)
    mean, cov = oracle.moments(x)
    s, sa = M.colsum(x)
    np.testing.assert_allclose(mean, (s / n).astype(np.float64), rtol=1e-12)
    g, mag, s1 = M.centered_gram(x, mean)
    np.testing.assert_allclose(cov, (g / (n - 1)).astype(np.float64), rtol=1e-10, atol=1e-12)
    M.compare(mean * n, s, M.tol_colsum(n, sa) + M.ulp64(s), f"oracle colsum {n}x{d} {kind}")
    M.compare(cov * (n - 1), g, M.tol_gram(n, mag) + 2 * M.ulp64(g), f"oracle gram {n}x{d} {kind}")


@pytest.mark.parametrize("d,C", [(1, 1), (4, 2), (7, 3), (32, 4), (100, 8)])
def test_oracle_mixture_agrees_with_the_restatement_and_keeps_the_non_finite_contract(oracle, d, C):
    for zw in (None, "one", "all"):
        logw, mu, prec = M.mixture_params(d, C, zero_weight=zw)
        x, nan_rows = M.mixture_rows(120, d, mu, prec)
        ref, mag, _ = M.mixture_logpdf(x, logw, mu, prec)
        got = oracle.Mixture(logw, mu, prec).logpdf(x)
        assert M.same_nonfinite(got, ref.astype(np.float64)), (d, C, zw)
        assert np.isnan(got[nan_rows]).all() and np.isnan(got).sum() == len(nan_rows)  # NaN coordinate -> NaN, for every C
        assert np.all(np.isneginf(got[4:6]))  # +-inf coordinate: every term -inf -> -inf
        if zw == "all":
            assert np.all(np.isneginf(np.delete(got, nan_rows)))
        fin = np.isfinite(got)
        np.testing.assert_allclose(got[fin], ref[fin].astype(np.float64), rtol=1e-12, atol=1e-12)  # test_mixture_logpdf_vs_oracle's
        M.compare(got, ref, M.tol_mixture(d, mag, ref), f"oracle mixture d={d} C={C} {zw}")


def test_host_target_agrees_on_the_non_finite_contract():
    """The project's host evaluation of the same density (targets.py, torch.logsumexp): NaN for a NaN row, -inf for far rows."""
    import torch
    from aspire_amd.targets import DiagGaussianMixture

    d, C = 4, 3
    logw, mu, prec = M.mixture_params(d, C)
    x, nan_rows = M.mixture_rows(40, d, mu, prec)
    ref, _, _ = M.mixture_logpdf(x, logw, mu, prec)
    t = DiagGaussianMixture(mu, 1.0 / prec)
    t.logw = logw
    for got in (t(x), t(torch.as_tensor(x)).numpy()):
        assert M.same_nonfinite(got, ref.astype(np.float64))
        assert math.isnan(got[nan_rows[0]]) and np.all(np.isneginf(got[4:6]))
