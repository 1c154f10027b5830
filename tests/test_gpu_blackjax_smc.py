"""The random-walk and HMC kernels of the "blackjax_smc" sampler on the HIP engine (csrc/asmc_hmc.hip; include/asmc.h asmc_rw_* /
asmc_mh_* / asmc_hmc_*).

* k_rw_propose / k_mh_accept / k_hmc_accept against tests/hmc_ref.py: proposals to the fp64 noise-parity tolerance of
  tests/test_gpu_parity.py (rtol 1e-12, atol 1e-13; fp32 state: one rounding), decisions restated from the device's own proposals
  and therefore exact, rejected rows bit-identical, counts;
* k_hmc_mix, one transition: dH against the restatement within 8 x |fp64 - long double| of the restatement on that case plus 64 ulp
  of the larger energy (largest tolerance over the grid as measured: see DESIGN.md §3.13), decisions restated from the device's dH,
  end points, carried densities against `mixture_logpdf`, a second run bit for bit;
* several transitions in one launch = the same transitions launched one by one, bit for bit (the register-carry path);
* the integrator's order (mean |dH| falls 4x when the step halves) and stationarity on a Gaussian to exact 5-sigma bounds;
* the split path (torch.autograd gradients) against the fused kernel on the same mixtures;
* end to end through `Aspire(...).sample_posterior(sampler="blackjax_smc")`: log Z against (d/2) log pi, torch callables, a trained
  coupling-flow proposal, bounded_to_unbounded, the likelihood hole of tests/test_gpu_hole.py under both algorithms.
Specification: reference src/aspire/samplers/smc/blackjax.py:13-349.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hmc_ref as H

pytestmark = pytest.mark.gpu

NS, DS = (7, 257, 4097), (1, 2, 7, 32, 33, 128)
GRID = [(n, d) for n in NS for d in DS]
GRID_IDS = [f"n{n}-d{d}" for n, d in GRID]


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


def _dev(eng, a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=eng.device, dtype=dtype)


def _densities(y64):
    """(ll, lp, lq) of rows (host fp64): a quadratic target with a hole of -inf / NaN in a few rows."""
    q = (y64 * y64).sum(1)
    ll = -0.5 * q
    lp = -0.1 * y64[:, 0]
    lq = -0.25 * q
    with np.errstate(invalid="ignore"):
        ll[(np.arange(len(q)) % 97) == 5] = -np.inf
        lq[(np.arange(len(q)) % 89) == 7] = np.nan
    return ll, lp, lq


@pytest.mark.parametrize("n,d", GRID, ids=GRID_IDS)
def test_rw_propose_and_mh_accept_against_the_restatement(eng, n, d):
    """Three sigma forms x two state dtypes, two steps each (the second step starts from the first one's accepts)."""
    g = np.random.default_rng(1000 * n + d)
    A = g.normal(size=(d, d)) / math.sqrt(d)
    forms = {"scalar": 0.3, "diag": g.uniform(0.1, 0.5, size=d), "tril": np.linalg.cholesky(0.04 * (A @ A.T + np.eye(d)))}
    seed, gid0, beta = 0x0FEDCBA987654321, (1 << 32) - 5, 0.6
    for name, sigma in forms.items():
        for tdt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            x = g.normal(size=(n, d)).astype(npdt)
            ll, lp, lq = _densities(x.astype(np.float64))
            logj = g.normal(size=n) if name == "diag" else None  # one family with a preconditioning log-Jacobian
            xd = _dev(eng, x, tdt)
            lld, lpd, lqd = (_dev(eng, a.copy()) for a in (ll, lp, lq))
            ljd = None if logj is None else _dev(eng, logj.copy())
            sig_d = sigma if name == "scalar" else _dev(eng, sigma)
            total = 0
            for step in (3, 4):
                y = eng.rw_propose(xd, sig_d, seed, gid0, step, 1)
                y_h = y.cpu().numpy()
                y_ref = H.rw_propose(x, sigma, seed, gid0, step)
                assert y_h.dtype == npdt
                if npdt is np.float64:
                    np.testing.assert_allclose(y_h, y_ref, rtol=1e-12, atol=1e-13)
                else:  # the fp64 sum rounded once to fp32: at most one fp32 ulp from the restatement's rounding
                    assert np.all(np.abs(y_h - y_ref) <= np.spacing(np.abs(y_ref)))
                lln, lpn, lqn = _densities(y_h.astype(np.float64))
                ljn = None if logj is None else g.normal(size=n)
                x_before = x.copy()
                eng.mh_accept(xd, y, beta, lld, lpd, lqd, *(_dev(eng, v.copy()) for v in (lln, lpn, lqn)), seed, gid0, step, 1, logj=ljd,
                              logj_new=None if ljn is None else _dev(eng, ljn))
                acc = H.mh_accept(x, y_h, beta, ll, lp, lq, lln, lpn, lqn, seed, gid0, step, logj=logj, logj_new=ljn)
                assert np.array_equal(x[~acc], x_before[~acc])
                assert np.array_equal(xd.cpu().numpy(), x), f"{name} {npdt.__name__} step {step}: state differs"
                for dev, ref in ((lld, ll), (lpd, lp), (lqd, lq)) + (((ljd, logj),) if logj is not None else ()):
                    np.testing.assert_array_equal(dev.cpu().numpy(), ref)
                # rw_propose opens the counter of its step index: the count is this step's alone
                assert int(eng.mh_counts(2)[1]) == int(acc.sum())
                total += int(acc.sum())
            assert 0 <= total <= 2 * n and (total > 0 or n < 8)


@pytest.mark.parametrize("n,d", [(7, 1), (257, 7), (4097, 33), (4097, 128)])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_hmc_momentum_leap_and_accept_against_the_restatement(eng, n, d, dt):
    """The split path's launches, with a NaN / inf hole in the proposed densities and NaN momenta (a divergent trajectory)."""
    tdt, npdt = (torch.float64, np.float64) if dt == "f64" else (torch.float32, np.float32)
    g = np.random.default_rng(n + d)
    seed, gid0, step, beta = 77, 123456789, 9, 0.45
    minv = g.uniform(0.5, 2.0, size=d)
    for mass in (None, minv):
        md = None if mass is None else _dev(eng, mass)
        p0 = eng.hmc_momentum(n, d, md, seed, gid0, step, 0)
        p_ref = H.momenta(seed, gid0, n, step, d, mass)
        np.testing.assert_allclose(p0.cpu().numpy(), p_ref, rtol=1e-12, atol=1e-13)
        x = g.normal(size=(n, d)).astype(npdt)
        z, grad = x.astype(np.float64), g.normal(size=(n, d))
        zd, pd = _dev(eng, z), p0.clone()
        eng.hmc_leap(zd, pd, _dev(eng, grad), md, 0.05, 0.1)
        p0_h = p0.cpu().numpy()
        z_ref, p1_ref = H.leap(z, p0_h, grad, mass, 0.05, 0.1)
        np.testing.assert_allclose(pd.cpu().numpy(), p1_ref, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(zd.cpu().numpy(), z_ref, rtol=1e-14, atol=1e-15)
        z_h, p1_h = zd.cpu().numpy(), pd.cpu().numpy()
        if n > 8:
            p1_h[3] = np.nan
            pd = _dev(eng, p1_h)
        ll, lp, lq = _densities(z)
        lln, lpn, lqn = _densities(z_h)
        lln[1::5] = np.inf
        xd = _dev(eng, x, tdt)
        lld, lpd, lqd = (_dev(eng, a.copy()) for a in (ll, lp, lq))
        flags, dH = eng.hmc_accept(xd, zd, p0, pd, md, beta, lld, lpd, lqd, *(_dev(eng, v) for v in (lln, lpn, lqn)), seed, gid0, step, 0,
                                   want_dH=True)
        dH_h = dH.cpu().numpy()
        _, dH_ref = H.hmc_accept(x.copy(), z_h, p0_h, p1_h, mass, beta, ll.copy(), lp.copy(), lq.copy(), lln, lpn, lqn, seed, gid0, step)
        fin = np.isfinite(dH_ref)
        assert np.array_equal(np.isnan(dH_h), np.isnan(dH_ref)) and np.array_equal(dH_h[~fin & ~np.isnan(dH_ref)], dH_ref[~fin & ~np.isnan(dH_ref)])
        np.testing.assert_allclose(dH_h[fin], dH_ref[fin], rtol=1e-13, atol=1e-13 * d)
        acc = H.hmc_decide(dH_h, seed, gid0, step)  # restated from the device's own dH: exact
        assert np.array_equal(flags.cpu().numpy(), acc) and not acc[1::5].any() and (n <= 8 or not acc[3])
        x_ref = x.copy()
        x_ref[acc] = z_h[acc].astype(npdt)
        assert np.array_equal(xd.cpu().numpy(), x_ref)
        for dev, old, new in ((lld, ll, lln), (lpd, lp, lpn), (lqd, lq, lqn)):
            np.testing.assert_array_equal(dev.cpu().numpy(), np.where(acc, new, old))
        assert int(eng.mh_counts(1)[0]) == int(acc.sum())


# (C of the likelihood, num_integration_steps, diagonal mass?, beta): every level of every factor, prior and proposal Gaussian
DESIGN = [(1, 1, False, 1.0), (3, 10, True, 0.3), (8, 10, False, 0.3), (8, 1, True, 1.0)]
MAX_TOL = {}  # the largest dH tolerance each case allowed itself (printed; DESIGN.md §3.13 quotes the run's maximum)


def _mix_case(eng, n, d, C, seed):
    g = np.random.default_rng(seed)
    mixes = [H.random_mixture(g, C, d, spread=1.0), H.random_mixture(g, 1, d, spread=0.3), H.random_mixture(g, 1, d, spread=0.3)]
    x = g.normal(size=(n, d))
    dm = [eng.make_mixture(*m) for m in mixes]
    xd = _dev(eng, x)
    dens = [eng.mixture_logpdf(xd, m) for m in dm]
    return mixes, x, dm, xd, dens, g.uniform(0.5, 2.0, size=d)


@pytest.mark.parametrize("C,n_leap,diag,beta", DESIGN, ids=[f"C{c}-L{L}-{'diag' if m else 'unit'}-b{b}" for c, L, m, b in DESIGN])
@pytest.mark.parametrize("n,d", GRID, ids=GRID_IDS)
def test_hmc_mix_one_transition_against_the_restatement(eng, n, d, C, n_leap, diag, beta):
    """dH within 8 x max |dH_fp64 - dH_longdouble| of the restatement on this case + 64 ulp of the larger energy (largest tolerance
    over the grid on MI355X: 9.3e-12, at n = 4097, d = 128, C = 1, one step; largest device error there: 3.4e-13); decisions restated from the device's dH: exact."""
    mixes, x, dm, xd, dens, minv = _mix_case(eng, n, d, C, 31 * n + d + C)
    mass = minv if diag else None
    md = None if mass is None else _dev(eng, mass)
    seed, gid0, step = 0x5EED5EED5EED, (1 << 32) - 2, 6
    eps = 0.4 / math.sqrt(d)  # acceptance well inside (0, 1) at every d
    lld, lpd, lqd = (v.clone() for v in dens)
    dH = eng.hmc_mix(xd, lld, lpd, lqd, beta, *dm, md, eps, n_leap, seed, gid0, step, 1, 0, want_dH=True)
    dH_h = dH.cpu().numpy()
    r, tol, tol_x, gap = H.dh_tolerance(mixes, beta, x, eps, n_leap, mass, seed, gid0, step)
    MAX_TOL[(n, d, C, n_leap)] = float(tol.max())
    err = np.abs(dH_h - r["dH"])
    print(f"hmc_mix n={n} d={d} C={C} L={n_leap}: max |dH dev - ref| {err.max():.3e}, tolerance {tol.max():.3e} (fp64 vs long double {gap:.3e})")
    assert np.all(err <= tol), (err.max(), tol.max())
    acc = H.hmc_decide(dH_h, seed, gid0, step)
    assert int(eng.mh_counts(1)[0]) == int(acc.sum())
    got = xd.cpu().numpy()
    assert np.array_equal(got[~acc], x[~acc])  # rejected rows: bit-identical, and so are their carried densities
    for dev, old in zip((lld, lpd, lqd), dens):
        assert torch.equal(dev[torch.from_numpy(~acc).to(eng.device)], old[torch.from_numpy(~acc).to(eng.device)])
    assert np.all(np.abs(got[acc] - r["x"][acc]).max(axis=1) <= tol_x[acc]) if acc.any() else True
    for dev, m in zip((lld, lpd, lqd), dm):  # every row's carried densities are the densities of the stored row
        torch.testing.assert_close(dev, eng.mixture_logpdf(xd, m), rtol=1e-12, atol=1e-12)
    assert 0 < acc.sum() or n < 8
    # a second run: identical bits
    xd2, l2 = _dev(eng, x), [v.clone() for v in dens]
    dH2 = eng.hmc_mix(xd2, *l2, beta, *dm, md, eps, n_leap, seed, gid0, step, 1, 0, want_dH=True)
    assert torch.equal(dH2, dH) and torch.equal(xd2, xd) and all(torch.equal(a, b) for a, b in zip(l2, (lld, lpd, lqd)))


def test_transitions_in_one_launch_equal_transitions_launched_one_by_one(eng):
    n, d, steps = 257, 7, 5
    mixes, x, dm, xd, dens, minv = _mix_case(eng, n, d, 3, 5)
    md = _dev(eng, minv)
    a = [xd.clone()] + [v.clone() for v in dens]
    b = [xd.clone()] + [v.clone() for v in dens]
    dHa = eng.hmc_mix(*a, 0.5, *dm, md, 0.15, 4, 99, 1000, 10, steps, 0, want_dH=True)
    ca = eng.mh_counts(steps)
    cb = []
    for s in range(steps):
        dHb = eng.hmc_mix(*b, 0.5, *dm, md, 0.15, 4, 99, 1000, 10 + s, 1, 0, want_dH=True)
        cb.append(int(eng.mh_counts(1)[0]))
    assert ca.tolist() == cb and 0 < sum(cb) < n * steps
    assert torch.equal(dHa, dHb) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[0], xd)


def _gaussian_target(eng, d, var):
    """ll = N(0, diag var) un-normalised, a flat prior (precision 1e-30) and, at beta = 1, an idle proposal."""
    ll = eng.make_mixture([0.0], np.zeros((1, d)), (1.0 / np.asarray(var))[None])
    flat = eng.make_mixture([0.0], np.zeros((1, d)), np.full((1, d), 1e-30))
    return ll, flat, flat


def test_order_of_the_integrator(eng):
    """Same seed, trajectory length 1, N(0, I): halving the step divides the mean |dH| by 4 (second order)."""
    n, d = 100_000, 8
    x = np.random.default_rng(8).normal(size=(n, d))
    mixes = _gaussian_target(eng, d, np.ones(d))
    mean_abs = []
    for eps, L in ((0.1, 10), (0.05, 20)):
        xd = _dev(eng, x)
        zero = [torch.zeros(n, dtype=torch.float64, device=eng.device) for _ in range(3)]
        dH = eng.hmc_mix(xd, *zero, 1.0, *mixes, None, eps, L, 2024, 0, 0, 1, 0, want_dH=True)
        mean_abs.append(float(dH.abs().mean()))
    ratio = mean_abs[0] / mean_abs[1]
    print(f"mean |dH|: {mean_abs[0]:.3e} at step 0.1, {mean_abs[1]:.3e} at step 0.05, ratio {ratio:.3f}")
    assert 3.0 <= ratio <= 5.0


def test_stationarity_on_a_gaussian(eng):
    """Exact draws of N(0, diag v), 50 transitions: the particles are independent chains, each still distributed as the target, so
    the bounds are exact 5-sigma bounds of a sample of n."""
    n, d = 200_000, 8
    v = np.linspace(0.5, 2.0, d)
    x = np.random.default_rng(9).normal(size=(n, d)) * np.sqrt(v)
    xd = _dev(eng, x)
    zero = [torch.zeros(n, dtype=torch.float64, device=eng.device) for _ in range(3)]
    eng.hmc_mix(xd, *zero, 1.0, *_gaussian_target(eng, d, v), None, 0.35, 4, 31337, 0, 0, 50, 0)
    counts = eng.mh_counts(50)
    acc = counts.sum() / (50 * n)
    got = xd.cpu().numpy()
    assert 0.6 < acc < 0.999 and not np.array_equal(got, x)
    mean, var = got.mean(axis=0), got.var(axis=0, ddof=1)
    print(f"stationarity: acceptance {acc:.3f}, max |mean| / sigma {np.max(np.abs(mean) / np.sqrt(v / n)):.2f}, "
          f"max |var - v| / sigma {np.max(np.abs(var - v) / (v * math.sqrt(2.0 / (n - 1)))):.2f}")
    assert np.all(np.abs(mean) <= 5.0 * np.sqrt(v / n))
    assert np.all(np.abs(var - v) <= 5.0 * v * math.sqrt(2.0 / (n - 1)))


def test_split_path_against_fused_path(eng):
    """The mixtures of hmc_ref.split_fused_case as built-ins (fused kernel) and wrapped as torch lambdas (autograd gradients between
    the split launches): one transition, n = 4097, d = 7."""
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.history import SMCHistory
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    mixes, x, beta, eps, n_leap, seed = H.split_fused_case()
    n, d = x.shape
    (lw, mu, pr), (plw, pmu, ppr), (_, qmu, qpr) = mixes
    lik = DiagGaussianMixture(mu, 1.0 / pr, weights=[0.2, 0.3, 0.5])
    prior = DiagGaussianMixture(pmu, 1.0 / ppr)
    np.testing.assert_allclose(lik.logw, lw, rtol=1e-13)
    r, tol, _, _ = H.dh_tolerance(mixes, beta, x, eps, n_leap, None, seed, 0, 0)
    out = {}
    for name, (fl, fp, xp) in {"fused": (lik, prior, np), "split": (lambda s: lik(s.x), lambda s: prior(s.x), torch)}.items():
        flow = GaussianFlow(d, mu=qmu[0], sigma=1.0 / np.sqrt(qpr[0]), engine=eng, seed=1)
        sp = HipBlackJAXSMC(log_likelihood=fl, log_prior=fp, dims=d, prior_flow=flow, xp=xp, engine=eng, rng=np.random.default_rng(0))
        sp.sampler_kwargs = {"algorithm": "hmc", "step_size": eps, "num_integration_steps": n_leap, "n_steps": 1}
        sp.key, sp._minv, sp.record_dH, sp.history = 42, None, True, SMCHistory()
        xd = _dev(eng, x)
        dm = [eng.make_mixture(*m) for m in mixes]
        parts = sp._wrap(xd, *(eng.mixture_logpdf(xd, m) for m in dm), beta)
        new = sp.mutate(parts, beta)
        assert name in sp.last_mutation_path
        out[name] = (sp.last_dH.cpu().numpy(), new.x.cpu().numpy(), sp.history.mcmc_acceptance[-1])
    for name in out:
        assert np.all(np.abs(out[name][0] - r["dH"]) <= tol), name
    assert np.all(np.abs(out["fused"][0] - out["split"][0]) <= tol)
    with np.errstate(all="ignore"):
        near = np.abs(r["dH"] - np.log(H.accept_uniforms(seed, 0, n, 0))) < tol
    moved = {k: np.any(v[1] != x, axis=1) for k, v in out.items()}
    assert int(near.sum()) <= 2 and np.array_equal(moved["fused"][~near], moved["split"][~near])
    assert np.array_equal(moved["fused"][~near], H.hmc_decide(r["dH"], seed, 0, 0)[~near])
    assert 0.3 < out["fused"][2] < 1.0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _run(eng, d, n, seed, sampler_kwargs, xp=np, lik=None, flow_backend="gaussian", sample_kw=None, **kw):
    from aspire_amd import Aspire, Samples
    from aspire_amd.targets import DiagGaussianMixture

    lik = lik or DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend=flow_backend, engine=eng, seed=seed, xp=xp, **kw)
    aspire.fit(Samples(1.5 * np.random.default_rng(seed).normal(size=(5000, d))), **({"n_epochs": 8} if flow_backend != "gaussian" else {}))
    out, hist = aspire.sample_posterior(sampler="blackjax_smc", n_samples=n, engine=eng, rng=np.random.default_rng(1000 + seed),
                                        rng_key=seed, sampler_kwargs=sampler_kwargs, store_sample_history=False, return_history=True,
                                        **(sample_kw or {}))
    return aspire, out, hist


def test_hmc_logz_d8_eight_seeds(eng):
    d, true = 8, 4.0 * math.log(math.pi)
    z = []
    for s in range(8):
        aspire, out, hist = _run(eng, d, 50_000, s, {"step_size": 0.3, "num_integration_steps": 5, "n_steps": 8})
        z.append((float(out.log_evidence) - true) / float(out.log_evidence_error))
        assert hist.beta[-1] == 1.0 and len(hist.mcmc_acceptance) == len(hist.beta) and "fused" in aspire.sampler.last_mutation_path
    z = np.array(z)
    print(f"blackjax_smc hmc d=8 N=50000 z-scores: {np.round(z, 2).tolist()}")
    assert abs(z.mean()) <= 1.0 and np.sqrt((z**2).mean()) <= 1.6, z


def _tlik(smp):
    return -0.5 * (smp.x * smp.x).sum(1)


def test_rwmh_torch_callables_coupling_flow_and_bounded(eng):
    d, true = 8, 4.0 * math.log(math.pi)
    kw = {"algorithm": "rwmh", "sigma": 0.35, "n_steps": 30}
    _, out, _ = _run(eng, d, 50_000, 5, kw, xp=torch, lik=_tlik)
    assert abs(float(out.log_evidence) - true) <= 4 * float(out.log_evidence_error) + 0.02
    aspire, out, _ = _run(eng, d, 50_000, 6, kw, flow_backend="coupling")
    assert "rwmh split" in aspire.sampler.last_mutation_path
    assert abs(float(out.log_evidence) - true) <= 4 * float(out.log_evidence_error) + 0.02
    params = [f"x_{i}" for i in range(d)]
    aspire, out, _ = _run(eng, d, 50_000, 7, dict(kw, sigma=0.05), parameters=params, prior_bounds={p: [-10.0, 10.0] for p in params},
                          bounded_to_unbounded=True, sample_kw={"preconditioning_kwargs": {"bounded_to_unbounded": True}})
    assert "CompositeTransform" in type(aspire.sampler.preconditioning_transform).__name__
    x = np.asarray(out.x)
    assert np.all(np.abs(x) < 10.0) and abs(float(out.log_evidence) - true) <= 4 * float(out.log_evidence_error) + 0.02


def test_hmc_split_with_a_coupling_flow_and_torch_callables(eng):
    d, true = 8, 4.0 * math.log(math.pi)
    aspire, out, hist = _run(eng, d, 20_000, 8, {"step_size": 0.3, "num_integration_steps": 5, "n_steps": 4}, xp=torch, lik=_tlik,
                             flow_backend="coupling")
    assert "hmc split" in aspire.sampler.last_mutation_path and all(0.3 < a <= 1.0 for a in hist.mcmc_acceptance)
    assert abs(float(out.log_evidence) - true) <= 4 * float(out.log_evidence_error) + 0.02


@pytest.mark.parametrize("algorithm", ["rwmh", "hmc"])
@pytest.mark.parametrize("value", [-np.inf, np.nan, np.inf], ids=["-inf", "nan", "+inf"])
def test_likelihood_hole(eng, value, algorithm):
    """tests/test_gpu_hole.py's problem; HMC takes gradients, so it gets the same construction in torch."""
    from test_likelihood_hole import check_hole_run, hole_problem

    from aspire_amd import Aspire, Samples

    d, n, seed = 2, 4000, 21
    log_like, log_prior = hole_problem(value, d)
    xp, kw = np, {"algorithm": "rwmh", "sigma": 0.8, "n_steps": 10}
    if algorithm == "hmc":
        xp, kw = torch, {"algorithm": "hmc", "step_size": 0.9, "num_integration_steps": 3, "n_steps": 5}

        def log_like(samples):  # noqa: F811
            x = samples.x.to(torch.float64)
            logl = (math.log(1.0 / math.sqrt(2 * math.pi)) - 0.5 * (x - 2.0) ** 2).sum(-1)
            return torch.where(x.norm(dim=1) < 1.0, torch.full_like(logl, value), logl)

        def log_prior(samples):  # noqa: F811
            x = samples.x.to(torch.float64)
            return torch.where((x >= -10.0) & (x <= 10.0), torch.full_like(x, math.log(1.0 / 20.0)), torch.full_like(x, -math.inf)).sum(-1)

    params = [f"x_{i}" for i in range(d)]
    asp = Aspire(log_likelihood=log_like, log_prior=log_prior, dims=d, parameters=params, prior_bounds={p: [-10, 10] for p in params},
                 bounded_to_unbounded=False, flow_backend="gaussian", engine=eng, seed=seed + 1, xp=xp)
    asp.fit(Samples(np.random.default_rng(seed).normal(2.0, 1.0, size=(500, d)), parameters=params, xp=np))
    out, history = asp.sample_posterior(n_samples=n, sampler="blackjax_smc", return_history=True, engine=eng, sampler_kwargs=kw,
                                        rng=np.random.default_rng(seed + 2))
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else v  # noqa: E731
    check_hole_run(asp, SimpleNamespace(x=host(out.x), log_likelihood=host(out.log_likelihood), log_prior=host(out.log_prior),
                                        log_evidence=out.log_evidence, log_evidence_error=out.log_evidence_error), history, n)


def test_same_rng_key_same_bits(eng):
    kw = {"step_size": 0.3, "num_integration_steps": 5, "n_steps": 4}
    outs = [_run(eng, 8, 20_000, 9, kw)[1] for _ in range(2)]
    assert np.array_equal(np.asarray(outs[0].x), np.asarray(outs[1].x))
    assert float(outs[0].log_evidence) == float(outs[1].log_evidence)
