"""Chain diagnostics without a GPU: the direct-summation restatement of tests/autocorr_ref.py against the FFT
estimator `integrated_time` and the closed form, the razor guard over every fixture of this file and of
tests/test_gpu_chain_diagnostics.py, and the containers and samplers on numpy arrays and on the CPU test double.
"""
import logging

import numpy as np
import pytest
import torch

import autocorr_ref as R
from autocorr_ref import DiagMixin, DiagOracleEngine
from pt_ref import PTOracleEngine, gaussian_targets

PHI3 = (0.0, 0.5, 0.9)
D = 4


class PTDiagEngine(DiagMixin, PTOracleEngine):
    pass


def fft_curves(x, c=5.0):
    """The intermediate arrays of `integrated_time` (aspire_amd/samplers/emcee_smc.py): (rho [S, d], windows [d])."""
    n_t = x.shape[0]
    n = 1 << (n_t - 1).bit_length()
    f = np.fft.fft(x - x.mean(axis=0), n=2 * n, axis=0)
    acf = np.fft.ifft(f * np.conjugate(f), axis=0)[:n_t].real
    rho = (acf / acf[0]).mean(axis=1)
    m = np.arange(n_t)[:, None] < c * (2.0 * np.cumsum(rho, axis=0) - 1.0)
    return rho, np.where(m.any(axis=0), np.argmin(m, axis=0), n_t - 1)


@pytest.mark.parametrize("seed", [11, 12])
def test_direct_summation_is_the_fft_estimator(seed):
    """S = 400, W = 64, phi = 0, 0.5, 0.9: rho within 1e-10 at every lag, equal windows, tau within 1e-9."""
    from aspire_amd.samplers.emcee_smc import integrated_time

    x = R.ar1(seed, 400, 64, PHI3)
    r = R.autocorr_direct(x, all_lags=True)
    rho_fft, win_fft = fft_curves(x)
    assert np.max(np.abs(r["rho"] - rho_fft)) < 1e-10
    assert np.all(r["mass"] <= 1.0 + 1e-12) and np.all(r["mass"][0] > 1.0 - 1e-12)  # Cauchy-Schwarz; lag 0 is c0 / c0
    assert np.array_equal(r["window"], win_fft)
    tau = integrated_time(x, quiet=True)
    assert np.max(np.abs(r["tau"] - tau)) < 1e-9
    assert np.array_equal(R.autocorr_direct(x)["window"], r["window"])  # stopping at the last window changes nothing
    assert np.array_equal(R.autocorr_direct(x)["tau"], r["tau"])


def test_direct_summation_against_the_closed_form():
    """tau of AR(1) is (1 + phi) / (1 - phi); the band is the 10 % of tests/test_emcee_smc.py::test_integrated_time_of_ar1_chains,
    at that test's chain (4000 steps, 32 walkers), where it is a statistical band.  At 400 steps x 64 walkers it is none: emcee's
    estimator itself - the FFT form and this restatement agree to 1e-9 there - is biased low by the centring, tau_hat / tau =
    1.04, 0.90, 0.77 (seed 11) and 0.97, 0.95, 0.73 (seed 12) for phi = 0, 0.5, 0.9."""
    phi = np.array(PHI3)
    x = R.ar1(7, 4000, 32, phi)
    tau = R.autocorr_direct(x)["tau"]
    assert np.all(np.abs(tau / ((1 + phi) / (1 - phi)) - 1) < 0.1), tau


def test_the_window_is_always_found_by_the_last_lag():
    """sum over all lags of the zero-padded autocorrelation of a centred series is 0, so tau_{S-1} = 0 up to rounding and lag S - 1
    passes k >= c tau_k whenever S >= 2: 'no window' happens for NaN alone.  phi = 0.99 at S = 50 - far too short a chain - finds
    its window before the last lag."""
    r = R.autocorr_direct(R.ar1(13, 50, 7, [0.99]), all_lags=True)
    assert abs(r["taus"][-1, 0]) < 1e-12 and 0 < r["window"][0] < 49
    x = R.ar1(14, 50, 7, [0.5, 0.5])
    x[:, :, 1] = 3.0  # never moves: c0 = 0, rho = NaN
    r = R.autocorr_direct(x)
    assert np.isnan(r["tau"][1]) and r["window"][1] == 49 and np.isfinite(r["tau"][0])
    assert np.isnan(R.autocorr_direct(np.zeros((1, 3, 2)))["tau"]).all()


def all_fixtures():
    for seed in (11, 12):
        yield f"fft-{seed}", R.ar1(seed, 400, 64, PHI3)
    yield "closed-form", R.ar1(7, 4000, 32, PHI3)
    yield "phi-0.99", R.ar1(13, 50, 7, [0.99])
    for S, W, d in R.GPU_SHAPES:
        for dt in (np.float64, np.float32):
            yield f"gpu-{S}-{W}-{d}-{np.dtype(dt).name}", R.fixture(S, W, d, dt)
    for name, x in R.special_fixtures().items():
        yield name, x


def test_razor_guard():
    """No window decision of any fixture is within 1e-6 of flipping, so no comparison of windows needs an excuse."""
    worst = {}
    for name, x in all_fixtures():
        for rung in (x if x.ndim == 4 else [x]):
            worst[name] = min(worst.get(name, np.inf), R.razor_margin(rung))
    bad = {k: v for k, v in worst.items() if not v > 1e-6}
    assert not bad, bad


# ---- containers ---------------------------------------------------------------------------------------------------------------
def iid_chain(seed=0, S=200, W=16, d=3):
    return np.random.default_rng(seed).normal(size=(S, W, d))


def test_mcmc_samples_on_numpy_arrays(caplog):
    from aspire_amd import MCMCSamples

    x = R.ar1(21, 300, 16, PHI3)
    s = MCMCSamples.from_chain(x)
    assert s.autocorrelation_time is None
    with caplog.at_level(logging.WARNING):
        tau = s.integrated_autocorr_time()
    assert "shorter than 50 times" in caplog.text  # quiet by default: phi = 0.9 needs more than 300 steps
    ref = R.autocorr_direct(x)
    assert tau.shape == (3,) and tau is s.autocorrelation_time and np.max(np.abs(tau - ref["tau"])) < 1e-9
    with pytest.raises(RuntimeError, match="shorter than 50 times"):
        s.integrated_autocorr_time(quiet=False)
    np.testing.assert_allclose(s.effective_sample_size(), 300 * 16 / ref["tau"], rtol=1e-9)
    cut = s.integrated_autocorr_time(discard=100)
    assert np.max(np.abs(cut - R.autocorr_direct(x[100:])["tau"])) < 1e-9
    with pytest.raises(ValueError, match="discard"):
        s.integrated_autocorr_time(discard=300)
    fresh = MCMCSamples.from_chain(x)
    np.testing.assert_allclose(fresh.effective_sample_size(), 300 * 16 / ref["tau"], rtol=1e-9)  # computes tau itself
    assert fresh.autocorrelation_time is not None
    flat = MCMCSamples.from_chain(x[:, 0])  # [S, d]: one walker
    assert np.max(np.abs(flat.integrated_autocorr_time() - R.autocorr_direct(x[:, :1])["tau"])) < 1e-9


def test_split_rhat_on_numpy_arrays():
    from aspire_amd import MCMCSamples
    from aspire_amd.samples import split_rhat_host

    x = iid_chain()
    r = MCMCSamples.from_chain(x).split_rhat()
    assert r.shape == (3,) and np.all(np.abs(r - 1) < 0.02), r
    np.testing.assert_allclose(r, R.split_rhat_direct(x)[0], rtol=1e-12)
    x[:, ::2] += 3.0  # half the walkers three standard deviations away
    assert np.all(MCMCSamples.from_chain(x).split_rhat() > 1.5)
    odd = iid_chain(1, S=9, W=5)
    np.testing.assert_allclose(split_rhat_host(odd), split_rhat_host(np.delete(odd, 4, axis=0)), rtol=0)  # the middle step is dropped
    assert np.isnan(split_rhat_host(iid_chain(2, S=3))).all()


def test_field_survives_post_process_to_numpy_and_hdf5(monkeypatch, tmp_path):
    from fake_h5 import FakeFile

    from aspire_amd import MCMCSamples, io

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    x = torch.from_numpy(R.ar1(22, 120, 8, PHI3))
    s = MCMCSamples.from_chain(x, xp=torch, engine=DiagOracleEngine())
    tau = s.integrated_autocorr_time()
    np.testing.assert_array_equal(tau, R.autocorr_direct(x.numpy())["tau"])  # a tensor goes through the engine
    np.testing.assert_array_equal(s.split_rhat(), R.split_rhat_direct(x.numpy())[0])
    cut = s.post_process(burn_in=10, thin=2)
    assert cut.engine is s.engine and np.array_equal(cut.autocorrelation_time, tau)
    host = cut.to_numpy()
    assert isinstance(host.x, np.ndarray) and np.array_equal(host.autocorrelation_time, tau)
    path = tmp_path / "chain.h5"
    with io.open_h5(path, "w") as fp:
        host.save(fp, path="chain")
    with io.open_h5(path, "r") as fp:
        back = MCMCSamples.load(fp, path="chain")
    assert np.array_equal(np.asarray(back.autocorrelation_time), tau) and tuple(back.chain_shape) == (55, 8)


def test_tempered_container():
    from aspire_amd import PTMCMCSamples

    x = np.stack([R.ar1(30 + r, 150, 12, PHI3) for r in range(3)])  # [T, S, W, d]
    betas = np.array([1.0, 0.3, 0.0])
    want = np.stack([R.autocorr_direct(x[r])["tau"] for r in range(3)])
    for s in (PTMCMCSamples.from_chain(x, betas=betas),
              PTMCMCSamples.from_chain(torch.from_numpy(x), betas=betas, xp=torch, engine=PTDiagEngine())):
        tau = s.integrated_autocorr_time()
        assert tau.shape == (3, 3) and np.max(np.abs(tau - want)) < 1e-9
        assert np.array_equal(np.asarray(s.at_temperature(1).autocorrelation_time), tau[1])
        np.testing.assert_allclose(s.effective_sample_size(), 150 * 12 / want, rtol=1e-9)
        rh = s.split_rhat()
        assert rh.shape == (3, 3)
        np.testing.assert_allclose(rh, np.stack([R.split_rhat_direct(x[r])[0] for r in range(3)]), rtol=1e-12)
        cut = s.integrated_autocorr_time(discard=50)
        assert np.max(np.abs(cut[2] - R.autocorr_direct(x[2, 50:])["tau"])) < 1e-9


# ---- samplers -------------------------------------------------------------------------------------------------------------------
def make(kind, seed=0, eng=None, xp=np):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipEmcee, HipMiniPCN, HipPTMiniPCN
    from aspire_amd.targets import DiagGaussianMixture

    if kind == "pt_minipcn":
        eng, cls, d = eng or PTDiagEngine(), HipPTMiniPCN, gaussian_targets()[0].dims
        lik, pri = gaussian_targets()
    else:
        eng, cls, d = eng or DiagOracleEngine(), (HipEmcee if kind == "emcee" else HipMiniPCN), D
        lik = DiagGaussianMixture.isotropic(d, mean=1.0, var=1.0, normalized=False)
        pri = DiagGaussianMixture.isotropic(d, mean=0.0, var=4.0, normalized=True)
    return cls(log_likelihood=lik, log_prior=pri, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, engine=eng, seed=100 + seed), xp=xp,
               engine=eng, rng=np.random.default_rng(seed))


RUN = {"minipcn": dict(n_walkers=12, n_steps=40), "emcee": dict(nwalkers=12, nsteps=40),
       "pt_minipcn": dict(n_walkers=12, n_temps=3, n_steps=40)}


@pytest.mark.parametrize("kind", ["minipcn", "emcee", "pt_minipcn"])
def test_autocorr_keyword(kind):
    """autocorr=True fills the field from the returned chain and changes nothing else; the default leaves it None."""
    plain = make(kind).sample(**RUN[kind])
    assert plain.autocorrelation_time is None
    s = make(kind)
    out = s.sample(autocorr=True, **RUN[kind])
    assert np.array_equal(out.x, plain.x) and np.array_equal(out.log_likelihood, plain.log_likelihood)
    tau = np.asarray(out.autocorrelation_time)
    if kind == "pt_minipcn":
        want = np.stack([R.autocorr_direct(out.chain[r])["tau"] for r in range(3)])
        assert tau.shape == (3, out.dims) and np.array_equal(s.history.mcmc_autocorr[-1], tau[0])
    else:
        want = R.autocorr_direct(out.chain)["tau"]
        assert tau.shape == (D,)
    np.testing.assert_array_equal(tau, want)
    np.testing.assert_allclose(out.effective_sample_size(), 40 * 12 / want)


def test_autocorr_keyword_after_burn_in():
    out = make("minipcn").sample(autocorr=True, burnin=10, thin=2, **RUN["minipcn"])
    full = make("minipcn").sample(**RUN["minipcn"])
    np.testing.assert_array_equal(out.autocorrelation_time, R.autocorr_direct(full.chain[10:])["tau"])
    assert out.chain_shape == (15, 12)
    with pytest.raises(ValueError, match="last_step_only"):
        make("minipcn").sample(autocorr=True, last_step_only=True, **RUN["minipcn"])


@pytest.mark.parametrize("kind", ["minipcn", "emcee", "pt_minipcn"])
def test_get_autocorr_time(kind):
    s = make(kind)
    with pytest.raises(RuntimeError, match="call sample"):
        s.get_autocorr_time()
    out = s.sample(**RUN[kind])
    with pytest.raises(RuntimeError, match="shorter than 50 times"):  # emcee's default: not quiet, and 40 steps are few
        s.get_autocorr_time()
    chains = out.chain if kind == "pt_minipcn" else out.chain[None]
    ref = lambda sl: np.stack([R.autocorr_direct(ch[sl])["tau"] for ch in chains])  # noqa: E731
    shape = (3, out.dims) if kind == "pt_minipcn" else (out.dims,)
    tau = s.get_autocorr_time(quiet=True)
    assert tau.shape == shape
    np.testing.assert_array_equal(tau.reshape(len(chains), -1), ref(slice(None)))
    assert out.autocorrelation_time is None  # the call does not write into the container it was given back
    np.testing.assert_array_equal(s.get_autocorr_time(discard=8, quiet=True).reshape(len(chains), -1), ref(slice(8, None)))
    # emcee: thin * integrated_time(get_chain(discard, thin)), get_chain keeping the steps discard + thin - 1, discard + 2 thin - 1, ...
    np.testing.assert_array_equal(s.get_autocorr_time(discard=4, thin=3, quiet=True).reshape(len(chains), -1), 3 * ref(slice(6, None, 3)))
    np.testing.assert_array_equal(s.get_autocorr_time(tol=0), tau)  # tol = 0 never raises
    assert not np.array_equal(s.get_autocorr_time(c=2.0, quiet=True), tau)


def test_last_step_only_run_forgets_the_chain():
    s = make("minipcn")
    s.sample(**RUN["minipcn"])
    s.sample(n_walkers=12, n_steps=5, last_step_only=True)
    with pytest.raises(RuntimeError, match="call sample"):
        s.get_autocorr_time()
