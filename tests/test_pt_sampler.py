"""The "pt_minipcn" sampler on the CPU test double (tests/pt_ref.py): each rung alone is the pCN chain of its rows, the exchange keeps
rows and densities together, the facade and its errors, both dispatch paths, and the statistical check of DESIGN.md section 3.21.
The exchange and reduction kernels are checked in tests/test_gpu_pt.py.
"""
import numpy as np
import pytest
import torch

import pt_ref
from chain_ref import ChainOracleEngine
from pt_ref import GAUSS_D as D
from pt_ref import PTOracleEngine, gaussian_closed_form, gaussian_targets, pt_z_scores


def make(seed=0, callables=False, eng=None, d=D, targets=None, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    eng = eng or PTOracleEngine()
    lik, pri = targets or gaussian_targets()
    if callables:
        l0, p0 = lik, pri
        lik, pri = (lambda s: l0(s)), (lambda s: p0(s))
    return HipPTMiniPCN(log_likelihood=lik, log_prior=pri, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, engine=eng, seed=100 + seed), xp=np,
                        engine=eng, rng=np.random.default_rng(seed), **kw)


class SpyEngine(PTOracleEngine):
    """Keeps what every rung's first `pcn_mutate` call was given."""

    def __init__(self):
        super().__init__()
        self.first, self.swaps = {}, []

    def pcn_mutate(self, x, ll, lp, lq, beta, mu, L, Linv, t_ll, t_lp, t_lq, seed, gid0, rho, n_steps, *a, **k):
        if gid0 not in self.first:
            self.first[gid0] = dict(x=x.clone(), ll=ll.clone(), lp=lp.clone(), lq=lq.clone(), beta=beta, mu=mu.clone(), L=L.clone(),
                                    Linv=Linv.clone(), mixes=(t_ll, t_lp, t_lq), seed=seed, rho=rho, rest=(a, k))
        return super().pcn_mutate(x, ll, lp, lq, beta, mu, L, Linv, t_ll, t_lp, t_lq, seed, gid0, rho, n_steps, *a, **k)

    def pt_swap(self, *a, **k):
        self.swaps.append(a[5])
        return super().pt_swap(*a, **k)


def test_without_exchange_every_rung_is_its_own_pcn_chain():
    """swap_every = 0: rung r's recorded rows and densities are, bit for bit, what `pcn_mutate` alone returns for that rung's rows at
    beta_r with gid0 = r W and the run's seed - the log q mixture being the prior's, log q the prior's value."""
    W, steps = 12, 7
    eng = SpyEngine()
    s = make(eng=eng)
    out = s.sample(n_walkers=W, n_temps=4, n_steps=steps, swap_every=0)
    assert out.chain_shape == (4, steps, W) and eng.swaps == [] and np.all(s.swap_acceptance == 0)
    betas = np.asarray(out.betas)
    assert sorted(eng.first) == [0, W, 2 * W, 3 * W] and len({f["seed"] for f in eng.first.values()}) == 1
    plain = ChainOracleEngine()  # (no chain target: the step loop alone)
    ll4, lp4 = np.asarray(out.log_likelihood).reshape(4, steps, W), np.asarray(out.log_prior).reshape(4, steps, W)
    for r in range(4):
        f = eng.first[r * W]
        assert f["beta"] == betas[r] and f["mixes"][2] is f["mixes"][1] and torch.equal(f["lq"], f["lp"])
        a, k = f["rest"]
        for n in (3, steps):
            x, ll, lp, lq = f["x"].clone(), f["ll"].clone(), f["lp"].clone(), f["lq"].clone()
            plain.pcn_mutate(x, ll, lp, lq, f["beta"], f["mu"], f["L"], f["Linv"], *f["mixes"], f["seed"], r * W, f["rho"], n, *a, **k)
            assert x.numpy().tobytes() == np.ascontiguousarray(out.chain[r, n - 1]).tobytes()
            assert ll.numpy().tobytes() == ll4[r, n - 1].tobytes() and lp.numpy().tobytes() == lp4[r, n - 1].tobytes()
    assert not np.array_equal(out.chain[0], out.chain[1])


@pytest.mark.parametrize("callables", [False, True], ids=["mixtures", "callables"])
@pytest.mark.parametrize("swap_every", [1, 3])
def test_with_exchange_rows_and_densities_stay_together(callables, swap_every):
    eng = SpyEngine()
    s = make(eng=eng, callables=callables, seed=2)
    out = s.sample(n_walkers=10, n_temps=5, n_steps=9, swap_every=swap_every)
    lik, pri = gaussian_targets()
    np.testing.assert_allclose(out.log_likelihood, lik(out.x), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out.log_prior, pri(out.x), rtol=1e-12, atol=1e-12)
    assert eng.swaps == list(range(9 // swap_every))  # round k after step (k + 1) swap_every
    assert s.swap_acceptance.shape == (4,) and np.all(s.swap_acceptance >= 0) and s.swap_acceptance.sum() > 0
    assert ("asmc_pcn_split" if callables else "asmc_pcn_mutate") in s.last_mutation_path and "asmc_pt_swap" in s.last_mutation_path
    # the record of step t precedes the exchange behind it: the last slot is the state the last exchange was given
    quiet = make(eng=PTOracleEngine(), callables=callables, seed=2).sample(n_walkers=10, n_temps=5, n_steps=swap_every, swap_every=swap_every)
    assert np.array_equal(quiet.chain[:, :swap_every], out.chain[:, :swap_every])


def test_the_two_dispatch_paths_are_one_chain():
    a = make(seed=5).sample(n_walkers=8, n_temps=3, n_steps=6)
    b = make(seed=5, callables=True).sample(n_walkers=8, n_temps=3, n_steps=6)
    np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)


def test_default_ladder_and_given_betas():
    from aspire_amd.samplers.mcmc import default_ladder

    lad = default_ladder(8, 1e-3)
    assert lad.shape == (8,) and lad[0] == 1.0 and lad[-1] == 0.0 and lad[-2] == pytest.approx(1e-3) and np.all(np.diff(lad) < 0)
    np.testing.assert_allclose(lad[1:-1] / lad[:-2], 1e-3 ** (1 / 6))
    assert list(default_ladder(1, 1e-3)) == [1.0] and list(default_ladder(2, 1e-3)) == [1.0, 0.0] and list(default_ladder(3, 0.1)) == [1.0, 0.1, 0.0]
    s = make()
    out = s.sample(n_samples=6, n_steps=3, betas=[1.0, 0.5, 0.25])
    assert out.chain_shape == (3, 3, 6) and list(out.betas) == [1.0, 0.5, 0.25]
    assert s.evidence["stepping_stone"] is None and len(s.evidence["thermodynamic_integration"]) == 2
    for bad in ([0.9, 0.5], [1.0, 0.5, 0.5], [1.0, -0.1], [[1.0, 0.0]]):
        with pytest.raises(ValueError, match="betas must be"):
            make().sample(n_samples=6, n_steps=3, betas=bad)


def test_kwargs_contract_and_result():
    from aspire_amd import PTMCMCSamples

    s = make()
    out = s.sample(n_samples=6, n_temps=3, n_steps=10, burnin=2, thin=3)
    assert isinstance(out, PTMCMCSamples) and isinstance(out.x, np.ndarray) and out.chain_shape == (3, 3, 6)
    assert out.thin == 3 and out.burn_in == 2 and out.n_temps == 3
    assert s.rung_acceptance.shape == (3,) and s.rung_step_size.shape == (3,) and s.swap_acceptance.shape == (2,)
    assert np.all((s.rung_acceptance > 0) & (s.rung_acceptance <= 1)) and np.all((s.rung_step_size >= 1e-4) & (s.rung_step_size <= 0.99))
    full = make().sample(n_samples=6, n_temps=3, n_steps=10)
    assert np.array_equal(out.chain, full.chain[:, 2::3])
    # the evidence attribute: the container's estimators on the FULL chain with the default burn-in fraction
    assert s.evidence == {"thermodynamic_integration": full.log_evidence_thermodynamic_integration(),
                          "stepping_stone": full.log_evidence_stepping_stone()}
    for kw, exc, msg in ((dict(step_fn="rwm"), NotImplementedError, "step_fn"), (dict(n_steps=0), ValueError, "n_steps"),
                         (dict(swap_every=-1), ValueError, "swap_every"), (dict(n_temps=65), ValueError, "at most 64"),
                         (dict(n_temps=0), ValueError, "n_temps"), (dict(beta_min=1.5), ValueError, "beta_min")):
        with pytest.raises(exc, match=msg):
            make().sample(n_samples=6, **kw)
    with pytest.raises(ValueError, match="n_walkers or n_samples"):
        make().sample()
    with pytest.raises(TypeError):
        make().sample(n_samples=6, last_step_only=True)


def test_one_rung_runs_without_exchange_and_refit_stops_at_burnin():
    eng = SpyEngine()
    s = make(eng=eng)
    out = s.sample(n_samples=6, n_temps=1, n_steps=5)
    assert out.chain_shape == (1, 5, 6) and eng.swaps == [] and s.swap_acceptance.shape == (0,) and s.evidence["stepping_stone"] is None
    fits = []
    s = make()
    inner = s._fit_reference
    s._fit_reference = lambda *a, **k: (fits.append(1), inner(*a, **k))[1]
    s.sample(n_samples=8, n_temps=2, n_steps=12, burnin=7, refit_every=3, swap_every=2)
    assert len(fits) == 2 * (1 + 2)  # at the start, and before steps 3 and 6 (t < burnin)


def test_memory_guard_one_rank_and_registration(monkeypatch):
    from aspire_amd import Aspire, PTMCMCSamples, Samples
    from aspire_amd import samples as samples_mod
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    eng = PTOracleEngine()
    eng.free_bytes = 1000
    need = 3 * 5 * 6 * (D * 8 + 16)
    with pytest.raises(ValueError, match=rf"{need} bytes.*1000 bytes are free"):
        make(eng=eng).sample(n_samples=6, n_temps=3, n_steps=5)
    assert eng.chain_allocs == 0

    class TwoRanks:
        sharded, world, rank = True, 2, 0

    with pytest.raises(NotImplementedError, match="one rank"):
        make(comm=TwoRanks()).sample(n_samples=6)
    monkeypatch.setattr(samples_mod, "_default_engine", PTOracleEngine())
    lik, pri = gaussian_targets()
    aspire = Aspire(log_likelihood=lik, log_prior=pri, dims=D, flow_backend="gaussian")
    aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, D))))
    assert aspire.get_sampler_class("pt_minipcn") is HipPTMiniPCN
    out = aspire.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=PTOracleEngine(), rng=np.random.default_rng(1), n_walkers=6,
                                  n_temps=3, n_steps=4)
    assert isinstance(out, PTMCMCSamples) and out.chain_shape == (3, 4, 6)


def test_preconditioned_chain_and_wrappers(monkeypatch):
    from aspire_amd import Aspire, Samples
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(samples_mod, "_default_engine", PTOracleEngine())
    lik, pri = gaussian_targets()
    names = [f"x_{i}" for i in range(D)]
    bounds = {n: [-12, 12] for n in names}
    aspire = Aspire(log_likelihood=lambda s: lik(s), log_prior=lambda s: pri(s), dims=D, parameters=names, prior_bounds=bounds,
                    flow_backend="gaussian")
    aspire.fit(Samples(np.random.default_rng(0).normal(size=(400, D))))
    out = aspire.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=PTOracleEngine(), rng=np.random.default_rng(2), n_walkers=8,
                                  n_temps=3, n_steps=6, preconditioning_kwargs={"bounded_to_unbounded": True})
    s = aspire.sampler
    assert "preconditioned" in s.last_mutation_path and np.all(np.abs(out.x) < 12)
    np.testing.assert_allclose(out.log_likelihood, lik(out.x), rtol=1e-9, atol=1e-9)
    z = np.asarray(s.preconditioning_transform.forward(out.x[:5])[0])
    x, logj = s.preconditioning_transform.inverse(z)
    np.testing.assert_allclose(s.log_likelihood_wrapper(z), lik(np.asarray(x)), rtol=1e-9)
    np.testing.assert_allclose(s.log_prior_wrapper(z), pri(np.asarray(x)) + np.asarray(logj), rtol=1e-9)


def test_rung_means_and_evidence_against_the_closed_form():
    """d = 4, prior N(0, 4 I), likelihood N(x; m, 0.25 I), 6 rungs ending at 0, 64 walkers, 400 steps, half discarded, swap_every = 1
    (the adaptation's gain stays 1: its worst case).  Every rung's mean log-likelihood, the stepping-stone log Z and the TI log Z
    (against the trapezoid of the closed-form means on the same ladder) within 5 standard errors from the between-walker spread of
    the run itself (tests/pt_ref.py pt_z_scores).  Over 8 seeds (rng seeds 0 .. 7, flow seeds 100 .. 107) on this restatement,
    before the bound was fixed: the largest |z| of the 64 statistics was 2.31."""
    s = make(seed=3)
    out = s.sample(n_walkers=64, n_temps=6, n_steps=400, burnin=200, swap_every=1)
    betas = np.asarray(out.betas)
    assert betas[-1] == 0.0 and out.chain_shape == (6, 200, 64)
    mean_ll, logz = gaussian_closed_form(pt_ref.GAUSS_M, pt_ref.GAUSS_SP2, pt_ref.GAUSS_SL2, betas)
    z_mean, z_ti, z_ss = pt_z_scores(np.asarray(out.log_likelihood).reshape(out.chain_shape), betas, mean_ll, logz)
    print("z(rung means)", np.round(z_mean, 2), "z(TI)", round(z_ti, 2), "z(SS)", round(z_ss, 2), "acceptance", np.round(s.rung_acceptance, 2),
          "swaps", np.round(s.swap_acceptance, 2), s.evidence, "log Z", logz)
    assert np.all(np.abs(z_mean) < 5.0) and abs(z_ti) < 5.0 and abs(z_ss) < 5.0
    assert np.all(s.swap_acceptance > 0.05) and 0.1 < s.rung_acceptance[0] < 0.8
    assert abs(out.log_evidence_stepping_stone()[0] - logz) < 0.5  # (the estimator on the kept half, loosely: the z-score is the check)
