"""The NUTS mutation of the "blackjax_smc" sampler on the CPU test double: the facade, the reference's integration scenario on the
split path, option errors and defaults, the restatement's own invariants, stationarity, and a two-rank gloo run.

Specification: reference src/aspire/samplers/smc/blackjax.py:119, 229-277 (blackjax and jax are absent: DESIGN.md §3.18 is this
repository's reading, tests/nuts_ref.py its restatement).  The device kernels are checked against the restatement in
tests/test_gpu_nuts.py.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

import hmc_ref as H
import nuts_ref as N
from nuts_ref import NutsOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampler(d, eng=None, seed=4, lik=None, xp=np, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    eng = eng or NutsOracleEngine()
    lik = lik or DiagGaussianMixture.isotropic(d, normalized=False)
    return HipBlackJAXSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=xp,
                          engine=eng, rng=np.random.default_rng(seed), **kw)


def test_sample_posterior_with_nuts_returns_samples_with_evidence(monkeypatch):
    """Before the NUTS kernels, `algorithm="nuts"` raised NotImplementedError."""
    from aspire_amd import Aspire, Samples
    from aspire_amd import samples as samples_mod
    from aspire_amd.targets import DiagGaussianMixture

    monkeypatch.setattr(samples_mod, "_default_engine", NutsOracleEngine())  # (no GPU in this suite)
    d = 2
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend="gaussian")
    aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, d))))
    out = aspire.sample_posterior(n_samples=200, sampler="blackjax_smc", sampler_kwargs={"algorithm": "nuts", "step_size": 0.3, "n_steps": 3},
                                  engine=NutsOracleEngine(), rng=np.random.default_rng(1))
    assert len(out.x) == 200 and np.isfinite(float(out.log_evidence)) and np.isfinite(float(out.log_evidence_error))
    sp = aspire.sampler
    assert "nuts fused" in sp.last_mutation_path
    assert all(0.0 < a <= 1.0 for a in sp.history.mcmc_acceptance)
    assert 1.0 <= sp.last_nuts["mean_depth"] <= 10.0 and sp.last_nuts["steps_per_transition"] >= 1.0
    assert sp.last_nuts["divergent_share"] == 0.0


@pytest.fixture
def h5(monkeypatch):
    from fake_h5 import FakeFile

    from aspire_amd import io
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    monkeypatch.setattr(samples_mod, "_default_engine", NutsOracleEngine())
    return io


@pytest.mark.parametrize("xp_name", ["numpy", "torch"])
@pytest.mark.parametrize("bounded_to_unbounded", [True, False])
def test_reference_integration_scenario_nuts(h5, tmp_path, bounded_to_unbounded, xp_name):
    """tests/test_blackjax_smc.py's `_scenario` (reference tests/integration_tests/test_integration.py:11-48) with algorithm = "nuts":
    torch callables and a trained flow, so the split path; the numpy callables are refused with HMC's TypeError."""
    from test_reference_integration import _fixtures

    from aspire_amd import Aspire, Samples

    dims, parameters, prior_bounds, xp, log_likelihood, log_prior, init = _fixtures(xp_name)
    samples = Samples(init if xp is np else torch.as_tensor(init), xp=xp)
    aspire = Aspire(log_likelihood=log_likelihood, log_prior=log_prior, dims=dims, parameters=parameters, prior_bounds=prior_bounds,
                    flow_matching=False, bounded_to_unbounded=bounded_to_unbounded, flow_backend="zuko")
    aspire.fit(samples, n_epochs=5)
    kw = {"algorithm": "nuts", "step_size": 0.3, "n_steps": 3, "max_num_doublings": 5}

    def run():
        return aspire.sample_posterior(n_samples=100, sampler="blackjax_smc", adaptive=True, sampler_kwargs=kw, engine=NutsOracleEngine(),
                                       rng=np.random.default_rng(3))

    if xp_name == "numpy":
        with pytest.raises(TypeError, match="torch-differentiable"):
            run()
        return
    out = run()
    assert len(out.x) == 100 and out.parameters == parameters and np.isfinite(float(out.log_evidence))
    x = np.asarray(out.x.cpu())
    assert np.all(np.abs(x) <= 10.0) and abs(x.mean() - 2.0) < 0.6
    with h5.open_h5(tmp_path / "test_integration_blackjax_smc_nuts.h5", "w") as h5_file:
        aspire.save_config(h5_file)
        samples.save(h5_file, path="posterior_samples")
    sp = aspire.sampler
    assert "nuts split" in sp.last_mutation_path
    assert all(0.0 < a <= 1.0 for a in sp.history.mcmc_acceptance) and sp.last_nuts["mean_depth"] <= 5.0


def test_option_errors_and_defaults():
    from hmc_ref import HmcOracleEngine

    d = 2
    run = lambda kw, **skw: _sampler(d, **skw).sample(64, sampler_kwargs=dict({"algorithm": "nuts", "step_size": 0.3, "n_steps": 1}, **kw),  # noqa: E731
                                                     store_sample_history=False, max_n_steps=1)
    for bad in (0, 11, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_num_doublings"):
            run({"max_num_doublings": bad})
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="divergence_threshold"):
            run({"divergence_threshold": bad})
    with pytest.raises(ValueError, match="step_size"):
        run({"step_size": 0.0})
    with pytest.raises(TypeError, match="max_doublings"):
        run({"max_doublings": 3})  # (not blackjax's name)
    with pytest.raises(NotImplementedError, match="dense inverse_mass_matrix"):
        run({"inverse_mass_matrix": np.eye(d)})
    with pytest.raises(NotImplementedError, match='"hmc" or "rwmh"'):
        run({}, eng=HmcOracleEngine())  # an engine without the NUTS entry points
    with pytest.raises(TypeError, match='"nuts" takes gradients'):
        run({}, lik=lambda s: -0.5 * np.sum(np.asarray(s.x) ** 2, axis=-1))
    sp = _sampler(d)
    sp.sample(64, sampler_kwargs={"algorithm": "NUTS", "step_size": 0.4, "n_steps": 2}, store_sample_history=False, max_n_steps=1)
    kw = sp.sampler_kwargs
    assert (kw["max_num_doublings"], kw["divergence_threshold"], kw["inverse_mass_matrix"]) == (10, 1000.0, None)
    assert "nuts fused" in sp.last_mutation_path and sp.key == 42
    # the default algorithm stays "hmc", and HMC takes the two new keys without using them
    sp = _sampler(d)
    sp.sample(64, sampler_kwargs={"n_steps": 1, "max_num_doublings": 3}, store_sample_history=False, max_n_steps=1)
    assert sp.sampler_kwargs["algorithm"] == "hmc" and "hmc fused" in sp.last_mutation_path and sp.last_nuts is None


def test_likelihood_evaluations_and_history():
    n = 128
    sp = _sampler(2)
    post = sp.sample(n, sampler_kwargs={"algorithm": "nuts", "step_size": 0.3, "n_steps": 3}, max_n_steps=1, n_final_samples=150,
                     store_sample_history=False)
    h = sp.history
    assert len(post.x) == 150 and len(h.mcmc_acceptance) == len(h.beta) + 1 and h.mcmc_step_size == []
    # the initial population, then per mutation one evaluation per particle and launch plus the leapfrog steps taken
    steps = sp.n_likelihood_evaluations - n - n * len(h.mcmc_acceptance)
    assert steps > 0 and sp.last_nuts["steps_per_transition"] * n * 3 <= steps


def _case(n=257, d=7, C=3, seed=11):
    return N.mix_case(n, d, C, seed)


def test_restatement_float_types_agree_and_leaf_counts():
    """fp64 and long-double runs of the restatement give every row the same diagnostics; a transition that ended at a whole-tree
    test or at the depth limit took 2^depth - 1 steps."""
    for n, d, C, eps in ((257, 7, 3, 0.3), (257, 33, 1, 0.2), (129, 128, 2, 0.1), (257, 1, 2, 0.05), (129, 7, 3, 2.5)):
        mixes, x, minv = _case(n, d, C, n + d)
        r64, rld, tol_x, keep, gap = N.nuts_tolerance(mixes, 0.6, x, eps, None, 12345, 7, 0)
        assert np.array_equal(r64["info"], rld["info"]) and keep.all() and r64["margin"].min() > 1e-7
        assert gap < 1e-12
        info = r64["info"]
        depth, steps, flags = info[:, 0], info[:, 1], info[:, 2]
        whole = steps == (1 << depth) - 1  # nothing beyond the last complete sub-tree
        assert whole.any() and np.all(steps >= (1 << depth) - 1) and np.all(steps <= (1 << (depth + 1)) - 1)
        assert np.all((flags[~whole] != 0)) and np.all((flags[whole] & N.DIVERGENT) == 0)
        assert np.all((flags[whole] & N.TURNING) != 0)  # (no tree reaches ten doublings at these step sizes)
    assert (r64["info"][:, 2] & N.DIVERGENT).sum() > 0  # the last case diverges


def test_restatement_depth_limit_hole_and_streams():
    mixes, x, minv = _case()
    n, d = x.shape
    ll, lp, lq = (np.zeros(n) for _ in range(3))
    # max_num_doublings = 1: at most one leapfrog step, a moved row sits at position +-1
    xx = x.copy()
    r = N.nuts_mix(xx, ll, lp, lq, 0.6, mixes, minv, 0.3, 5, 0, 0, 1, max_doublings=1)
    assert r["info"][:, 1].max() == 1 and set(np.unique(r["info"][:, 3])) <= {-1, 0, 1} and np.all(r["info"][:, 0] == 1)
    assert np.array_equal(r["info"][:, 3] != 0, np.any(xx != x, axis=1))
    # depth limit 3 with a small step: every tree stops at the limit with 7 steps and no flag
    r = N.nuts_mix(x.copy(), ll, lp, lq, 0.6, mixes, None, 0.01, 5, 0, 0, 1, max_doublings=3)
    assert np.all(r["info"][:, 0] == 3) and np.all(r["info"][:, 1] == 7) and np.all(r["info"][:, 2] == 0)
    assert np.all(np.abs(r["info"][:, 3]) <= 7) and r["stats"][0, 1] == 7 * n
    # a start whose tempered target is -inf: unchanged, zero steps, not moved
    tree = N.Tree(n, d, 10, 0.3, None, 0.6, 1000.0)
    l0, p0, q0, g0 = H.target(mixes, 0.6, x)
    l0 = l0.copy()
    l0[::5] = -np.inf
    l0[1::5] = np.nan
    tree.set_point(x, g0, l0, p0, q0)
    N.run_transition(tree, lambda z: H.target(mixes, 0.6, z), 5, 0, 0)
    hole = np.zeros(n, dtype=bool)
    hole[::5] = hole[1::5] = True
    assert np.all(tree.info()[hole] == 0) and np.array_equal(tree.zp[hole], x[hole]) and np.all(tree.info()[~hole, 1] > 0)
    # the tree's uniforms are a stream of their own, keyed by the global id
    u = N.nuts_uniform(5, (1 << 32) - 3, 9, 7, 1)
    assert np.array_equal(u[4:], N.nuts_uniform(5, (1 << 32) + 1, 5, 7, 1)) and np.all((u > 0) & (u < 1))
    assert not np.array_equal(u, H.accept_uniforms(5, (1 << 32) - 3, 9, 7))


def test_transitions_chain_and_key_by_global_id():
    """Five transitions in one call equal five calls of one; rows 100 .. of a run with gid0 = 0 are a run with gid0 = 100."""
    mixes, x, minv = _case()
    n = len(x)
    a = [x.copy()] + [np.zeros(n) for _ in range(3)]
    b = [x.copy()] + [np.zeros(n) for _ in range(3)]
    ra = N.nuts_mix(*a, 0.5, mixes, minv, 0.3, 99, 0, 10, 5)
    for s in range(5):
        rb = N.nuts_mix(*b, 0.5, mixes, minv, 0.3, 99, 0, 10 + s, 1)
        assert np.array_equal(rb["stats"][0], ra["stats"][s])
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    c = [x[100:].copy()] + [np.zeros(n - 100) for _ in range(3)]
    N.nuts_mix(*c, 0.5, mixes, minv, 0.3, 99, 100, 10, 5)
    assert np.array_equal(c[0], a[0][100:])


def test_restatement_leaves_out_no_row_of_the_device_cases():
    """The cap tests/test_gpu_nuts.py allows itself - at most 1 % of a case's rows within 1e-9 of a decision threshold, or with
    diagnostics that differ between the fp64 and the long-double run - is not needed by the restatement itself."""
    for case in N.fused_cases():
        _, x, _, (r64, rld, tol_x, keep, gap) = N.fused_case_reference(*case)
        assert keep.all(), case
        assert 2 <= np.median(r64["info"][:, 0]) <= 5, (case, np.bincount(r64["info"][:, 0]))
        assert tol_x.max() < 1e-11
    mixes, x, beta, eps, _, seed = H.split_fused_case()
    assert N.nuts_tolerance(mixes, beta, x, eps, None, seed, 0, 0)[3].all()
    # the divergent edge case of the device tests shows both endings
    mixes, x, beta, eps, thr = N.divergent_case()
    r64, _, _, keep, _ = N.nuts_tolerance(mixes, beta, x, eps, None, *N.CASE_KEY, threshold=thr)
    flags = r64["info"][:, 2]
    assert keep.all() and (flags & N.DIVERGENT).sum() >= 50 and (flags & N.TURNING).sum() >= 50 and (r64["info"][:, 3] != 0).sum() >= 50


def test_stationarity_on_a_gaussian():
    """3000 exact draws of N(0, diag(0.3, 1, 2.5)), 8 transitions: every particle is still distributed as the target, so the bounds
    are the exact 5-sigma bounds of a sample of n (tests/test_gpu_blackjax_smc.py test_stationarity_on_a_gaussian)."""
    n, v = 3000, np.array([0.3, 1.0, 2.5])
    d = len(v)
    x0 = np.random.default_rng(9).normal(size=(n, d)) * np.sqrt(v)
    x = x0.copy()
    target = (np.array([0.0]), np.zeros((1, d)), (1.0 / v)[None])
    flat = (np.array([0.0]), np.zeros((1, d)), np.full((1, d), 1e-30))
    r = N.nuts_mix(x, *(np.zeros(n) for _ in range(3)), 1.0, [target, flat, flat], None, 0.45, 31337, 0, 0, 8)
    acc = r["stats"][:, 3].sum() / (N.TWO32 * n * 8)
    mean, var = x.mean(axis=0), x.var(axis=0, ddof=1)
    print(f"stationarity: acceptance {acc:.3f}, max |mean| / sigma {np.max(np.abs(mean) / np.sqrt(v / n)):.2f}, "
          f"max |var - v| / sigma {np.max(np.abs(var - v) / (v * math.sqrt(2.0 / (n - 1)))):.2f}")
    assert 0.8 < acc < 0.999 and r["stats"][:, 2].sum() == 0 and np.all(np.any(x != x0, axis=1))
    assert np.all(np.abs(mean) <= 5.0 * np.sqrt(v / n))
    assert np.all(np.abs(var - v) <= 5.0 * v * math.sqrt(2.0 / (n - 1)))


def test_split_path_equals_fused_path_on_the_restatement():
    from aspire_amd.targets import DiagGaussianMixture

    d = 7
    g = np.random.default_rng(70)
    mix = DiagGaussianMixture(g.normal(size=(3, d)), g.uniform(0.5, 2.0, size=(3, d)), weights=[0.2, 0.3, 0.5])
    kw = {"algorithm": "nuts", "step_size": 0.2, "n_steps": 2, "inverse_mass_matrix": np.linspace(0.7, 1.4, d)}
    a = _sampler(d, lik=mix)
    pa = a.sample(512, sampler_kwargs=kw, store_sample_history=False)
    b = _sampler(d, lik=lambda s: mix(s.x), xp=torch)
    pb = b.sample(512, sampler_kwargs=kw, store_sample_history=False)
    assert "nuts fused" in a.last_mutation_path and "nuts split" in b.last_mutation_path
    assert a.history.mcmc_acceptance == b.history.mcmc_acceptance and a.last_nuts == b.last_nuts
    np.testing.assert_allclose(np.asarray(pa.x), np.asarray(pb.x.cpu() if torch.is_tensor(pb.x) else pb.x), rtol=1e-9, atol=1e-9)


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nuts_ref import NutsOracleEngine as Eng

    from aspire_amd.comm import TorchDistComm
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    d = 4
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    eng = Eng()
    sp = HipBlackJAXSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=np,
                        engine=eng, comm=TorchDistComm(torch.device("cpu")), rng=np.random.default_rng(4))
    sp.shard_layout = "slots"  # reproduces the single-rank particle order
    post = sp.sample(1024, sampler_kwargs=GLOO_KW, store_sample_history=False)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), x=np.asarray(post.x), acc=np.array(sp.history.mcmc_acceptance),
             beta=np.array(sp.history.beta), logz=float(post.log_evidence), depth=sp.last_nuts["mean_depth"])
    dist.barrier()
    dist.destroy_process_group()


GLOO_KW = {"algorithm": "nuts", "step_size": 0.3, "n_steps": 2}


def test_two_rank_gloo_run_gives_the_single_rank_particles(tmp_path):
    """The tree's streams are keyed by the global particle id: two ranks (slot layout) draw what one rank draws.  The acceptance
    figure comes from integer sums, so it is equal wherever the betas are; the betas agree to the rounding of the sharded weight
    reductions (tests/test_blackjax_smc.py's two-rank test)."""
    from test_dist_gloo import spawn_ranks

    spawn_ranks(_gloo_worker, 2, lambda port: (2, port, str(tmp_path)))
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    sp = _sampler(4)
    post = sp.sample(1024, sampler_kwargs=GLOO_KW, store_sample_history=False)
    assert np.array_equal(r0["beta"], r1["beta"]) and np.array_equal(r0["acc"], r1["acc"]) and float(r0["depth"]) == float(r1["depth"])
    np.testing.assert_allclose(r0["beta"], sp.history.beta, rtol=1e-9)
    assert float(r0["logz"]) == pytest.approx(float(post.log_evidence), abs=5e-9)
    np.testing.assert_allclose(r0["acc"], sp.history.mcmc_acceptance, atol=1e-12)
    assert r0["acc"][0] == sp.history.mcmc_acceptance[0]  # (the first mutation runs at the same beta to the bit: integers)
    xs = np.concatenate([r0["x"], r1["x"]])
    np.testing.assert_allclose(xs, np.asarray(post.x), rtol=1e-9, atol=1e-9)
    assert abs(float(post.log_evidence) - 2.0 * math.log(math.pi)) < 0.3
