"""`rung_launch="batched"` and `adapt_ladder=True` of the "pt_minipcn" sampler on the CPU test double (tests/pt_batch_ref.py; DESIGN.md
section 3.22): the two launch paths are one chain, the errors, the ladder's invariants, and the statistical check of section 3.21 from a
deliberately uneven ladder.  The kernels are checked in tests/test_gpu_pt_batched.py.
"""
import numpy as np
import pytest

import pt_ref
from pt_batch_ref import PTBatchOracleEngine, ladder_update_ref
from pt_ref import GAUSS_D, gaussian_closed_form, gaussian_targets, pt_z_scores


def mixture_targets(d, seed=0):
    """A 3-component likelihood and a broad single-Gaussian prior at dimension d, both normalised."""
    from aspire_amd.targets import DiagGaussianMixture

    g = np.random.default_rng([seed, d])
    return (DiagGaussianMixture(g.normal(size=(3, d)), 0.5, normalized=True), DiagGaussianMixture(np.zeros((1, d)), 4.0, normalized=True))


def make(seed=0, d=GAUSS_D, targets=None, callables=False, eng=None, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    eng = eng or PTBatchOracleEngine()
    lik, pri = targets or (gaussian_targets() if d == GAUSS_D else mixture_targets(d))
    if callables:
        l0, p0 = lik, pri
        lik, pri = (lambda s: l0(s)), (lambda s: p0(s))
    return HipPTMiniPCN(log_likelihood=lik, log_prior=pri, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, engine=eng, seed=100 + seed), xp=np,
                        engine=eng, rng=np.random.default_rng(seed), **kw)


def assert_same_run(a, sa, b, sb):
    for name in ("chain", "log_likelihood", "log_prior", "betas"):
        assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), name
    for name in ("rung_step_size", "rung_acceptance", "swap_acceptance", "betas", "ladder_history"):
        assert np.asarray(getattr(sa, name)).tobytes() == np.asarray(getattr(sb, name)).tobytes(), name
    assert sa.evidence == sb.evidence and sa.swap_acceptance_kept is None and sb.swap_acceptance_kept.shape == sb.swap_acceptance.shape


SHAPES = [(1, 7, 4, 0, "tpcn"), (2, 1, 4, 1, "pcn"), (3, 7, 8, 2, "tpcn"), (5, 7, 4, 5, "pcn"), (5, 1, 8, 1, "tpcn"), (3, 7, 4, 1, "tpcn"),
          (2, 7, 8, 0, "pcn"), (5, 7, 8, 2, "pcn")]


@pytest.mark.parametrize("n_temps,W,d,swap_every,step_fn", SHAPES)
def test_the_two_launch_paths_are_one_chain(n_temps, W, d, swap_every, step_fn):
    """Byte for byte: chain, ll, lp, step sizes, acceptances and evidence; 11 steps, so swap_every = 5 leaves a ragged last segment and
    swap_every = 0 one segment of all steps."""
    kw = dict(n_walkers=W, n_temps=n_temps, n_steps=11, swap_every=swap_every, step_fn=step_fn, burnin=4)
    sa, sb = make(seed=7, d=d), make(seed=7, d=d)
    a = sa.sample(**kw)
    b = sb.sample(rung_launch="batched", **kw)
    assert_same_run(a, sa, b, sb)
    assert sb.engine.calls["pt_steps"] > 0 and sa.engine.calls["pt_steps"] == 0
    assert "asmc_pt_steps" in sb.last_mutation_path and "asmc_pcn_mutate" in sa.last_mutation_path


def test_the_two_paths_agree_across_refits():
    """refit_every = 3 with burnin = 7: segments end at 3 and 6, the references are fitted again and the tables packed again."""
    kw = dict(n_walkers=7, n_temps=3, n_steps=10, swap_every=2, burnin=7, refit_every=3)
    sa, sb = make(seed=1), make(seed=1)
    assert_same_run(sa.sample(**kw), sa, sb.sample(rung_launch="batched", **kw), sb)
    assert sb.engine.calls["pt_pack"] == 3


def test_errors():
    s = lambda **k: make(**k).sample  # noqa: E731
    base = dict(n_walkers=6, n_temps=4, n_steps=8, burnin=4)
    with pytest.raises(ValueError, match="rung_launch must be"):
        s()(rung_launch="fused", **base)
    with pytest.raises(NotImplementedError, match="callables"):
        s(callables=True)(rung_launch="batched", **base)
    with pytest.raises(NotImplementedError, match="d=5"):
        make(d=5, targets=mixture_targets(5)).sample(rung_launch="batched", **base)
    with pytest.raises(NotImplementedError, match="noise='f32'"):
        s()(rung_launch="batched", noise="f32", **base)
    with pytest.raises(ValueError, match="rung_launch='batched'"):
        s()(adapt_ladder=True, **base)
    ad = dict(rung_launch="batched", adapt_ladder=True)
    with pytest.raises(ValueError, match="swap_every >= 1"):
        s()(swap_every=0, **ad, **base)
    with pytest.raises(ValueError, match="at least 3 rungs"):
        s()(**ad, **{**base, "n_temps": 2})
    with pytest.raises(ValueError, match="ends at 0"):
        s()(betas=[1.0, 0.5, 0.1], **ad, **{k: v for k, v in base.items() if k != "n_temps"})
    with pytest.raises(ValueError, match="burnin >= 2 swap_every"):
        s()(swap_every=3, **ad, **{**base, "burnin": 5})
    with pytest.raises(ValueError, match="burnin < n_steps"):
        s()(**ad, **{**base, "burnin": 8})
    with pytest.raises(ValueError, match="ladder_lag and ladder_time"):
        s()(ladder_lag=0.0, **ad, **base)


def test_a_transform_is_outside_the_batched_scope(monkeypatch):
    from aspire_amd import Aspire, Samples
    from aspire_amd import samples as samples_mod

    monkeypatch.setattr(samples_mod, "_default_engine", PTBatchOracleEngine())
    lik, pri = gaussian_targets()
    names = [f"x_{i}" for i in range(GAUSS_D)]
    aspire = Aspire(log_likelihood=lik, log_prior=pri, dims=GAUSS_D, parameters=names, prior_bounds={n: [-12, 12] for n in names},
                    flow_backend="gaussian")
    aspire.fit(Samples(np.random.default_rng(0).normal(size=(400, GAUSS_D))))
    with pytest.raises(NotImplementedError, match="transform"):
        aspire.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=PTBatchOracleEngine(), rng=np.random.default_rng(2), n_walkers=8,
                                n_temps=3, n_steps=6, rung_launch="batched", preconditioning_kwargs={"bounded_to_unbounded": True})


def test_ladder_update_invariants():
    g = np.random.default_rng(3)
    for T in (3, 5, 64):
        b0 = np.concatenate(([1.0], np.sort(g.uniform(1e-3, 0.99, T - 2))[::-1], [0.0]))
        b, snap, counts = b0.copy(), np.zeros(T - 1, dtype=np.int64), np.zeros(T - 1, dtype=np.int64)
        for m in range(1, 6):
            counts = counts + g.integers(0, 101, T - 1)
            b, snap2 = ladder_update_ref(b, counts, snap, 100, m, 10.0, 2.0)
            assert b[0] == 1.0 and b[-1] == 0.0 and np.all(np.diff(b) < 0) and np.array_equal(snap2, counts)
            snap = snap2
        same, _ = ladder_update_ref(b0, np.full(T - 1, 37) + snap, snap, 100, 1, 10.0, 2.0)  # equal acceptances: the gaps stay
        np.testing.assert_allclose(same, b0, rtol=4 * T * np.finfo(float).eps, atol=0)
    # the pair that accepts more than its hotter neighbour widens: its upper rung moves away
    b, _ = ladder_update_ref([1.0, 0.5, 0.1, 0.0], [90, 10, 50], [0, 0, 0], 100, 1, 10.0, 2.0)
    assert b[1] < 0.5


def test_adaptive_run_history_and_frozen_ladder():
    eng = PTBatchOracleEngine()
    s = make(seed=4, eng=eng)
    start = [1.0, 0.9, 0.8, 0.01, 0.0]
    out = s.sample(n_walkers=16, betas=start, n_steps=30, swap_every=2, burnin=13, rung_launch="batched", adapt_ladder=True)
    # odd rounds k with (k + 1) 2 <= 13: k = 1, 3, 5 -> three updates; rounds run to k = 14
    assert eng.calls["pt_ladder_adapt"] == 3 and s.ladder_history.shape == (4, 5)
    assert list(s.ladder_history[0]) == start and np.array_equal(s.ladder_history[-1], s.betas) and np.array_equal(np.asarray(out.betas), s.betas)
    assert np.all(s.ladder_history[:, 0] == 1.0) and np.all(s.ladder_history[:, -1] == 0.0) and np.all(np.diff(s.ladder_history, axis=1) < 0)
    assert not np.array_equal(s.ladder_history[1], s.ladder_history[0])
    assert "asmc_pt_ladder_adapt" in s.last_mutation_path and out.chain_shape == (5, 17, 16)
    # the evidence: the kept steps alone, no further burn-in fraction
    full = make(seed=4).sample(n_walkers=16, betas=start, n_steps=30, swap_every=2, burnin=13, rung_launch="batched", adapt_ladder=True)
    assert s.evidence == {"thermodynamic_integration": full.log_evidence_thermodynamic_integration(burn_in_fraction=None),
                          "stepping_stone": full.log_evidence_stepping_stone(burn_in_fraction=None)}
    # without adaptation nothing moves and the history is the ladder
    q = make(seed=4)
    q.sample(n_walkers=16, betas=start, n_steps=6, rung_launch="batched")
    assert q.engine.calls["pt_ladder_adapt"] == 0 and q.ladder_history.shape == (1, 5) and list(q.betas) == start


UNEVEN = [1.0, 0.9, 0.8, 0.01, 0.0]


def uneven_run(seed, adapt, eng=None, n_walkers=64, n_steps=400, **kw):
    s = make(seed=seed, eng=eng, **kw)
    out = s.sample(n_walkers=n_walkers, betas=UNEVEN, n_steps=n_steps, burnin=n_steps // 2, swap_every=1, rung_launch="batched", adapt_ladder=adapt)
    return s, out


def uneven_check(s, out, fixed):
    """The assertions the CPU and the GPU form of the statistical check share; `fixed`: the same run on the fixed ladder."""
    betas = np.asarray(out.betas)
    assert betas[0] == 1.0 and betas[-1] == 0.0 and np.all(np.diff(betas) < 0) and not np.array_equal(betas, UNEVEN)
    mean_ll, logz = gaussian_closed_form(pt_ref.GAUSS_M, pt_ref.GAUSS_SP2, pt_ref.GAUSS_SL2, betas)
    z_mean, z_ti, z_ss = pt_z_scores(np.asarray(out.log_likelihood).reshape(out.chain_shape), betas, mean_ll, logz)
    spread = lambda a: float(np.max(a) - np.min(a))  # noqa: E731
    print("final ladder", betas, "z(rung means)", np.round(z_mean, 2), "z(TI)", round(z_ti, 2), "z(SS)", round(z_ss, 2), "swaps kept: adaptive",
          np.round(s.swap_acceptance_kept, 3), "fixed", np.round(fixed.swap_acceptance_kept, 3), s.evidence, "log Z", logz)
    assert np.all(np.abs(z_mean) < 5.0) and abs(z_ti) < 5.0 and abs(z_ss) < 5.0
    assert spread(s.swap_acceptance_kept) < spread(fixed.swap_acceptance_kept)


def test_uneven_ladder_evens_out_and_keeps_the_closed_form():
    """The problem of DESIGN.md section 3.21 (d = 4, prior N(0, 4 I), likelihood N(x; m, 0.25 I), 64 walkers, 400 steps, half discarded,
    swap_every = 1) from the ladder [1, 0.9, 0.8, 0.01, 0] with adapt_ladder=True: every rung's mean log-likelihood on the FINAL ladder,
    the stepping-stone and the TI log Z within 5 standard errors of their closed forms, and - same seed - the spread (max - min) of the
    pairs' swap acceptance over the kept steps below that of the run on the fixed ladder.  Every pair (r, r + 1) has an interior rung
    at one end at least, so all T - 1 of them count.  Over 8 seeds on this restatement, before the bound was fixed, the largest |z|
    of the 56 statistics: DESIGN.md section 3.22."""
    s, out = uneven_run(3, True)
    fixed, _ = uneven_run(3, False)
    assert out.chain_shape == (5, 200, 64) and s.ladder_history.shape == (101, 5)
    uneven_check(s, out, fixed)
