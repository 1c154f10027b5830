"""Micro-driver of the "blackjax_smc" mutations at 1M x 32 fp64, exactly as HipBlackJAXSMC.mutate enqueues them, timed with events
after a warm-up:
  hmc fused   transitions of num_integration_steps = 10 on the built-in mixtures (one k_hmc_mix launch for all of them)
  hmc split   the same mixtures wrapped as torch callables: momentum / leapfrog / accept launches around torch.autograd gradients
  rwmh        propose -> log q -> built-in log prior / log likelihood -> accept per step
Prints ms per transition (or step), the acceptance and, with PROFILE=1, the per-kernel HIP-event table.
Env: N, D, STEPS (fused / rwmh; the split path runs STEPS_SPLIT), LEAP, EPS, KIND=fused|split|rwmh|all.
`--algorithm nuts`: the fused HMC kernel (the yardstick, ms per leapfrog step) and then, in the same process, the fused NUTS kernel
(k_nuts_mix) on the same target at step_size EPS: STEPS_NUTS transitions, ms per transition and per leapfrog step (time over the mean
number of steps a row takes), mean depth and steps, and the means of their per-wave maxima - a wave runs until its longest tree ends."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd.engine import HipEngine  # noqa: E402
from aspire_amd.flows import GaussianFlow  # noqa: E402
from aspire_amd.history import SMCHistory  # noqa: E402
from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402


def bench(eng, kind, n, d, steps, n_leap, eps):
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    as_callables = kind == "split"
    f = (lambda s: lik(s.x)) if as_callables else lik
    sp = HipBlackJAXSMC(log_likelihood=f, log_prior=f, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, seed=3, engine=eng),
                        xp=torch if as_callables else np, engine=eng, rng=np.random.default_rng(1))
    sp.sampler_kwargs = {"algorithm": "rwmh" if kind == "rwmh" else "hmc", "step_size": eps, "num_integration_steps": n_leap,
                         "sigma": 2.38 / np.sqrt(d) * 0.7, "inverse_mass_matrix": None, "n_steps": steps}
    sp.key = 42
    sp._check_options()
    x, _ = GaussianFlow(d, sigma=1.5, seed=5, engine=eng).sample_and_log_prob(n)
    x = eng.asarray(x)
    lq = eng.mixture_logpdf(x, sp.prior_flow.device_mixture(eng))
    ll = eng.mixture_logpdf(x, lik.device_mixture(eng))
    parts = sp._wrap(x, ll, ll.clone(), lq, 0.5)
    sp.history = SMCHistory()
    parts = sp.mutate(parts, 0.5, n_steps=2)  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prof = os.environ.get("PROFILE") == "1"
    if prof:
        eng.profile(True)
    e0.record()
    sp.mutate(parts, 0.5, n_steps=steps)
    e1.record()
    torch.cuda.synchronize()
    unit = "step" if kind == "rwmh" else f"transition of {n_leap} leapfrog steps"
    print(f"{kind:6s} n={n} d={d} fp64: {e0.elapsed_time(e1) / steps:.3f} ms per {unit}, acceptance {sp.history.mcmc_acceptance[-1]:.3f} "
          f"({sp.last_mutation_path})")
    if prof:
        for k, (cnt, ms) in sorted(eng.profile_report().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            print(f"  {k:32s} {cnt:6d} launches {ms * 1e3:9.1f} us avg")
        eng.profile(False)


def bench_nuts(eng, n, d, steps, eps):
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    sp = HipBlackJAXSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, seed=3, engine=eng), xp=np,
                        engine=eng, rng=np.random.default_rng(1))
    sp.sampler_kwargs = {"algorithm": "nuts", "step_size": eps, "num_integration_steps": 10, "inverse_mass_matrix": None, "n_steps": steps,
                         "max_num_doublings": 10, "divergence_threshold": 1000.0}
    sp.key = 42
    sp._check_options()
    x, _ = GaussianFlow(d, sigma=1.5, seed=5, engine=eng).sample_and_log_prob(n)
    x = eng.asarray(x)
    lq = eng.mixture_logpdf(x, sp.prior_flow.device_mixture(eng))
    ll = eng.mixture_logpdf(x, lik.device_mixture(eng))
    parts = sp._wrap(x, ll, ll.clone(), lq, 0.5)
    sp.history = SMCHistory()
    parts = sp.mutate(parts, 0.5, n_steps=1)  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    parts = sp.mutate(parts, 0.5, n_steps=steps)
    e1.record()
    torch.cuda.synchronize()
    ms, last = e0.elapsed_time(e1) / steps, sp.last_nuts
    print(f"nuts   n={n} d={d} fp64 step_size={eps}: {ms:.3f} ms per transition, {last['steps_per_transition']:.2f} leapfrog steps per "
          f"transition, {ms / last['steps_per_transition']:.4f} ms per leapfrog step, acceptance {sp.history.mcmc_acceptance[-1]:.3f}, "
          f"divergent share {last['divergent_share']:.2e} ({sp.last_mutation_path})")
    # one more transition with the per-row output: what a wave pays is its longest tree
    mixes = (lik.device_mixture(eng), lik.device_mixture(eng), sp.prior_flow.device_mixture(eng))
    info = eng.nuts_mix(parts.x, parts.log_likelihood, parts.log_prior, parts.log_q, 0.5, *mixes, None, eps, 10, 1000.0, 7, 0, 0, 1,
                        want_info=True).cpu().numpy()
    lanes = 1 << max(0, int(np.ceil(np.log2(max(1, (d + 3) // 4)))))
    rows = 64 // lanes  # rows of one wave
    m = (n // rows) * rows
    depth, leaps = info[:m, 0].reshape(-1, rows), info[:m, 1].reshape(-1, rows)
    print(f"       depth: mean {info[:, 0].mean():.3f}, mean of the per-wave maximum {depth.max(axis=1).mean():.3f}, largest {info[:, 0].max()}; "
          f"leapfrog steps: mean {info[:, 1].mean():.2f}, mean of the per-wave maximum {leaps.max(axis=1).mean():.2f} ({rows} rows per wave)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--algorithm", choices=("hmc", "nuts"), default="hmc")
    args = ap.parse_args()
    n, d = int(os.environ.get("N", 1_000_000)), int(os.environ.get("D", 32))
    steps, steps_split = int(os.environ.get("STEPS", 50)), int(os.environ.get("STEPS_SPLIT", 5))
    n_leap, eps = int(os.environ.get("LEAP", 10)), float(os.environ.get("EPS", 0.1))
    kinds = os.environ.get("KIND", "all")
    eng = HipEngine(0, n_max=n, d_max=max(d, 32))
    if args.algorithm == "nuts":
        bench(eng, "fused", n, d, steps, n_leap, eps)
        bench_nuts(eng, n, d, int(os.environ.get("STEPS_NUTS", 10)), eps)
        return
    for kind in ("fused", "split", "rwmh"):
        if kinds in ("all", kind):
            bench(eng, kind, n, d, steps_split if kind == "split" else steps, n_leap, eps)


if __name__ == "__main__":
    main()
