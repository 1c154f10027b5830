"""Micro-driver of one stretch-move step (both half-sweeps) of the "emcee_smc" mutation at 1M x 32 fp64: the step exactly as
HipEmceeSMC.mutate enqueues it (propose -> log q -> built-in log prior / log likelihood -> accept, twice), timed with events over
STEPS steps after a warm-up, for two proposals: the analytic Gaussian with the built-in mixture target, and a coupling flow
(fp32 MFMA log-density kernel).  Prints ms per step, the acceptance and the per-kernel HIP-event table (PROFILE=1).
Env: N, STEPS, KIND=gaussian|coupling|both."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import random_coupling_flow  # noqa: E402

from aspire_amd.engine import HipEngine  # noqa: E402
from aspire_amd.flows import GaussianFlow  # noqa: E402
from aspire_amd.moves import MoveSpec, run_step  # noqa: E402
from aspire_amd.samplers.emcee_smc import HipEmceeSMC  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402


def bench(eng, kind, n, d, steps):
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    flow = GaussianFlow(d, sigma=1.5, seed=3, engine=eng) if kind == "gaussian" else random_coupling_flow(d, 4, 64, device=eng.device)
    sp = HipEmceeSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=flow, xp=np, engine=eng, rng=np.random.default_rng(1))
    x, lq = GaussianFlow(d, sigma=1.5, seed=5, engine=eng).sample_and_log_prob(n)
    x = eng.asarray(x)
    lq = sp._flow_log_prob(x)
    lp, ll = sp._eval_prior_likelihood(x, lq)
    beta, seed = 0.5, 12345

    spec = MoveSpec("stretch", 2, 2.0)

    def step(t, tc):
        run_step(eng, spec, d, x, beta, ll, lp, lq, None, lambda y: sp._proposal_densities(y, None, x.dtype)[1:], seed, 0, t, tc)

    for t in range(3):
        step(t, t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prof = os.environ.get("PROFILE") == "1"
    if prof:
        eng.profile(True)
    e0.record()
    for t in range(steps):
        step(100 + t, t)
    e1.record()
    torch.cuda.synchronize()
    acc = eng.stretch_counts(steps).sum() / (n * steps)
    print(f"stretch step {kind:8s} n={n} d={d} fp64: {e0.elapsed_time(e1) / steps:.3f} ms per step (both halves), acceptance {acc:.3f}")
    if prof:
        for k, (cnt, ms) in sorted(eng.profile_report().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            print(f"  {k:32s} {cnt:6d} launches {ms * 1e3:9.1f} us avg")
        eng.profile(False)


def main():
    n, d, steps = int(os.environ.get("N", 1_000_000)), 32, int(os.environ.get("STEPS", 50))
    kinds = os.environ.get("KIND", "both")
    eng = HipEngine(0, n_max=n, d_max=d)
    for kind in ("gaussian", "coupling"):
        if kinds in ("both", kind):
            bench(eng, kind, n, d, steps)


if __name__ == "__main__":
    main()
