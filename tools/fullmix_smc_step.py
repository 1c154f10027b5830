"""Per-step time of one `sampler="smc"` run (pCN, 32 steps per temperature) at 1M x 32 fp64 with a correlated Gaussian likelihood
(condition number 100) under a standard-normal DiagGaussianMixture prior and a Gaussian proposal.  MODE=kernel: the likelihood is a
GaussianMixture (asmc_fullmix_logpdf); MODE=callable: the same density written as a torch callable, `xp=torch` - the only form a
tree without the class can run, so this script also runs from the parent commit's tree (ROOT=<that tree>).  Prints one JSON line:
wall time of the run behind a device synchronise, over temperatures x steps.
"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd.engine import HipEngine  # noqa: E402
from aspire_amd.flows import GaussianFlow  # noqa: E402
from aspire_amd.samplers.smc import HipSMC  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402


def main():
    assert torch.cuda.is_available(), "fullmix_smc_step.py needs a HIP device"
    mode = os.environ.get("MODE", "kernel")
    n, d, steps = int(os.environ.get("N", 1_000_000)), int(os.environ.get("D", 32)), int(os.environ.get("STEPS", 32))
    g = np.random.default_rng(2024)
    Q = np.linalg.qr(g.normal(size=(d, d)))[0]
    Sigma = (Q * np.geomspace(0.1, 10.0, d)) @ Q.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    m = 0.5 * g.normal(size=d)
    eng = HipEngine(0, n_max=n, d_max=d)
    if mode == "kernel":
        from aspire_amd import GaussianMixture

        lik, xp = GaussianMixture(m, Sigma), np
    else:
        W = torch.as_tensor(np.linalg.inv(np.linalg.cholesky(Sigma)), device=eng.device)
        mt = torch.as_tensor(m, device=eng.device)
        logw = -0.5 * d * math.log(2 * math.pi) + float(torch.log(torch.diagonal(W)).sum())

        def lik(smp):
            v = (smp.x.to(torch.float64) - mt) @ W.T
            return logw - 0.5 * (v * v).sum(1)

        xp = torch
    prior = DiagGaussianMixture.isotropic(d)
    runs = []
    for rep in range(int(os.environ.get("REPS", 3))):
        sp = HipSMC(log_likelihood=lik, log_prior=prior, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, seed=rep, engine=eng), xp=xp,
                    engine=eng, rng=np.random.default_rng(100 + rep))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sp.sample(n, sampler_kwargs=dict(n_steps=steps, step_fn="pcn"), store_sample_history=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        temps = max(1, len(sp.history.beta))
        runs.append(dict(seconds=round(dt, 4), temperatures=temps, ms_per_step=round(1e3 * dt / (temps * steps), 4),
                         log_evidence=round(float(out.log_evidence), 4), path=sp.last_mutation_path))
    print(json.dumps(dict(mode=mode, tree=os.path.relpath(ROOT), shape=f"{n}x{d} fp64", steps_per_temperature=steps, runs=runs)))


if __name__ == "__main__":
    main()
