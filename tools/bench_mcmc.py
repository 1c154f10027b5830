"""What recording costs: the "minipcn" sampler with built-in mixture densities at N x 32 fp64 (default N = 1M), with the chain
recorder on and with last_step_only (nothing recorded).

A run of S steps costs setup (the flow's draw, the reference fit, the chain's allocation) plus S steps; the time per step is the
difference between a run of S2 and one of S1 steps over S2 - S1, the median of REPS such pairs after a warm-up pair.  The recorder's
cost per step is the difference of the two modes; per step it reads the state once and writes n d 8 bytes of rows (plus 16 n of
densities), so its achieved bandwidth is 2 n d 8 / cost.  Prints one JSON line.  Env: N, S1, S2, REPS, STEP_FN=pcn|tpcn.
(In asmc_pcn_mutate's loop the record is the un-whitening launch, which also re-evaluates the three densities at the stored row.)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd.engine import HipEngine  # noqa: E402
from aspire_amd.flows import GaussianFlow  # noqa: E402
from aspire_amd.samplers.mcmc import HipMiniPCN  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402


def one_run(eng, n, d, steps, last_step_only, step_fn):
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    s = HipMiniPCN(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, seed=3, engine=eng), xp=torch,
                   engine=eng, rng=np.random.default_rng(1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = s.sample(n_walkers=n, n_steps=steps, last_step_only=last_step_only, step_fn=step_fn)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    path = s.last_mutation_path
    del out, s
    torch.cuda.empty_cache()
    return dt, path


def per_step(eng, n, d, s1, s2, reps, last_step_only, step_fn):
    vals, path = [], None
    for r in range(reps + 1):
        a, path = one_run(eng, n, d, s1, last_step_only, step_fn)
        b, _ = one_run(eng, n, d, s2, last_step_only, step_fn)
        if r:  # (the first pair warms up: code objects, the allocator's pool)
            vals.append((b - a) / (s2 - s1))
    return statistics.median(vals), path


def main():
    n, d = int(os.environ.get("N", 1 << 20)), 32
    s1, s2, reps = int(os.environ.get("S1", 8)), int(os.environ.get("S2", 40)), int(os.environ.get("REPS", 3))
    step_fn = os.environ.get("STEP_FN", "pcn")
    eng = HipEngine(0, n_max=n, d_max=d)
    t_last, path = per_step(eng, n, d, s1, s2, reps, True, step_fn)
    t_rec, _ = per_step(eng, n, d, s1, s2, reps, False, step_fn)
    cost = t_rec - t_last
    print(json.dumps({"n": n, "d": d, "step_fn": step_fn, "path": path, "ms_per_step_last_step_only": round(1e3 * t_last, 4),
                      "ms_per_step_recording": round(1e3 * t_rec, 4), "recorder_ms_per_step": round(1e3 * cost, 4),
                      "recorder_bytes_per_step": 2 * n * d * 8,
                      "recorder_TB_per_s": round(2 * n * d * 8 / cost / 1e12, 3) if cost > 0 else None}))


if __name__ == "__main__":
    main()
