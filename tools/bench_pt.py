"""What parallel tempering costs: the "pt_minipcn" sampler with built-in mixture densities at T rungs x W walkers x 32 fp64 (default
8 x 128k), against T independent "minipcn" runs of W walkers; the exchange kernel; the evidence reductions.

Per-round times are the difference between a run of S2 and one of S1 steps over S2 - S1, the median of REPS such pairs after a
warm-up pair (tools/bench_mcmc.py).  The exchange kernel's time is the library's own per-kernel event timing over a run with
swap_every = 1; its traffic is 2 rows read and 2 written per accepted pair plus the two log-likelihoods every pair reads.  The
evidence reductions are timed on the full recorded chain of the S2 run (wall time of the call, which ends in its one
synchronisation) next to asmc_weights_stats on three arrays of the same total size.  Prints one JSON line.
Env: T, W, S1, S2, REPS, STEP_FN=pcn|tpcn.
--rung-launch per_rung|batched: how the rungs' steps are launched; --adapt-ladder: the ladder adapts until
the last step of the run (batched only; swap_every = 1 alone is timed); --rounds-only: the per-round times alone."""
import argparse
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
from aspire_amd.samplers.mcmc import HipMiniPCN, HipPTMiniPCN  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402

D = 32


def sampler(cls, eng):
    lik = DiagGaussianMixture.isotropic(D, mean=1.0, var=1.0, normalized=True)
    pri = DiagGaussianMixture.isotropic(D, mean=0.0, var=4.0, normalized=True)
    return cls(log_likelihood=lik, log_prior=pri, dims=D, prior_flow=GaussianFlow(D, sigma=1.5, seed=3, engine=eng), xp=torch, engine=eng,
               rng=np.random.default_rng(1))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


LAUNCH = {}  # the sampler keywords the command line adds


def pt_run(eng, n_temps, w, steps, swap_every, step_fn):
    s = sampler(HipPTMiniPCN, eng)
    kw = dict(LAUNCH, burnin=steps - 1) if LAUNCH.get("adapt_ladder") else LAUNCH  # (the ladder moves through all but the last step)
    dt, out = timed(lambda: s.sample(n_walkers=w, n_temps=n_temps, n_steps=steps, swap_every=swap_every, step_fn=step_fn, **kw))
    return dt, s, out


def independent_run(eng, n_temps, w, steps, step_fn):
    """T separate minipcn runs of W walkers, one after the other (each records its chain)."""
    total = 0.0
    for _ in range(n_temps):
        s = sampler(HipMiniPCN, eng)
        dt, out = timed(lambda: s.sample(n_walkers=w, n_steps=steps, step_fn=step_fn))
        total += dt
        del out, s
    torch.cuda.empty_cache()
    return total


def per_step(run, s1, s2, reps):
    vals = []
    for r in range(reps + 1):
        a, b = run(s1), run(s2)
        if r:  # (the first pair warms up: code objects, the allocator's pool)
            vals.append((b - a) / (s2 - s1))
    return statistics.median(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rung-launch", choices=("per_rung", "batched"), default="per_rung")
    ap.add_argument("--adapt-ladder", action="store_true")
    ap.add_argument("--rounds-only", action="store_true")
    args = ap.parse_args()
    LAUNCH.update(rung_launch=args.rung_launch)
    if args.adapt_ladder:
        LAUNCH.update(adapt_ladder=True)
    n_temps, w = int(os.environ.get("T", 8)), int(os.environ.get("W", 1 << 17))
    s1, s2, reps = int(os.environ.get("S1", 8)), int(os.environ.get("S2", 40)), int(os.environ.get("REPS", 3))
    step_fn = os.environ.get("STEP_FN", "tpcn")
    eng = HipEngine(0, n_max=n_temps * w, d_max=D)
    res = {"n_temps": n_temps, "n_walkers": w, "d": D, "step_fn": step_fn, "rung_launch": args.rung_launch, "adapt_ladder": args.adapt_ladder}

    def pt_time(swap_every):
        def run(steps):
            dt, s, out = pt_run(eng, n_temps, w, steps, swap_every, step_fn)
            del out, s
            torch.cuda.empty_cache()
            return dt
        return per_step(run, s1, s2, reps)

    for k in ((1,) if args.adapt_ladder else (0, 1, 8)):
        res[f"ms_per_step_swap_every_{k}"] = round(1e3 * pt_time(k), 4)
    if args.rounds_only:
        print(json.dumps(res))
        return
    res["ms_per_step_independent_minipcn"] = round(1e3 * per_step(lambda steps: independent_run(eng, n_temps, w, steps, step_fn), s1, s2, reps), 4)

    # the exchange kernel at the acceptance of a real run
    eng.profile(True)
    _, s, out = pt_run(eng, n_temps, w, s2, 1, step_fn)
    rep = eng.profile_report()
    eng.profile(False)
    launches, avg_ms = rep["k_pt_swap"]
    tries = np.array([len(range(r % 2, s2, 2)) for r in range(n_temps - 1)]) * w
    accepted = float(np.sum(s.swap_acceptance * tries))
    nbytes = (accepted * 4 * D * 8 + float(tries.sum()) * 16) / launches
    res.update(swap_launches=launches, swap_ms=round(avg_ms, 5), swap_acceptance=[round(float(v), 3) for v in s.swap_acceptance],
               swap_bytes_per_launch=int(nbytes), swap_TB_per_s=round(nbytes / (avg_ms * 1e-3) / 1e12, 3), path=s.last_mutation_path)

    # the evidence reductions over the full chain of that run, and asmc_weights_stats over as many bytes
    ll = out.log_likelihood
    stride = s2 * w
    coef = np.stack([np.full(n_temps, 1.0 / n_temps), np.full(n_temps, 0.1)])
    eng.pt_evidence(ll, n_temps, stride, 0, stride, coef)
    t_ev = statistics.median(timed(lambda: eng.pt_evidence(ll, n_temps, stride, 0, stride, coef))[0] for _ in range(5))
    third = ll.numel() // 3
    a, b, c = (ll[i * third:(i + 1) * third] for i in range(3))
    eng.ensure_capacity(third, D)
    eng.weights_stats(a, b, c, 0.0, [1.0])
    t_ws = statistics.median(timed(lambda: eng.weights_stats(a, b, c, 0.0, [1.0]))[0] for _ in range(5))
    res.update(evidence_bytes=ll.numel() * 8, evidence_ms=round(1e3 * t_ev, 4), evidence_TB_per_s=round(ll.numel() * 8 / t_ev / 1e12, 3),
               weights_stats_ms=round(1e3 * t_ws, 4), weights_stats_TB_per_s=round(3 * third * 8 / t_ws / 1e12, 3),
               evidence=s.evidence)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
