"""Micro-driver of one Markov step of each ensemble move of the "emcee_smc" mutation at 1M x 32 fp64: the step exactly as
HipEmceeSMC.mutate enqueues it (per group-sweep: propose -> log q -> built-in log prior / log likelihood -> accept), with the
analytic Gaussian proposal and the built-in mixture target, for the stretch move, the DE move, the snooker move and the 0.8 / 0.2
DE / snooker mixture, one after the other in one process.  Timed with events over STEPS steps after a warm-up; prints ms per step
and the acceptance of each, and the bytes a slot moves in each new kernel.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py`, or PROFILE=1 for the engine's HIP-event table.
Env: N, STEPS, MOVES (comma list of stretch,de,snooker,mixture)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd import DEMove, DESnookerMove, StretchMove  # noqa: E402
from aspire_amd.engine import HipEngine  # noqa: E402
from aspire_amd.flows import GaussianFlow  # noqa: E402
from aspire_amd.moves import parse_moves, run_step  # noqa: E402
from aspire_amd.samplers.emcee_smc import HipEmceeSMC  # noqa: E402
from aspire_amd.targets import DiagGaussianMixture  # noqa: E402

MOVES = {"stretch": [StretchMove()], "de": DEMove(), "snooker": DESnookerMove(), "mixture": [(DEMove(), 0.8), (DESnookerMove(), 0.2)]}


def bench(eng, name, n, d, steps):
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    sp = HipEmceeSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=1.5, seed=3, engine=eng), xp=np,
                     engine=eng, rng=np.random.default_rng(1))
    x, lq = GaussianFlow(d, sigma=1.5, seed=5, engine=eng).sample_and_log_prob(n)
    x = eng.asarray(x)
    lq = sp._flow_log_prob(x)
    lp, ll = sp._eval_prior_likelihood(x, lq)
    beta, seed = 0.5, 12345
    move_set = parse_moves(MOVES[name])
    schedule = move_set.schedule(seed, steps + 3)

    def step(t, tc):
        run_step(eng, move_set.specs[schedule[tc]], d, x, beta, ll, lp, lq, None,
                 lambda y: sp._proposal_densities(y, None, x.dtype)[1:], seed, 0, t, tc)

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
    ms = e0.elapsed_time(e1) / steps
    print(f"ensemble step {name:8s} ({move_set.names}) n={n} d={d} fp64: {ms:.3f} ms per step (all group-sweeps), acceptance {acc:.3f}")
    if prof:
        for k, (cnt, kms) in sorted(eng.profile_report().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            print(f"  {k:32s} {cnt:6d} launches {kms * 1e3:9.1f} us avg")
        eng.profile(False)
    return ms, float(acc)


def main():
    n, d, steps = int(os.environ.get("N", 1_000_000)), 32, int(os.environ.get("STEPS", 50))
    names = os.environ.get("MOVES", "stretch,de,snooker,mixture").split(",")
    eng = HipEngine(0, n_max=n, d_max=d)
    row = 8 * d
    # a slot reads its partners' rows and its own and writes y (propose); the accept reads y and four densities per slot and, where
    # it accepts, writes a row and three densities
    print(f"bytes per slot at d={d} fp64: k_de_propose {3 * row + row + 8} (3 rows read, y and logf written), k_snooker_propose "
          f"{4 * row + row + 8} (4 rows read), k_ensemble_accept {row + 7 * 8} read + up to {row + 3 * 8} written")
    res = {name: bench(eng, name, n, d, steps) for name in names}
    if "stretch" in res:
        for name, (ms, _) in res.items():
            print(f"{name:8s} {ms:.3f} ms = {ms / res['stretch'][0]:.2f} x the stretch step")


if __name__ == "__main__":
    main()
