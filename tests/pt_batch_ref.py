"""CPU restatement of the rung-batched entry points (include/asmc.h asmc_pt_steps_supported / _pack / _steps / _ladder_adapt, DESIGN.md
section 3.22): TEST INFRASTRUCTURE.

`PTBatchOracleEngine` is `PTOracleEngine` (tests/pt_ref.py) plus `pt_steps_supported`, `pt_pack`, `pt_steps` - loops over the existing
oracle `pcn_mutate`, one call per rung on the rung's rows at beta_r with gid0 = r W, which is the specification of the batched kernel -
and `pt_ladder_adapt`, which applies `ladder_update_ref`, the ladder update in numpy.  The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

from chain_ref import OracleChain
from pt_ref import PTOracleEngine, _np


def ladder_update_ref(betas, counts, snap, n_walkers: int, update: int, lag: float, time: float):
    """Update number `update` = m >= 1 of a ladder that starts at 1 and ends at 0: (new betas [T], new snap [T - 1]).
    A_r = (counts[r] - snap[r]) / W; kappa = lag / (time (m - 1 + lag)); the gap g_i = 1 / beta_i - 1 / beta_{i-1} becomes
    g_i exp(kappa (A_{i-1} - A_i)) for i = 1 .. T - 2, and 1 / beta_i = 1 + g_1 + ... + g_i summed in index order.  The ends stay."""
    b = np.array(betas, dtype=np.float64)
    T = b.size
    counts, snap = np.asarray(counts, dtype=np.int64)[:T - 1], np.asarray(snap, dtype=np.int64)[:T - 1]
    A = (counts - snap).astype(np.float64) / np.float64(n_walkers)
    kappa = np.float64(lag) / (np.float64(time) * (np.float64(update - 1) + np.float64(lag)))
    inv_prev, total = np.float64(1.0) / b[0], np.float64(1.0)
    for i in range(1, T - 1):
        inv = np.float64(1.0) / b[i]
        g = (inv - inv_prev) * np.exp(kappa * (A[i - 1] - A[i]))
        inv_prev = inv
        total = total + g
        b[i] = np.float64(1.0) / total
    return b, counts.copy()


class PTBatchOracleEngine(PTOracleEngine):
    """Counts the calls, so that a test can tell which path a run took."""

    def __init__(self):
        super().__init__()
        self.calls = {"pt_pack": 0, "pt_steps": 0, "pt_ladder_adapt": 0}

    def pt_steps_supported(self, x):
        return x.shape[1] in (4, 8, 16, 32)

    def pt_pack(self, x, n_temps, refs, t_ll, t_lp, t_lq):
        assert x.shape[0] % n_temps == 0 and len(refs) == n_temps and self.pt_steps_supported(x)
        self.calls["pt_pack"] += 1
        return {"n_temps": n_temps, "n_walkers": x.shape[0] // n_temps, "mixes": (t_ll, t_lp, t_lq),
                "refs": [(mu.clone(), L.clone(), Linv.clone(), float(nu)) for mu, L, Linv, nu in refs]}

    def pt_steps(self, pack, x, ll, lp, lq, betas, rho, accept, seed, n_steps, step0=0, target_accept=0.234, adapt=True, chain=None,
                 n_slots=0, slot0=0):
        T, W = pack["n_temps"], pack["n_walkers"]
        assert x.shape[0] == T * W and betas.numel() == T and rho.numel() == T and accept.numel() == T and accept.dtype == torch.int64
        self.calls["pt_steps"] += 1
        d = x.shape[1]
        held = self._chain_target
        try:
            for r in range(T):
                sl = slice(r * W, (r + 1) * W)
                mu, L, Linv, nu = pack["refs"][r]
                self._chain_target = None
                if chain is not None:
                    self._chain_target = (OracleChain(chain.x.view(T, n_slots, W, d)[r], chain.ll.view(T, n_slots, W)[r],
                                                      chain.lp.view(T, n_slots, W)[r]), int(slot0), 1)
                n_acc, _, rho_out = self.pcn_mutate(x[sl], ll[sl], lp[sl], lq[sl], float(betas[r]), mu, L, Linv, *pack["mixes"], int(seed), r * W,
                                                    float(rho[r]), int(n_steps), int(step0), target_accept, bool(adapt), "f64", nu)
                rho[r] = rho_out
                accept[r] += int(np.sum(n_acc))
        finally:
            self._chain_target = held

    def pt_ladder_adapt(self, n_walkers, counts, snap, betas, history, update, lag, time):
        self.calls["pt_ladder_adapt"] += 1
        T = betas.numel()
        b, s = ladder_update_ref(_np(betas), _np(counts), _np(snap), n_walkers, update, lag, time)
        betas.copy_(torch.from_numpy(b))
        snap[:T - 1] = torch.from_numpy(s)
        history[update].copy_(betas)
