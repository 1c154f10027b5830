"""CPU restatement of the chain recorder (include/asmc.h asmc_chain_*) on the oracle-backed engine double: TEST INFRASTRUCTURE.

`ChainOracleEngine` is `StretchOracleEngine` (tests/stretch_ref.py, itself tests/oracle_engine.py's `OracleEngine`) plus
`free_memory`, `chain_alloc`, `chain_record`, `chain_set` / `chain_clear` and a `pcn_mutate` whose step loop honours the target -
what the "minipcn" / "emcee" samplers ask of an engine beyond what the SMC samplers do.  `closed_form_moments` and `moment_z_scores`
are the statistical check the CPU and the GPU sampler tests share.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle_engine as OE
from stretch_ref import StretchOracleEngine

O = OE.O
_np = OE._np


class OracleChain:
    def __init__(self, x, ll, lp):
        self.x, self.ll, self.lp = x, ll, lp


class ChainOracleEngine(StretchOracleEngine):
    free_bytes = 1 << 40  # what `free_memory` reports (a test of the guard lowers it)

    def __init__(self):
        super().__init__()
        self._chain_target = None
        self.chain_allocs = 0

    def free_memory(self):
        return self.free_bytes

    def chain_alloc(self, n_slots, n, d, dtype=torch.float64):
        self.chain_allocs += 1
        return OracleChain(torch.full((n_slots, n, d), float("nan"), dtype=dtype), torch.full((n_slots, n), float("nan"), dtype=torch.float64),
                           torch.full((n_slots, n), float("nan"), dtype=torch.float64))

    def chain_record(self, chain, slot, x=None, ll=None, lp=None, sess=None, transform=None):
        assert 0 <= slot < chain.x.shape[0]
        if sess is not None:  # what pcn_ysplit_end writes, without ending the session
            rows = torch.from_numpy((sess["mu"] + sess["y"] @ sess["L"].T).astype(sess["npdt"]))
        elif transform is not None:
            rows = self.transform_inverse(x, transform, want_logj=False)[0]
        else:
            rows = x
        chain.x[slot].copy_(rows)
        if ll is not None:
            chain.ll[slot].copy_(ll)
        if lp is not None:
            chain.lp[slot].copy_(lp)

    def chain_set(self, chain, slot0, stride=1):
        self._chain_target = (chain, int(slot0), int(stride))

    def chain_clear(self):
        self._chain_target = None

    def pcn_mutate(self, x, ll, lp, lq, beta, mu, L, Linv, t_ll, t_lp, t_lq, seed, gid0, rho, n_steps, step0=0, target_accept=0.234,
                   adapt=True, noise="f64", nu=0.0):
        if self._chain_target is None:
            return super().pcn_mutate(x, ll, lp, lq, beta, mu, L, Linv, t_ll, t_lp, t_lq, seed, gid0, rho, n_steps, step0, target_accept,
                                      adapt, noise, nu)
        chain, slot0, stride = self._chain_target
        assert int(adapt) in (0, 1) and getattr(self, "_count_hook", None) is None
        n = x.shape[0]
        n_acc, hist = np.zeros(n_steps, dtype=np.int64), np.zeros(n_steps)
        for t in range(n_steps):  # OracleEngine.pcn_mutate's loop, one rank, no lag, with the record behind every step
            hist[t] = rho
            args = (_np(x), _np(ll), _np(lp), _np(lq), beta, _np(mu), _np(L), _np(Linv), rho)
            if nu > 0.0:
                c = O.tpcn_step(*args, nu, t_ll.mix, t_lp.mix, t_lq.mix, seed, gid0, step0 + t, noise)
            else:
                c = O.pcn_step(*args, t_ll.mix, t_lp.mix, t_lq.mix, seed, gid0, step0 + t, noise)
            n_acc[t] = int(c)
            if adapt:
                rho = O.pcn_adapt(rho, int(c) / n, target_accept, t)
            if t % stride == stride - 1:
                self.chain_record(chain, slot0 + t // stride, x=x, ll=ll, lp=lp)
        return n_acc, hist, rho


def moment_z_scores(chain: np.ndarray, mean: np.ndarray, var: np.ndarray):
    """z-scores of the chain's mean and variance per coordinate against the closed form, with standard errors from THIS run's own
    effective sample size.  chain: [n_steps, n_walkers, d].  The walkers are n_w chains of the same law - independent for pCN,
    coupled only through the complementary half for the stretch move - so the spread of their time averages measures what one
    walker's average is worth: with m_w the time average of f over walker w and s^2 their sample variance,
    se(mean of f) = s / sqrt(n_w), i.e. ESS = n_w Var(f) / s^2.  f = x for the mean, f = (x - mean)^2 for the variance.
    (An autocorrelation-time estimate from 200 kept steps is biased low at the stretch move's tau of 10 - 20 steps: over 8 seeds it
    gave z-scores 1.6 times these.)"""
    n_t, n_w, d = chain.shape
    f_mean, f_var = chain.mean(axis=0), ((chain - mean) ** 2).mean(axis=0)  # [n_w, d] time averages
    z_mean = (f_mean.mean(axis=0) - mean) / (f_mean.std(axis=0, ddof=1) / np.sqrt(n_w))
    z_var = (f_var.mean(axis=0) - var) / (f_var.std(axis=0, ddof=1) / np.sqrt(n_w))
    return z_mean, z_var
