"""Host restatement of the DE and snooker moves of the "emcee_smc" / "emcee" samplers (include/asmc.h asmc_ensemble_*, DESIGN.md
§3.26), on top of stretch_ref's Philox, split and accept.

`groups` (the S-way split), `draws` (every per-slot draw), `propose_de`, `propose_snooker` (written for any numpy float type: an
`np.longdouble` run sets the tolerance of the device test, the fp64 run follows the specified order of the row sums), `accept`, and
`EnsembleOracleEngine`, the CPU test double with the two engine entry points.  The normal of the DE move is libm's Box-Muller on the
specified 32-bit uniforms: the device's table-driven generator is within 1e-16 of it, so proposals of the DE move
are restated to that error, not to the bit.  A test helper: the product never imports it.
"""
from __future__ import annotations

import numpy as np
import torch

import stretch_ref as S
from oracle_engine import _np

TAG_DRAW = 0x70000000
PERMS = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]])
_TWO_M32 = 1.0 / 4294967296.0


def group_size(n: int, nsplits: int, g: int) -> int:
    return (n - g + nsplits - 1) // nsplits


def groups(n, nsplits, step, shard, seed):
    """The walkers of every group, in slot order: slot m of group g is sigma^-1(S m + g)."""
    return [S.sigma_inv(nsplits * np.arange(group_size(n, nsplits, g), dtype=np.uint64) + np.uint64(g), n, step, shard, seed)
            for g in range(nsplits)]


def _index(hi, lo, K):
    """floor(((hi << 32) | lo) K / 2^64), exact (K < 2^32)."""
    K = np.uint64(K)
    return (hi * K + ((lo * K) >> np.uint64(32))) >> np.uint64(32)


def _blocks(n_slots, nsplits, group, step, shard, seed, n_blocks):
    m = np.arange(n_slots, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return [S.philox4x32_10(m, step, (b << 2) | group, TAG_DRAW | shard, k0, k1) for b in range(n_blocks)]


def draws(n, move, group, step, shard, seed):
    """Every draw of the slots of `group`: a dict with k, u_acc and, for "de", j1, j2, xi (and its Box-Muller radius rad); for
    "snooker", c [slots, 3] (one walker of each other group, ascending), r, and z, z1, z2 (the r-th permutation of c)."""
    nsplits = 2 if move == "de" else 4
    n_slots = group_size(n, nsplits, group)
    m = np.arange(n_slots, dtype=np.uint64)
    k = S.sigma_inv(np.uint64(nsplits) * m + np.uint64(group), n, step, shard, seed)
    if move == "de":
        w0, w1 = _blocks(n_slots, nsplits, group, step, shard, seed, 2)
        s_o = (n + group) // 2
        m1 = _index(w0[0], w0[1], s_o)
        m2 = _index(w1[0], w1[1], s_o - 1)
        m2 = m2 + (m2 >= m1).astype(np.uint64)
        other = np.uint64(1 - group)
        u = (w1[2].astype(np.float64) + 0.5) * _TWO_M32
        t = (w1[3].astype(np.float64) + 0.5) * _TWO_M32
        rad = np.sqrt(-2.0 * np.log(u))
        xi = rad * np.cos(2.0 * np.pi * t)
        return dict(k=k, u_acc=S.u01(w0[2], w0[3]), xi=xi, rad=rad, j1=S.sigma_inv(np.uint64(2) * m1 + other, n, step, shard, seed),
                    j2=S.sigma_inv(np.uint64(2) * m2 + other, n, step, shard, seed))
    w0, w1, w2 = _blocks(n_slots, nsplits, group, step, shard, seed, 3)
    others = [o for o in range(4) if o != group]
    words = ((w0[0], w0[1]), (w1[0], w1[1]), (w1[2], w1[3]))
    c = np.stack([S.sigma_inv(np.uint64(4) * _index(hi, lo, group_size(n, 4, o)) + np.uint64(o), n, step, shard, seed)
                  for (hi, lo), o in zip(words, others)], axis=1)
    r = ((w2[0] * np.uint64(6)) >> np.uint64(32)).astype(np.int64)
    p = PERMS[r]
    rows = np.arange(n_slots)
    return dict(k=k, u_acc=S.u01(w0[2], w0[3]), c=c, r=r, z=c[rows, p[:, 0]], z1=c[rows, p[:, 1]], z2=c[rows, p[:, 2]])


def propose_de(x, group, g0, sigma, seed, shard, step):
    """(y [|group|, d] in x's dtype, logf = 0, draws) of the DE move (asmc_ensemble_propose, ASMC_MOVE_DE)."""
    dr = draws(x.shape[0], "de", group, step, shard, seed)
    gamma = g0 * (1.0 + sigma * dr["xi"])
    xk, x1, x2 = (x[dr[name]].astype(np.float64) for name in ("k", "j1", "j2"))
    y = (xk + gamma[:, None] * (x2 - x1)).astype(x.dtype)
    return y, np.zeros(len(gamma)), dr


def _row_sum(v, ft):
    """Sum of the columns of v [rows, d] in the order of the kernel: 2^lg lanes per row, lane l adds its coordinates l, l + 2^lg,
    ... in ascending order, then the butterfly v <- v + v[lane ^ o], o = 2^(lg - 1) .. 1."""
    rows, d = v.shape
    if ft is not np.float64:  # the wider run is the yardstick, not a restatement of the order
        return v.sum(axis=1)
    lg = 0
    while (1 << lg) < d and lg < 6:
        lg += 1
    tpr = 1 << lg
    trips = -(-d // tpr)
    parts = np.zeros((rows, trips * tpr), dtype=ft)  # (a lane without a coordinate in the last trip adds a zero: the same bits)
    parts[:, :d] = v
    parts = parts.reshape(rows, trips, tpr)
    lanes = parts[:, 0, :]
    for j in range(1, trips):
        lanes = lanes + parts[:, j, :]
    o = tpr >> 1
    while o:
        lanes = lanes + lanes[:, np.arange(tpr) ^ o]
        o >>= 1
    return lanes[:, 0]


def propose_snooker(x, group, gammas, seed, shard, step, log_factor=True, ft=np.float64):
    """(y [|group|, d] in x's dtype - or unrounded in `ft` when ft is not float64 -, logf, draws) of the snooker move
    (asmc_ensemble_propose, ASMC_MOVE_SNOOKER)."""
    n, d = x.shape
    dr = draws(n, "snooker", group, step, shard, seed)
    xk, xz, x1, x2 = (x[dr[name]].astype(ft) for name in ("k", "z", "z1", "z2"))
    delta = xk - xz
    with np.errstate(all="ignore"):
        ss, dp = _row_sum(delta * delta, ft), _row_sum(delta * (x1 - x2), ft)
        r0 = np.sqrt(ss)
        ok = (r0 > 0) & (r0 < np.inf)
        gp = ft(gammas) * (dp / r0)
        y = np.where(ok[:, None], xk + gp[:, None] * (delta / r0[:, None]), xk)
        r1 = np.abs(r0 + gp)
        good = ok & (r1 > 0) & (r1 < np.inf)
        logf = np.where(good, ft(d - 1) * (np.log(r1) - np.log(r0)), -np.inf)
    if not log_factor:
        logf = np.where(good, 0.0, -np.inf)
    dr.update(r0=r0, gp=gp, rows=(xk, xz, x1, x2))
    return (y.astype(x.dtype) if ft is np.float64 else y), logf, dr


def accept(x, nsplits, group, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, logj=None, logj_new=None,
           dr=None):
    """asmc_ensemble_accept in place on numpy arrays (stretch_ref.accept on the S-way split with this stream's accept variate);
    returns the accept decisions of the slots and their walkers.  `dr`: the sweep's `draws`, where the caller has them."""
    dr = dr or draws(x.shape[0], "de" if nsplits == 2 else "snooker", group, step, shard, seed)
    k, u_acc = dr["k"], dr["u_acc"]
    nlp, olp = S.log_p_t(ll_new, lp_new, lq_new, beta), S.log_p_t(ll[k], lp[k], lq[k], beta)
    with np.errstate(all="ignore"):
        if logj is not None:
            nlp, olp = nlp + logj_new, olp + logj[k]
            nlp, olp = np.where(nlp < np.inf, nlp, -np.inf), np.where(olp < np.inf, olp, -np.inf)
        acc = (logf + nlp) - olp > np.log(u_acc)
    ka = k[acc]
    x[ka] = y[acc]
    ll[ka], lp[ka], lq[ka] = ll_new[acc], lp_new[acc], lq_new[acc]
    if logj is not None:
        logj[ka] = logj_new[acc]
    return acc, k


class EnsembleOracleEngine(S.StretchOracleEngine):
    """StretchOracleEngine plus the DE / snooker entry points (ensemble_propose / ensemble_accept)."""

    snooker_log_factor = True  # False drops the snooker's Jacobian factor: only for checking by hand that the stationarity test catches it

    def ensemble_propose(self, x, move, nsplits, group, p0, p1, seed, shard, step, t):
        assert nsplits == (2 if move == "de" else 4) and x.shape[0] >= 4
        if group == 0:
            self._stretch_counts[t] = 0
        if move == "de":
            y, logf, _ = propose_de(_np(x), group, p0, p1, seed, shard, step)
        else:
            y, logf, _ = propose_snooker(_np(x), group, p0, seed, shard, step, log_factor=self.snooker_log_factor)
        return torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(logf))

    def ensemble_accept(self, x, nsplits, group, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, t, logj=None,
                        logj_new=None):
        acc, _ = accept(x.numpy(), nsplits, group, _np(y), _np(logf), beta, ll.numpy(), lp.numpy(), lq.numpy(), _np(ll_new),
                        _np(lp_new), _np(lq_new), seed, shard, step, None if logj is None else logj.numpy(),
                        None if logj_new is None else _np(logj_new))
        self._stretch_counts[t] += int(acc.sum())
