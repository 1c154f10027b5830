"""Host restatement of the stretch move of the "emcee_smc" sampler (include/asmc.h asmc_stretch_*).

Vectorised numpy Philox4x32-10 (pinned to oracle.philox4x32_10 by tests/test_emcee_smc.py), the split sigma / sigma^-1 (Feistel
network with cycle walking), the propose and accept half-sweeps exactly as specified, and `StretchOracleEngine`, the CPU test
double with the engine methods the sampler calls.  A test helper: the product never imports it.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle_engine import OracleEngine, _np

TAG_DRAW = 0x60000000
TAG_SPLIT = 0xA0000000
ROUNDS = 4
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on broadcast counter words (values < 2^32) and one key; returns the four output words as uint64 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def u01(hi, lo):
    """53-bit uniform in (0, 1) from two words (asmc_pcn_dev.h u01_from_words)."""
    v = ((np.asarray(hi, dtype=np.uint64) << np.uint64(21)) ^ (np.asarray(lo, dtype=np.uint64) >> np.uint64(11)))
    v &= np.uint64((1 << 53) - 1)
    return (v.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def half_bits(n: int) -> int:
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return (bits + 1) // 2


def _network(v, step, shard, seed, hb, inverse):
    mask = np.uint64((1 << hb) - 1)
    L, R = v >> np.uint64(hb), v & mask
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF

    def F(r, a):
        return philox4x32_10(a, step, r, TAG_SPLIT | shard, k0, k1)[0] & mask

    if inverse:
        for r in range(ROUNDS - 1, -1, -1):
            L, R = R ^ F(r, L), L
    else:
        for r in range(ROUNDS):
            L, R = R, L ^ F(r, R)
    return (L << np.uint64(hb)) | R


def _walk(v, n, step, shard, seed, inverse):
    hb = half_bits(n)
    v = _network(np.asarray(v, dtype=np.uint64), step, shard, seed, hb, inverse)
    out = v >= np.uint64(n)
    while out.any():
        v[out] = _network(v[out], step, shard, seed, hb, inverse)
        out = v >= np.uint64(n)
    return v.astype(np.int64)


def sigma(i, n, step, shard, seed):
    """The split's bijection of [0, n): walker i is in half sigma(i) & 1."""
    return _walk(i, n, step, shard, seed, inverse=False)


def sigma_inv(s, n, step, shard, seed):
    return _walk(s, n, step, shard, seed, inverse=True)


def draws(n, half, step, shard, seed):
    """(k, j, u, u_acc) of every slot m of half `half`."""
    s_h, s_o = (n + 1 - half) // 2, (n + half) // 2
    m = np.arange(s_h, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    w = philox4x32_10(m, step, half, TAG_DRAW | shard, k0, k1)
    u, u_acc = u01(w[0], w[1]), u01(w[2], w[3])
    w = philox4x32_10(m, step, 2 | half, TAG_DRAW | shard, k0, k1)
    so = np.uint64(s_o)
    mo = (w[0] * so + ((w[1] * so) >> np.uint64(32))) >> np.uint64(32)
    k = sigma_inv(2 * m + np.uint64(half), n, step, shard, seed)
    j = sigma_inv(2 * mo + np.uint64(1 - half), n, step, shard, seed)
    return k, j, u, u_acc


def propose(x, half, a, seed, shard, step, log_factor=True):
    """(y [|half|, d] in x's dtype, logf, k, j) of half-sweep `half` (asmc_stretch_propose)."""
    n, d = x.shape
    k, j, u, _ = draws(n, half, step, shard, seed)
    t1 = (a - 1.0) * u + 1.0
    zz = t1 * t1 / a
    xj, xk = x[j].astype(np.float64), x[k].astype(np.float64)
    y = (xj - (xj - xk) * zz[:, None]).astype(x.dtype)
    logf = (d - 1) * np.log(zz) if log_factor else np.zeros_like(zz)
    return y, logf, k, j


def log_p_t(ll, lp, lq, beta):
    with np.errstate(all="ignore"):
        r = (1.0 - beta) * np.asarray(lq) + beta * (np.asarray(ll) + np.asarray(lp))
    return np.where(r < np.inf, r, -np.inf)


def accept(x, half, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, logj=None, logj_new=None):
    """asmc_stretch_accept in place on numpy arrays; returns the accept decisions of the slots and their walkers."""
    n = x.shape[0]
    k, _, _, u_acc = draws(n, half, step, shard, seed)
    nlp, olp = log_p_t(ll_new, lp_new, lq_new, beta), log_p_t(ll[k], lp[k], lq[k], beta)
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


class StretchOracleEngine(OracleEngine):
    """OracleEngine plus the stretch-move entry points (stretch_propose / stretch_accept / stretch_counts)."""

    log_factor = True  # False drops (d - 1) log zz: only for checking by hand that the stationarity test catches it

    def __init__(self):
        super().__init__()
        self._stretch_counts = np.zeros(2048, dtype=np.int64)

    def stretch_propose(self, x, half, a, seed, shard, step, t):
        if half == 0:
            self._stretch_counts[t] = 0
        y, logf, _, _ = propose(_np(x), half, a, seed, shard, step, log_factor=self.log_factor)
        return torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(logf)

    def stretch_accept(self, x, half, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, t, logj=None,
                       logj_new=None):
        acc, _ = accept(x.numpy(), half, _np(y), _np(logf), beta, ll.numpy(), lp.numpy(), lq.numpy(), _np(ll_new), _np(lp_new),
                        _np(lq_new), seed, shard, step, None if logj is None else logj.numpy(),
                        None if logj_new is None else _np(logj_new))
        self._stretch_counts[t] += int(acc.sum())

    def stretch_counts(self, n_steps):
        return self._stretch_counts[:n_steps].copy()
