"""Host restatement of the NUTS mutation of the "blackjax_smc" sampler (include/asmc.h asmc_nuts_*).

On top of hmc_ref (the per-particle normal stream, the mixture value and gradient, the leapfrog) and stretch_ref's Philox: the tree of
one transition - doubling, multinomial sampling along the trajectory, the iterative U-turn checkpoints, the divergence check - for any
numpy float type, vectorised over rows with masks.  `Tree` holds the state the split path keeps on the device and its methods are the
split path's launches (begin / select / drift / leaf / merge / finish); `run_transition` runs them around `hmc_ref.target`, which is
what the fused kernel computes.  `np.longdouble` runs of the same code set the tolerances of the device tests; `margin` is the
distance of a row's closest decision from its threshold.  `NutsOracleEngine` is the CPU test double with the engine methods the
sampler calls.  A test helper: the product never imports it.
"""
from __future__ import annotations

import numpy as np
import torch

import hmc_ref as H
import stretch_ref as S
from hmc_ref import HmcOracleEngine
from oracle_engine import _np

TAG_NUTS = 0x60000000
DIVERGENT, TURNING = 1, 2
TWO32 = 4294967296.0
MARGIN_MIN = 1e-9  # rows with a decision closer than this to its threshold are left out of a device comparison


def nuts_words(seed, gid0, n, step, k):
    """The Philox block {gid lo, gid hi, step, 0x60000000 | k} of every row; k a number or one per row."""
    lo, hi = H._gid_words(gid0, n)
    k0, k1 = H._key(seed)
    return S.philox4x32_10(lo, hi, step, np.asarray(k, dtype=np.uint64) | np.uint64(TAG_NUTS), k0, k1)


def nuts_uniform(seed, gid0, n, step, k):
    w = nuts_words(seed, gid0, n, step, k)
    return S.u01(w[0], w[1])


def acceptance_integer(acc_sum, leaves):
    """round(2^32 acc_sum / leaves) per row, 0 without leaves: the integer the device sums."""
    a = np.divide(np.asarray(acc_sum, dtype=np.float64), leaves, out=np.zeros(len(leaves)), where=leaves > 0)
    return np.rint(TWO32 * a).astype(np.int64)


class Tree:
    """State of one transition of n rows (float type `ft`), carried from transition to transition: the proposal slot (zp, gp, dens)
    is the chain's current point."""

    def __init__(self, n, d, max_doublings, eps, minv, beta, threshold, ft=np.float64):
        self.n, self.d, self.K, self.ft = n, d, int(max_doublings), ft
        self.eps, self.beta, self.thr = float(eps), float(beta), float(threshold)
        self.minv = None if minv is None else np.asarray(minv, dtype=ft)
        z = lambda *s: np.zeros(s, dtype=ft)
        self.zl, self.pl, self.gl, self.zr, self.pr, self.gr = (z(n, d) for _ in range(6))
        self.zc, self.pc, self.gc = z(n, d), z(n, d), z(n, d)
        self.zs, self.gs, self.zp, self.gp = z(n, d), z(n, d), z(n, d), z(n, d)
        self.psum, self.spsum = z(n, d), z(n, d)
        self.ck_p, self.ck_s = z(self.K, n, d), z(self.K, n, d)
        self.dens_p, self.dens_s = z(3, n), z(3, n)
        self.E0, self.tree_lw, self.sub_lw, self.accs = z(n), z(n), z(n), z(n)
        i = lambda: np.zeros(n, dtype=np.int64)
        self.depth, self.steps, self.leaves, self.flags, self.pos, self.spos, self.nl, self.nr, self.v = (i() for _ in range(9))
        self.dirw = np.zeros(n, dtype=np.uint64)
        self.building = np.zeros(n, dtype=bool)
        self.alive = np.zeros(n, dtype=bool)  # rows whose current sub-tree is still growing
        self.margin = np.full(n, np.inf)

    # ---- helpers ----
    def _im(self, a):
        return a if self.minv is None else self.minv * a

    def _near(self, rows, dist):
        d = np.asarray(dist, dtype=np.float64)
        d = np.where(np.isfinite(d), d, np.inf)
        self.margin[rows] = np.minimum(self.margin[rows], d)

    def _turning(self, rows, a, b, s):
        """turning(a, b, s) = (a^T M^-1 s <= 0) or (b^T M^-1 s <= 0) on the rows given; records the margins."""
        ms = self._im(s)
        with np.errstate(all="ignore"):
            da, db = (a * ms).sum(-1), (b * ms).sum(-1)
            ns = np.sqrt((s * s).sum(-1))
            self._near(rows, np.abs(da) / (np.sqrt((a * a).sum(-1)) * ns))
            self._near(rows, np.abs(db) / (np.sqrt((b * b).sum(-1)) * ns))
        return (da <= 0) | (db <= 0)

    def set_point(self, z, g, ll, lp, lq):
        self.zp[:], self.gp[:] = np.asarray(z, dtype=self.ft), np.asarray(g, dtype=self.ft)
        self.dens_p[0], self.dens_p[1], self.dens_p[2] = (np.asarray(v, dtype=self.ft) for v in (ll, lp, lq))

    # ---- the launches ----
    def begin(self, seed, gid0, step):
        ft, n = self.ft, self.n
        self.seed, self.gid0, self.step = seed, gid0, step
        p0 = H.momenta(seed, gid0, n, step, self.d, None if self.minv is None else self.minv.astype(np.float64)).astype(ft)
        lpt = H.log_p_t(self.dens_p[0], self.dens_p[1], self.dens_p[2], self.beta)
        with np.errstate(all="ignore"):
            self.E0[:] = H.kinetic(p0, self.minv) - lpt
        self.building[:] = np.isfinite(lpt.astype(np.float64))
        self.alive[:] = False
        for zz, pp, gg in ((self.zl, self.pl, self.gl), (self.zr, self.pr, self.gr), (self.zc, self.pc, self.gc)):
            zz[:], pp[:], gg[:] = self.zp, p0, self.gp
        self.psum[:] = p0
        self.tree_lw[:], self.accs[:] = 0, 0
        for v in (self.depth, self.steps, self.leaves, self.flags, self.pos, self.nl, self.nr):
            v[:] = 0
        self.dirw[:] = nuts_words(seed, gid0, n, step, 0)[0]

    def select(self):
        b = self.building
        self.alive[:] = b
        fwd = ((self.dirw >> self.depth.astype(np.uint64)) & np.uint64(1)) != 0
        self.v[:] = np.where(fwd, 1, -1)
        r, l = b & fwd, b & ~fwd
        for c, e_r, e_l in ((self.zc, self.zr, self.zl), (self.pc, self.pr, self.pl), (self.gc, self.gr, self.gl)):
            c[r], c[l] = e_r[r], e_l[l]
        self.sub_lw[b] = -np.inf
        self.spsum[b] = 0

    def drift(self):
        a, ft = self.alive, self.ft
        h = (self.v[a].astype(ft) * ft(self.eps))[:, None]
        with np.errstate(all="ignore"):
            p = self.pc[a] + ft(0.5) * h * self.gc[a]
            self.pc[a] = p
            self.zc[a] = self.zc[a] + h * self._im(p)

    def leaf(self, i, g_new, ll, lp, lq):
        """Second half kick, energy and divergence check, leaf sampling, checkpoint store or U-turn checks of leaf `i` (0-based in
        the doubling) for the rows whose sub-tree is alive; (g_new, ll, lp, lq) at zc."""
        ft, a = self.ft, self.alive.copy()
        if not a.any():
            return
        idx = np.flatnonzero(a)
        h = (self.v[idx].astype(ft) * ft(self.eps))[:, None]
        with np.errstate(all="ignore"):
            p = self.pc[idx] + ft(0.5) * h * np.asarray(g_new, dtype=ft)[idx]
            E = H.kinetic(p, self.minv) - H.log_p_t(np.asarray(ll, dtype=ft)[idx], np.asarray(lp, dtype=ft)[idx], np.asarray(lq, dtype=ft)[idx],
                                                    self.beta)
            delta = E - self.E0[idx]
            self._near(idx, np.abs(delta - ft(self.thr)))
            ok = delta <= ft(self.thr)
        u = nuts_uniform(self.seed, self.gid0 + 0, self.n, self.step, 16 + self.steps)[idx]
        self.pc[idx], self.gc[idx] = p, np.asarray(g_new, dtype=ft)[idx]
        self.steps[idx] += 1
        div = idx[~ok]
        self.flags[div] |= DIVERGENT
        idx, p, delta, u = idx[ok], p[ok], delta[ok], u[ok]
        with np.errstate(all="ignore"):
            lw = -delta
            self.accs[idx] += np.minimum(ft(1), np.exp(lw))
            self.leaves[idx] += 1
            new = np.logaddexp(self.sub_lw[idx], lw)
            pacc = np.exp(lw - new)
        if i == 0:
            take = np.ones(len(idx), dtype=bool)
        else:
            self._near(idx, np.abs(u - pacc.astype(np.float64)))
            take = u < pacc
        t = idx[take]
        self.zs[t], self.gs[t] = self.zc[t], self.gc[t]
        for k, v in enumerate((ll, lp, lq)):
            self.dens_s[k][t] = np.asarray(v, dtype=ft)[t]
        side = np.where(self.v[t] > 0, self.nr[t], self.nl[t])
        self.spos[t] = self.v[t] * (side + i + 1)
        self.sub_lw[idx] = new
        self.spsum[idx] += p
        top = bin(i >> 1).count("1")
        turn = np.zeros(len(idx), dtype=bool)
        if i % 2 == 0:
            self.ck_p[top, idx], self.ck_s[top, idx] = p, self.spsum[idx]
        else:
            ones = (i ^ (i + 1)).bit_length() - 1  # trailing one bits of i
            for k in range(top, top - ones, -1):
                cp, cs = self.ck_p[k, idx], self.ck_s[k, idx]
                turn |= self._turning(idx, cp, p, self.spsum[idx] - cs + cp)
        self.flags[idx[turn]] |= TURNING
        ended = np.concatenate([div, idx[turn]])
        self.alive[ended] = False
        self.building[ended] = False
        self.zc[ended] = self.zp[ended]  # (a finite point for the gradient launches that still see the row)

    def merge(self, j):
        """Sub-tree `j` is complete on the alive rows.  Returns the number of rows still building."""
        ft = self.ft
        idx = np.flatnonzero(self.alive)
        if len(idx):
            fwd = self.v[idx] > 0
            r, l = idx[fwd], idx[~fwd]
            self.zr[r], self.pr[r], self.gr[r] = self.zc[r], self.pc[r], self.gc[r]
            self.zl[l], self.pl[l], self.gl[l] = self.zc[l], self.pc[l], self.gc[l]
            self.nr[r] += 1 << j
            self.nl[l] += 1 << j
            u = nuts_uniform(self.seed, self.gid0, self.n, self.step, 1 + j)[idx]
            with np.errstate(all="ignore"):
                pacc = np.exp(np.minimum(ft(0), self.sub_lw[idx] - self.tree_lw[idx]))
                self._near(idx, np.abs(u - pacc.astype(np.float64)))
                t = idx[u < pacc]
                self.zp[t], self.gp[t], self.pos[t] = self.zs[t], self.gs[t], self.spos[t]
                self.dens_p[:, t] = self.dens_s[:, t]
                self.tree_lw[idx] = np.logaddexp(self.tree_lw[idx], self.sub_lw[idx])
            self.psum[idx] += self.spsum[idx]
            self.depth[idx] += 1
            turn = self._turning(idx, self.pl[idx], self.pr[idx], self.psum[idx])
            self.flags[idx[turn]] |= TURNING
            self.building[idx[turn]] = False
            self.building[idx[self.depth[idx] >= self.K]] = False
            self.zc[idx] = self.zp[idx]
        self.alive[:] = False
        return int(self.building.sum())

    def info(self):
        return np.stack([self.depth, self.steps, self.flags, self.pos], axis=1).astype(np.int32)

    def stats(self):
        """(moved rows, leapfrog steps, divergent rows, integer acceptance sum) of the transition."""
        q = acceptance_integer(self.accs, self.leaves)
        return np.array([int((self.pos != 0).sum()), int(self.steps.sum()), int(((self.flags & DIVERGENT) != 0).sum()), int(q.sum())],
                        dtype=np.int64)


def run_transition(tree, target_fn, seed, gid0, step):
    """One transition of `tree` from its proposal slot: target_fn(z) -> (ll, lp, lq, grad) at the rows z."""
    tree.begin(seed, gid0, step)
    for j in range(tree.K):
        if not tree.building.any():
            break
        tree.select()
        for i in range(1 << j):
            if not tree.alive.any():
                break
            tree.drift()
            ll, lp, lq, g = target_fn(tree.zc)
            tree.leaf(i, g, ll, lp, lq)
        tree.merge(j)


def nuts_mix(x, ll, lp, lq, beta, mixes, minv, eps, seed, gid0, step0, n_steps, max_doublings=10, threshold=1000.0, ft=np.float64):
    """asmc_nuts_mix on fp64 numpy arrays, in place: transitions step0 .. step0 + n_steps - 1 in the float type `ft`.  A dict:
    stats [n_steps, 4], info [n, 4] of the last transition, margin [n] (the smallest over the transitions), per transition the
    rows' info, acceptance integers and their distance from a rounding boundary, and `x` in `ft`."""
    n, d = x.shape
    tree = Tree(n, d, max_doublings, eps, minv, beta, threshold, ft)
    tgt = lambda z: H.target(mixes, beta, z)
    l0, p0, q0, g0 = tgt(x.astype(ft))
    tree.set_point(x.astype(ft), g0, l0, p0, q0)
    stats = np.zeros((n_steps, 4), dtype=np.int64)
    moved = np.zeros(n, dtype=bool)
    infos, accq, accfrac = [], [], []
    for s in range(n_steps):
        run_transition(tree, tgt, seed, gid0, step0 + s)
        stats[s] = tree.stats()
        moved |= tree.pos != 0
        infos.append(tree.info())
        a = np.divide(tree.accs.astype(np.float64), tree.leaves, out=np.zeros(n), where=tree.leaves > 0) * TWO32
        accq.append(np.rint(a).astype(np.int64))
        accfrac.append(np.abs(a - np.floor(a) - 0.5))
    x[moved] = tree.zp[moved].astype(np.float64)
    ll[moved], lp[moved], lq[moved] = (tree.dens_p[k][moved].astype(np.float64) for k in range(3))
    return dict(stats=stats, info=tree.info() if n_steps else np.zeros((n, 4), dtype=np.int32), margin=tree.margin, infos=infos,
                accq=accq, accfrac=accfrac, x=tree.zp.copy(), moved=moved)


def nuts_tolerance(mixes, beta, x, eps, minv, seed, gid0, step0, n_steps=1, max_doublings=10, threshold=1000.0):
    """The fp64 run of the restatement and what a device may differ from it by - hmc_ref.dh_tolerance's scheme for the end points:
    8 x the largest distance between the fp64 and the long-double run of this very case plus 64 ulp of the row's largest
    coordinate.  Rows whose closest decision lies within MARGIN_MIN of its threshold (in either run), or whose diagnostics differ
    between the two runs, are left out: (r64, rld, tol_x [n], keep [n] bool, gap_x)."""
    out = []
    for ft in (np.float64, np.longdouble):
        xx = x.copy()
        ll, lp, lq = (np.zeros(len(x)) for _ in range(3))
        r = nuts_mix(xx, ll, lp, lq, beta, mixes, minv, eps, seed, gid0, step0, n_steps, max_doublings, threshold, ft)
        r["x64"], r["dens"] = xx, (ll, lp, lq)
        out.append(r)
    r64, rld = out
    same = np.ones(len(x), dtype=bool)
    for a, b in zip(r64["infos"], rld["infos"]):
        same &= (a == b).all(axis=1)
    keep = same & (r64["margin"] >= MARGIN_MIN) & (rld["margin"] >= MARGIN_MIN)
    diff = np.abs(r64["x"] - rld["x"]).astype(np.float64)[keep]
    gap_x = float(diff.max()) if diff.size else 0.0
    tol_x = 8.0 * gap_x + 64.0 * np.spacing(np.abs(r64["x64"]).max(axis=1))
    return r64, rld, tol_x, keep, gap_x


# ---- the cases of the fused kernel's comparison (tests/test_gpu_nuts.py; tests/test_nuts.py checks that the restatement leaves out
# none of their rows) -------------------------------------------------------------------------------------------------------------
STEP_SIZES = (0.5, 0.35, 0.2, 0.12)  # depths 2 .. 5 on these targets


def fused_cases():
    """(n, d, C, diagonal mass, beta, step_size): n in {7, 257, 4097} x one d per instantiation of k_nuts_mix (d = 128: n <= 257, the
    long-double run), 1 and 3 components, unit and diagonal mass, beta 0.3 and 1.0 and the four step sizes spread over the grid."""
    out = []
    for a, n in enumerate((7, 257, 4097)):
        for b, d in enumerate((1, 7, 13, 32, 33, 128)):
            k = 6 * a + b
            out.append((min(n, 257 if a < 2 else 129) if d == 128 else n, d, (1, 3)[(a + b) % 2], bool((k // 2) % 2), (0.3, 1.0)[(k // 3) % 2],
                        STEP_SIZES[(a + b + b // 4) % 4]))
    return out


def mix_case(n, d, C, seed):
    """(mixes, x [n, d], diagonal of M^-1): a C-component likelihood, a Gaussian prior and a Gaussian proposal."""
    g = np.random.default_rng(seed)
    mixes = [H.random_mixture(g, C, d, spread=1.0), H.random_mixture(g, 1, d, spread=0.3), H.random_mixture(g, 1, d, spread=0.3)]
    return mixes, g.normal(size=(n, d)), g.uniform(0.5, 2.0, size=d)


CASE_KEY = (0x5EED5EED5EED, (1 << 32) - 2, 6)  # seed, gid0 (the ids cross the 32-bit word), step


def fused_case_reference(n, d, C, diag, beta, eps, n_steps=1):
    """(mixes, x, mass, nuts_tolerance(...)) of one case."""
    mixes, x, minv = mix_case(n, d, C, 31 * n + d + C)
    mass = minv if diag else None
    return mixes, x, mass, nuts_tolerance(mixes, beta, x, eps, mass, *CASE_KEY, n_steps=n_steps)


def divergent_case():
    """A case with both endings: 257 rows, d = 7, three components, step_size 1.2 and divergence_threshold 2 (119 divergent and 138
    turning rows in the restatement): (mixes, x, beta, step_size, threshold)."""
    mixes, x, _ = mix_case(257, 7, 3, 15)
    return mixes, x, 0.6, 1.2, 2.0


class NutsOracleEngine(HmcOracleEngine):
    """HmcOracleEngine plus the NUTS entry points of HipEngine."""

    def __init__(self):
        super().__init__()
        self._nuts_stats = np.zeros((2048, 4), dtype=np.int64)

    def nuts_mix(self, x, ll, lp, lq, beta, t_ll, t_lp, t_lq, minv, step_size, max_doublings, threshold, seed, gid0, step0, n_steps,
                 t0=0, want_info=False, max_blocks=0):
        assert x.dtype == torch.float64
        r = nuts_mix(x.numpy(), ll.numpy(), lp.numpy(), lq.numpy(), beta, [self._mix(m) for m in (t_ll, t_lp, t_lq)],
                     None if minv is None else _np(minv), step_size, seed, gid0, step0, n_steps, max_doublings, threshold)
        self._nuts_stats[t0:t0 + n_steps] = r["stats"]
        return torch.from_numpy(r["info"]) if want_info else None

    def nuts_stats(self, n_steps):
        return self._nuts_stats[:n_steps].copy()

    # the split path: the state is a Tree, the tensors the sampler touches are views of its arrays
    def nuts_state(self, n, d, max_doublings, minv, step_size, beta, threshold):
        st = Tree(n, d, max_doublings, step_size, None if minv is None else _np(minv), beta, threshold)
        st.z = torch.from_numpy(st.zc)
        return st

    def nuts_set_point(self, st, z, g, ll, lp, lq):
        st.set_point(_np(z), _np(g), _np(ll), _np(lp), _np(lq))

    def nuts_begin(self, st, seed, gid0, step):
        st.begin(seed, gid0, step)

    def nuts_select(self, st):
        st.select()

    def nuts_drift(self, st):
        st.drift()

    def nuts_leaf(self, st, i, g, ll, lp, lq):
        st.leaf(i, _np(g), _np(ll).astype(np.float64), _np(lp).astype(np.float64), _np(lq).astype(np.float64))

    def nuts_merge(self, st, j):
        return st.merge(j)

    def nuts_finish(self, st, x, ll, lp, lq, t, want_info=False):
        m = st.pos != 0
        xn = x.numpy()
        xn[m] = st.zp[m].astype(xn.dtype)
        for dst, src in zip((ll, lp, lq), st.dens_p):
            dst.numpy()[m] = src[m]
        self._nuts_stats[t] = st.stats()
        return torch.from_numpy(st.info()) if want_info else None
