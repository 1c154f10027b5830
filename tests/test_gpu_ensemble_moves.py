"""The DE and snooker kernels of the "emcee_smc" / "emcee" samplers on the HIP engine (csrc/asmc_ensemble.hip; include/asmc.h
asmc_ensemble_*).

* k_de_propose / k_snooker_propose / k_ensemble_accept against tests/ensemble_ref.py: one step, every group-sweep, every row; the
  accept decisions, rows, carried densities and counter restated from the device's own proposals must match exactly;
* degenerate ensembles (duplicated rows, a slot whose proposal falls on z): no NaN, logf = -inf where specified, rejected;
* later sweeps read what earlier sweeps of the step accepted; same seed, same bits; the stretch entry points keep their bits;
* end to end: log Z at d = 8 over eight seeds with emcee's recommended mixture, with the stretch test's z-score bound.
"""
import math

import numpy as np
import pytest
import torch

import ensemble_ref as E
import stretch_ref as S
from test_gpu_emcee_smc import _densities

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
XI_ERR = 1e-16  # the device's table-driven Box-Muller against libm on the same uniforms, absolute
G0, SIGMA, GAMMAS = 0.42, 0.3, 1.7  # sigma far above emcee's 1e-5 default, so that the normal xi matters in the comparison


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


def _de_bound(x, y_ref, dr, npdt):
    """|y_dev - y_ref| per coordinate when only xi differs, every rounding counted once for each side (half an ulp each, so one
    spacing per operation).  xi_dev = xi_ref + e with |e| <= XI_ERR + r 2 ulp(2 pi) + 3 ulp(r): the documented error of the generator
    plus this restatement's own in xi_ref = r cos(fl(fl(2 pi) t)), r = sqrt(-2 ln u) - the angle carries the rounding of 2 pi and of
    the product, an absolute ulp(2 pi) each at most, which the cosine passes on at slope <= 1 and r scales, whatever the size of
    xi itself; r, the cosine and their product add an ulp of r each.
    gamma = fl(g0 fl(1 + fl(sigma xi))) then differs by |g0| (|sigma| |e| + ulp(sigma xi) + ulp(1 + sigma xi)) + ulp(gamma), the
    product gamma (x_j2 - x_j1) by that times |x_j2 - x_j1| plus its ulp, the sum by the ulp of y - each ulp taken at the value
    plus the slack before it, since the two sides may lie on either side of a power of two - and one rounding to x_dtype where that
    is narrower."""
    xi = dr["xi"]
    s1 = SIGMA * xi
    s2 = 1.0 + s1
    gamma = G0 * s2
    dxi = XI_ERR + dr["rad"] * 2.0 * np.spacing(2.0 * np.pi) + 3.0 * np.spacing(dr["rad"])
    dgamma = abs(G0) * (abs(SIGMA) * dxi + np.spacing(np.abs(s1) + abs(SIGMA) * dxi) + np.spacing(np.abs(s2) + 1e-15))
    dgamma = dgamma + np.spacing(np.abs(gamma) + dgamma)
    diff = np.abs(x[dr["j2"]].astype(np.float64) - x[dr["j1"]].astype(np.float64))
    dprod = dgamma[:, None] * diff
    dprod = dprod + np.spacing(np.abs(gamma)[:, None] * diff + dprod)
    tol = dprod + np.spacing(np.abs(y_ref.astype(np.float64)) + dprod)
    if npdt is np.float32:
        tol = tol + np.spacing(np.abs(y_ref) + tol.astype(np.float32)).astype(np.float64)
    return tol


def _check_de(x, group, y_h, logf_h, seed, shard, step, npdt):
    y_ref, logf_ref, dr = E.propose_de(x, group, G0, SIGMA, seed, shard, step)
    assert y_h.shape == y_ref.shape and np.array_equal(logf_h, logf_ref)  # logf = 0
    err = np.abs(y_h.astype(np.float64) - y_ref.astype(np.float64))
    tol = _de_bound(x, y_ref, dr, npdt)
    # a wrong partner index moves y by the distance between two walkers, orders of magnitude beyond this bound
    assert np.all(err <= tol), f"group {group}: DE proposals differ, worst {np.max(err / tol):.3g} of the bound"
    return dr


def _check_snooker(x, group, y_h, logf_h, seed, shard, step, npdt):
    """Against the np.longdouble restatement: y within (d + 4) 2^-53 (|x_k| + |gammas| |e|.|z1 - z2|) per coordinate plus one
    rounding to x_dtype; logf within (d - 1) times [that bound relative to each logarithm's argument + 1 ulp of each device log]."""
    n, d = x.shape
    y_ref, logf_ref, dr = E.propose_snooker(x, group, GAMMAS, seed, shard, step, ft=np.longdouble)
    xk, xz, x1, x2 = dr["rows"]
    r0, gp = dr["r0"], dr["gp"]
    ok = r0 > 0
    assert ok.all()
    absdot = (np.abs(xk - xz) / r0[:, None] * np.abs(x1 - x2)).sum(1)
    rel = (d + 4) * U
    tol = rel * (np.abs(xk) + abs(GAMMAS) * absdot[:, None]) + np.spacing(np.abs(y_ref).astype(npdt)).astype(np.longdouble)
    err = np.abs(y_h.astype(np.longdouble) - y_ref)
    assert np.all(err <= tol), f"group {group}: snooker proposals differ, worst {float(np.max(err / tol)):.3g} of the bound"
    r1 = np.abs(r0 + gp)
    log1, log0 = np.log(r1).astype(np.float64), np.log(r0).astype(np.float64)
    ltol = (d - 1) * (rel * ((r0 + abs(GAMMAS) * absdot) / r1 + 1.0).astype(np.float64) + np.spacing(np.abs(log1))
                      + np.spacing(np.abs(log0))) + np.spacing(np.abs(logf_ref.astype(np.float64)))
    lerr = np.abs(logf_h - logf_ref.astype(np.float64))
    assert np.all(lerr <= ltol), f"group {group}: snooker logf differs, worst {float(np.max(lerr / np.maximum(ltol, 1e-300))):.3g} of the bound"
    return dr


CASES = ([(mv, n, d, dt) for mv in ("de", "snooker") for n in (4, 7, 4097) for d in (2, 7, 33, 128) for dt in ("f64", "f32")]
         + [(mv, 1_000_003, 32, "f64") for mv in ("de", "snooker")])


@pytest.mark.parametrize("move,n,d,dt", CASES, ids=[f"{mv}-n{n}-d{d}-{dt}" for mv, n, d, dt in CASES])
def test_kernels_against_the_restatement(eng, move, n, d, dt):
    """One step, all group-sweeps, every row.  The partner indices and the snooker's permutation are exact (they decide which rows
    enter y: see _check_de); the accept is restated from the device's y and logf, so decisions, rows, densities and the counter
    must agree exactly - with tests/test_gpu_emcee_smc.py's -inf / NaN density holes and, at d = 7, a log-Jacobian."""
    tdt, npdt = (torch.float64, np.float64) if dt == "f64" else (torch.float32, np.float32)
    g = np.random.default_rng(n + d)
    x = g.normal(size=(n, d)).astype(npdt)
    ll, lp, lq = _densities(x.astype(np.float64))
    logj = g.normal(size=n) if d == 7 else None
    xd = torch.from_numpy(x).to(eng.device)
    lld, lpd, lqd = (torch.from_numpy(a.copy()).to(eng.device) for a in (ll, lp, lq))
    ljd = None if logj is None else torch.from_numpy(logj.copy()).to(eng.device)
    seed, shard, step, beta = 0x0123456789ABCDEF, (3 if n == 4097 else 0), 11, 0.6
    nsplits, p0, p1 = (2, G0, SIGMA) if move == "de" else (4, GAMMAS, 0.0)
    total, x_before, stale_seen = 0, x.copy(), False
    for grp in range(nsplits):
        y, logf = eng.ensemble_propose(xd, move, nsplits, grp, p0, p1, seed, shard, step, 0)
        y_h, logf_h = y.cpu().numpy(), logf.cpu().numpy()
        assert y_h.dtype == npdt and y_h.shape == (E.group_size(n, nsplits, grp), d)
        check = _check_de if move == "de" else _check_snooker
        dr = check(x, grp, y_h, logf_h, seed, shard, step, npdt)
        if grp == 1 and 8 < n < 100_000:  # later sweeps read the rows that earlier sweeps of the step accepted
            moved = np.any(x != x_before, axis=1)
            partners = np.concatenate([dr[name] for name in (("j1", "j2") if move == "de" else ("z", "z1", "z2"))])
            assert moved[partners].any()
            def restated(state):
                return (E.propose_de(state, grp, p0, p1, seed, shard, step) if move == "de"
                        else E.propose_snooker(state, grp, p0, seed, shard, step))[0].astype(np.float64)

            # the proposals from the step's first state are far from the ones the device agrees with (checked above)
            assert np.max(np.abs(restated(x_before) - restated(x))) > 1e-3
            stale_seen = True
        lln, lpn, lqn = _densities(y_h.astype(np.float64))
        ljn = None if logj is None else g.normal(size=len(y_h))
        new = [torch.from_numpy(v.copy()).to(eng.device) for v in (lln, lpn, lqn)]
        eng.ensemble_accept(xd, nsplits, grp, y, logf, beta, lld, lpd, lqd, *new, seed, shard, step, 0, logj=ljd,
                            logj_new=None if ljn is None else torch.from_numpy(ljn).to(eng.device))
        acc, kk = E.accept(x, nsplits, grp, y_h, logf_h, beta, ll, lp, lq, lln, lpn, lqn, seed, shard, step, logj=logj, logj_new=ljn,
                           dr=dr)
        total += int(acc.sum())
        assert np.array_equal(xd.cpu().numpy(), x), f"group {grp}: state differs"
        for dev, ref in ((lld, ll), (lpd, lp), (lqd, lq)) + (((ljd, logj),) if logj is not None else ()):
            np.testing.assert_array_equal(dev.cpu().numpy(), ref)
    assert int(eng.stretch_counts(1)[0]) == total
    assert 0 <= total <= n and (total > 0 or n < 8) and (stale_seen or not 8 < n < 100_000)


def test_small_ensembles_and_bad_arguments_are_refused(eng):
    from aspire_amd._lib import AsmcError

    x = torch.zeros((3, 2), dtype=torch.float64, device=eng.device)
    with pytest.raises(AsmcError):
        eng.ensemble_propose(x, "de", 2, 0, G0, SIGMA, 1, 0, 0, 0)
    x = torch.zeros((8, 2), dtype=torch.float64, device=eng.device)
    for args in (("de", 4, 0), ("snooker", 2, 0), ("snooker", 4, 4)):
        with pytest.raises(AsmcError):
            eng.ensemble_propose(x, *args, G0, SIGMA, 1, 0, 0, 0)


def test_degenerate_rows(eng):
    """Half the rows are copies of one row (the state after resampling), and one slot of group 0 is built so that r0 + gammas proj
    = 0 exactly (its proposal falls on z): y has no NaN, logf = -inf exactly in those slots and nowhere else, they are rejected
    whatever the densities say, and the state stays finite through all four sweeps."""
    n, d, seed, gammas = 64, 3, 5, 1.0
    g = np.random.default_rng(3)
    x = g.normal(size=(n, d))
    dr = E.draws(n, "snooker", 0, 0, 0, seed)
    i = 0
    k, z, z1, z2 = (int(dr[name][i]) for name in ("k", "z", "z1", "z2"))
    copies = [r for r in range(n) if r not in (k, z, z1, z2)][:n // 2]
    x[copies] = x[copies[0]]
    x[z] = [1.0, -2.0, 0.5]
    x[k] = x[z] + [3.0, 4.0, 0.0]  # delta = (3, 4, 0): r0 = 5 exactly
    x[z2] = [0.25, 1.0, -1.0]
    x[z1] = x[z2] - [3.0, 4.0, 0.0]  # delta . (z1 - z2) = -25: proj = -5 = -r0 / gammas
    xd = torch.from_numpy(x).to(eng.device)
    ll = torch.zeros(n, dtype=torch.float64, device=eng.device)
    lp, lq = ll.clone(), ll.clone()
    for grp in range(4):
        before = xd.cpu().numpy()
        y, logf = eng.ensemble_propose(xd, "snooker", 4, grp, gammas, 0.0, seed, 0, 0, 0)
        y_h, logf_h = y.cpu().numpy(), logf.cpu().numpy()
        dg = E.draws(n, "snooker", grp, 0, 0, seed)
        dup = np.all(before[dg["k"]] == before[dg["z"]], axis=1)
        forced = np.zeros(len(dup), dtype=bool)
        if grp == 0:
            forced[i] = True
            assert dup.any() and not dup[i]
            np.testing.assert_allclose(y_h[i], x[z], atol=2e-15)
        assert not np.isnan(y_h).any() and not np.isnan(logf_h).any()
        assert np.array_equal(np.isneginf(logf_h), dup | forced) and np.all(np.isfinite(logf_h[~(dup | forced)]))
        assert np.array_equal(y_h[dup], before[dg["k"]][dup])
        big = torch.full((len(y_h),), 50.0, dtype=torch.float64, device=eng.device)  # a density that would accept anything
        zero = torch.zeros_like(big)
        eng.ensemble_accept(xd, 4, grp, y, logf, 1.0, ll, lp, lq, big, zero, zero, seed, 0, 0, 0)
        after = xd.cpu().numpy()
        bad = dg["k"][dup | forced]
        assert np.array_equal(after[bad], before[bad]) and np.all(ll.cpu().numpy()[bad] == 0.0)
        good = dg["k"][~(dup | forced)]
        assert np.array_equal(after[good], y_h[~(dup | forced)])
        assert np.all(np.isfinite(after))


@pytest.mark.parametrize("move", ["de", "snooker"])
def test_same_seed_same_bits(eng, move):
    x = torch.from_numpy(np.random.default_rng(1).normal(size=(5001, 9))).to(eng.device)
    nsplits, p0, p1 = (2, G0, SIGMA) if move == "de" else (4, GAMMAS, 0.0)
    a = [eng.ensemble_propose(x, move, nsplits, g, p0, p1, 42, 1, 7, 0) for g in range(nsplits)]
    b = [eng.ensemble_propose(x, move, nsplits, g, p0, p1, 42, 1, 7, 0) for g in range(nsplits)]
    c = eng.ensemble_propose(x, move, nsplits, 0, p0, p1, 43, 1, 7, 0)
    for (ya, fa), (yb, fb) in zip(a, b):
        assert torch.equal(ya, yb) and torch.equal(fa, fb)
    assert not torch.equal(a[0][0], c[0])


def test_stretch_entry_points_keep_their_bits(eng):
    """asmc_stretch_* share their device code with the new moves: the same bits as the restatement (what
    tests/test_gpu_emcee_smc.py pins), before and after the other kernels have run."""
    n, d, seed, shard, step = 4097, 7, 0x0123456789ABCDEF, 3, 11
    x = np.random.default_rng(n + d).normal(size=(n, d))
    xd = torch.from_numpy(x).to(eng.device)
    for h in (0, 1):
        y0, f0 = eng.stretch_propose(xd, h, 2.0, seed, shard, step, 0)
        eng.ensemble_propose(xd, "snooker", 4, h, GAMMAS, 0.0, seed, shard, step, 1)
        eng.ensemble_propose(xd, "de", 2, h, G0, SIGMA, seed, shard, step, 1)
        y1, f1 = eng.stretch_propose(xd, h, 2.0, seed, shard, step, 0)
        assert torch.equal(y0, y1) and torch.equal(f0, f1)
        assert np.array_equal(y0.cpu().numpy(), S.propose(x, h, 2.0, seed, shard, step)[0])


def _run(eng, d, n, seed, moves):
    from aspire_amd import Aspire, Samples
    from aspire_amd.targets import DiagGaussianMixture

    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend="gaussian", engine=eng, seed=seed)
    aspire.fit(Samples(1.5 * np.random.default_rng(seed).normal(size=(5000, d))))
    out, hist = aspire.sample_posterior(sampler="emcee_smc", n_samples=n, engine=eng, rng=np.random.default_rng(1000 + seed),
                                        store_sample_history=False, return_history=True, sampler_kwargs={"moves": moves})
    return aspire, out, hist


def test_logz_d8_eight_seeds_with_the_mixture(eng):
    """tests/test_gpu_emcee_smc.py::test_logz_d8_eight_seeds with emcee's mixture for multi-modal targets; same seeds, same bound."""
    from aspire_amd import DEMove, DESnookerMove

    d, true = 8, 4.0 * math.log(math.pi)
    z = []
    for s in range(8):
        aspire, out, hist = _run(eng, d, 100_000, s, [(DEMove(), 0.8), (DESnookerMove(), 0.2)])
        z.append((float(out.log_evidence) - true) / float(out.log_evidence_error))
        assert hist.beta[-1] == 1.0 and len(hist.mcmc_autocorr) == len(hist.beta)
        assert "de" in aspire.sampler.last_mutation_path and "snooker" in aspire.sampler.last_mutation_path
    z = np.array(z)
    print(f"emcee_smc DE/snooker d=8 N=100000 z-scores: {np.round(z, 2).tolist()}, acceptance {np.round(hist.mcmc_acceptance, 3).tolist()}")
    assert abs(z.mean()) <= 1.0 and np.sqrt((z**2).mean()) <= 1.6, z


def test_emcee_sampler_with_the_mixture(eng):
    from test_mcmc_samplers import POST_MEAN, POST_VAR, make

    from aspire_amd import DEMove, DESnookerMove

    sp = make("emcee", d=4, eng=eng)
    out = sp.sample(nwalkers=4096, nsteps=60, discard=30, moves=[(DEMove(), 0.8), (DESnookerMove(), 0.2)])
    x = np.asarray(out.x.cpu() if hasattr(out.x, "cpu") else out.x)
    assert out.chain_shape == (30, 4096) and "snooker" in sp.last_mutation_path
    assert np.all(np.abs(x.mean(0) - POST_MEAN) < 0.05) and np.all(np.abs(x.var(0) - POST_VAR) < 0.08)
