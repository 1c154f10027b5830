"""The NUTS kernels of the "blackjax_smc" sampler on the HIP engine (csrc/asmc_nuts.hip; include/asmc.h asmc_nuts_*).

* k_nuts_mix, one transition, against tests/nuts_ref.py on n in {7, 257, 4097} x one d per instantiation: depth, leapfrog steps, flags
  and position of every row equal; the new points within nuts_ref.nuts_tolerance's tol_x (8 x |fp64 - long double| of the restatement
  on that case + 64 ulp of the row's largest coordinate); rows with a decision within 1e-9 of its threshold are left out, at most 1 %
  of a case (tests/test_nuts.py: the restatement leaves out none); the four device counters against the restatement's integers;
* `max_blocks`: every block walks several tiles and reuses its slab of the checkpoint workspace - bit for bit the default launch;
* several transitions in one launch = the same transitions launched one by one, bit for bit, statistics per transition included;
* edges: max_num_doublings = 1, a case with divergent and turning rows, rows that start in a -inf / NaN hole;
* stationarity on a Gaussian to exact 5-sigma bounds;
* the split launches (k_nuts_begin / select / drift / leaf / merge / finish) driven one by one around an autograd lambda: per-row
  diagnostics against the fused kernel and the restatement, the counters of k_nuts_finish, an fp32 state; then the same through
  the sampler's `mutate`;
* divergence at the default threshold, up to energies that overflow;
* end to end through `Aspire(...).sample_posterior(sampler="blackjax_smc")`: log Z, the likelihood hole, reproducibility.
Every call passes an explicit step_size: the reference's default 1e-3 builds ten doublings per transition.
Specification: reference src/aspire/samplers/smc/blackjax.py:119, 229-277.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hmc_ref as H
import nuts_ref as N

pytestmark = pytest.mark.gpu

CASES = N.fused_cases()
# A row whose 2^32 acceptance lies this close to a half-integer may round the other way on the device: the acceptance is a mean of
# exp's of energy differences known to the tolerance scheme's ~1e-13 relative, so 2^32 of it carries an absolute error below 1e-6
NEAR_ROUNDING = 1e-5


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


def _dev(eng, a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=eng.device, dtype=dtype)


def _launch(eng, mixes, x, beta, eps, mass, key, n_steps=1, max_doublings=10, threshold=1000.0, max_blocks=0, dens=None):
    """One asmc_nuts_mix launch from fresh device copies: (x, ll, lp, lq, info, stats) on the host, and the device mixtures."""
    seed, gid0, step = key
    dm = [eng.make_mixture(*m) for m in mixes]
    xd = _dev(eng, x)
    dens = [eng.mixture_logpdf(xd, m) for m in dm] if dens is None else [_dev(eng, v) for v in dens]
    md = None if mass is None else _dev(eng, mass)
    info = eng.nuts_mix(xd, *dens, beta, *dm, md, eps, max_doublings, threshold, seed, gid0, step, n_steps, want_info=True,
                        max_blocks=max_blocks)
    stats = eng.nuts_stats(n_steps)
    return SimpleNamespace(x=xd.cpu().numpy(), dens=[v.cpu().numpy() for v in dens], info=info.cpu().numpy(), stats=stats, xd=xd, dm=dm,
                           dens_d=dens)


def _check_stats(stats, r64, keep, s=0):
    """The device counters of transition `s` against the restatement's integers: equal up to what the rows left out can hold, the
    acceptance sum also up to one unit per row that sits at a rounding boundary."""
    out = int((~keep).sum())
    ref = np.array([int((r64["infos"][s][:, 3] != 0).sum()), int(r64["infos"][s][:, 1].sum()), int((r64["infos"][s][:, 2] & 1).sum())])
    assert abs(int(stats[0]) - ref[0]) <= out and abs(int(stats[1]) - ref[1]) <= 1023 * out and abs(int(stats[2]) - ref[2]) <= out, (stats, ref)
    near = int((r64["accfrac"][s] < NEAR_ROUNDING).sum())
    assert abs(int(stats[3]) - int(r64["accq"][s].sum())) <= near + out * (1 << 32), (int(stats[3]), int(r64["accq"][s].sum()), near)


@pytest.mark.parametrize("n,d,C,diag,beta,eps", CASES, ids=[f"n{c[0]}-d{c[1]}-C{c[2]}-{'diag' if c[3] else 'unit'}-b{c[4]}-e{c[5]}" for c in CASES])
def test_nuts_mix_one_transition_against_the_restatement(eng, n, d, C, diag, beta, eps):
    """Largest tolerance over the grid on MI355X: 1.0e-12 (n = 4097, d = 32, C = 3; the device differs by 1.6e-13 there); largest
    device difference: 2.0e-13 (n = 129, d = 128, C = 3; tolerance 3.9e-13).  DESIGN.md §3.18."""
    mixes, x, mass, (r64, rld, tol_x, keep, gap) = N.fused_case_reference(n, d, C, diag, beta, eps)
    dev = _launch(eng, mixes, x, beta, eps, mass, N.CASE_KEY)
    out = int((~keep).sum())
    assert out <= n // 100, (out, n)
    same = (dev.info == r64["info"]).all(axis=1)
    err = np.abs(dev.x - r64["x64"]).max(axis=1)
    print(f"nuts_mix n={n} d={d} C={C}: depths {np.bincount(dev.info[:, 0]).tolist()}, rows left out {out}, max |x dev - ref| "
          f"{err[keep].max():.3e}, tolerance {tol_x.max():.3e} (fp64 vs long double {gap:.3e})")
    assert same[keep].all(), np.flatnonzero(~same & keep)[:10]
    assert np.all(err[keep] <= tol_x[keep]), (err[keep].max(), tol_x.max())
    moved = dev.info[:, 3] != 0
    assert np.array_equal(dev.x[~moved], x[~moved]) and moved.any()
    for got, m in zip(dev.dens_d, dev.dm):  # every row's carried densities are the densities of the stored row
        torch.testing.assert_close(got, eng.mixture_logpdf(dev.xd, m), rtol=1e-12, atol=1e-12)
    # the counters are the sums of the per-row output, and the restatement's integers
    assert dev.stats[0, :3].tolist() == [int(moved.sum()), int(dev.info[:, 1].sum()), int((dev.info[:, 2] & 1).sum())]
    _check_stats(dev.stats[0], r64, keep)
    again = _launch(eng, mixes, x, beta, eps, mass, N.CASE_KEY)  # a second run: identical bits
    assert np.array_equal(again.x, dev.x) and np.array_equal(again.info, dev.info) and np.array_equal(again.stats, dev.stats)
    assert all(np.array_equal(a, b) for a, b in zip(again.dens, dev.dens))


def test_max_blocks_three_equals_the_default_launch(eng):
    """n = 4097, d = 7: 32 rows per block, 129 tiles; three blocks walk 43 tiles each through one workspace slab each."""
    mixes, x, mass = N.mix_case(4097, 7, 3, 77)
    a = _launch(eng, mixes, x, 0.6, 0.2, mass, N.CASE_KEY, n_steps=2)
    b = _launch(eng, mixes, x, 0.6, 0.2, mass, N.CASE_KEY, n_steps=2, max_blocks=3)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.info, b.info) and np.array_equal(a.stats, b.stats)
    assert all(np.array_equal(u, v) for u, v in zip(a.dens, b.dens))
    assert a.stats[:, 1].min() > 4097 and not np.array_equal(a.x, x)


def test_transitions_in_one_launch_equal_transitions_launched_one_by_one(eng):
    n, d, steps = 257, 7, 5
    mixes, x, mass = N.mix_case(n, d, 3, 5)
    key = (99, 1000, 10)
    a = _launch(eng, mixes, x, 0.5, 0.3, mass, key, n_steps=steps)
    xb, db, sb = x, None, []
    for s in range(steps):
        b = _launch(eng, mixes, xb, 0.5, 0.3, mass, (99, 1000, 10 + s), dens=db)
        xb, db = b.x, b.dens
        sb.append(b.stats[0])
    assert np.array_equal(a.stats, np.array(sb)) and np.array_equal(a.x, b.x) and np.array_equal(a.info, b.info)
    assert all(np.array_equal(u, v) for u, v in zip(a.dens, b.dens))
    r64, rld, tol_x, keep, gap = N.nuts_tolerance(mixes, 0.5, x, 0.3, mass, *key, n_steps=steps)
    assert int((~keep).sum()) <= n // 100
    for s in range(steps):
        _check_stats(a.stats[s], r64, keep, s)
    assert np.array_equal(a.info[keep], r64["info"][keep])
    assert np.all(np.abs(a.x - r64["x64"]).max(axis=1)[keep] <= tol_x[keep])


def test_max_num_doublings_one(eng):
    mixes, x, mass = N.mix_case(257, 13, 1, 3)
    dev = _launch(eng, mixes, x, 0.6, 0.3, mass, N.CASE_KEY, max_doublings=1)
    r64, _, tol_x, keep, _ = N.nuts_tolerance(mixes, 0.6, x, 0.3, mass, *N.CASE_KEY, max_doublings=1)
    assert keep.all() and np.array_equal(dev.info, r64["info"]) and dev.info[:, 1].max() == 1 and np.all(dev.info[:, 0] == 1)
    assert np.all(np.abs(dev.x - r64["x64"]).max(axis=1) <= tol_x) and dev.stats[0, 1] == 257


def test_divergent_and_turning_rows(eng):
    mixes, x, beta, eps, thr = N.divergent_case()
    dev = _launch(eng, mixes, x, beta, eps, None, N.CASE_KEY, threshold=thr)
    r64, _, tol_x, keep, _ = N.nuts_tolerance(mixes, beta, x, eps, None, *N.CASE_KEY, threshold=thr)
    assert keep.all() and np.array_equal(dev.info, r64["info"])
    assert (dev.info[:, 2] & N.DIVERGENT).sum() >= 50 and (dev.info[:, 2] & N.TURNING).sum() >= 50
    assert np.all(np.abs(dev.x - r64["x64"]).max(axis=1) <= tol_x)
    _check_stats(dev.stats[0], r64, keep)


@pytest.mark.parametrize("eps", [3.0, 1e160], ids=["step3", "step1e160"])
def test_divergence_at_the_default_threshold(eng, eps):
    """Energies that blow up: at step 3 the restatement has 42 divergent and 215 turning rows at the default threshold of 1000; at
    step 1e160 the first leaf of every row overflows (delta is inf or NaN) and every row is divergent after one step.  No row moves."""
    mixes, x, _ = N.mix_case(257, 7, 3, 15)
    dev = _launch(eng, mixes, x, 0.6, eps, None, N.CASE_KEY)
    r64, _, tol_x, keep, _ = N.nuts_tolerance(mixes, 0.6, x, eps, None, *N.CASE_KEY)
    ndiv = int((r64["info"][:, 2] & N.DIVERGENT).sum())
    assert keep.all() and np.array_equal(dev.info, r64["info"]) and (ndiv == 257 if eps > 3 else 20 <= ndiv <= 200)
    assert np.all(np.abs(dev.x - r64["x64"]).max(axis=1) <= tol_x) and np.array_equal(dev.x[dev.info[:, 3] == 0], x[dev.info[:, 3] == 0])
    assert dev.stats[0, :3].tolist() == [int((dev.info[:, 3] != 0).sum()), int(dev.info[:, 1].sum()), ndiv]
    _check_stats(dev.stats[0], r64, keep)


def test_rows_that_start_in_a_hole_stay(eng):
    """A row whose tempered target is -inf (a coordinate of 1e200: the quadratic form overflows) or NaN at the start takes no step
    and is written nowhere; its neighbours in the same wave and row group are unaffected."""
    mixes, x, mass = N.mix_case(257, 7, 3, 21)
    clean = _launch(eng, mixes, x, 0.6, 0.3, mass, N.CASE_KEY)
    xh = x.copy()
    xh[::7, 2] = 1e200
    xh[3::7, 5] = np.nan
    hole = np.zeros(257, dtype=bool)
    hole[::7] = hole[3::7] = True
    dens = [np.full(257, 0.25), np.full(257, -1.5), np.full(257, 7.0)]  # (the carried arrays are outputs only)
    dev = _launch(eng, mixes, xh, 0.6, 0.3, mass, N.CASE_KEY, dens=dens)
    assert np.all(dev.info[hole] == 0) and np.array_equal(dev.x[hole], xh[hole], equal_nan=True)
    assert all(np.array_equal(got[hole], old[hole]) for got, old in zip(dev.dens, dens))
    assert np.array_equal(dev.x[~hole], clean.x[~hole]) and np.array_equal(dev.info[~hole], clean.info[~hole])
    assert dev.stats[0, 1] == clean.info[~hole, 1].sum()


def _gaussian_target(eng, d, var):
    """ll = N(0, diag var) un-normalised, a flat prior (precision 1e-30) and, at beta = 1, an idle proposal."""
    ll = eng.make_mixture([0.0], np.zeros((1, d)), (1.0 / np.asarray(var))[None])
    flat = eng.make_mixture([0.0], np.zeros((1, d)), np.full((1, d), 1e-30))
    return ll, flat, flat


def test_stationarity_on_a_gaussian(eng):
    """Exact draws of N(0, diag v), 30 transitions: the particles are independent chains, each still distributed as the target, so
    the bounds are exact 5-sigma bounds of a sample of n."""
    n, d, steps = 200_000, 8, 30
    v = np.linspace(0.5, 2.0, d)
    x = np.random.default_rng(9).normal(size=(n, d)) * np.sqrt(v)
    xd = _dev(eng, x)
    zero = [torch.zeros(n, dtype=torch.float64, device=eng.device) for _ in range(3)]
    eng.nuts_mix(xd, *zero, 1.0, *_gaussian_target(eng, d, v), None, 0.35, 10, 1000.0, 31337, 0, 0, steps)
    stats = eng.nuts_stats(steps)
    acc = stats[:, 3].sum() / (N.TWO32 * n * steps)
    got = xd.cpu().numpy()
    mean, var = got.mean(axis=0), got.var(axis=0, ddof=1)
    print(f"stationarity: acceptance {acc:.3f}, steps per transition {stats[:, 1].sum() / (n * steps):.2f}, max |mean| / sigma "
          f"{np.max(np.abs(mean) / np.sqrt(v / n)):.2f}, max |var - v| / sigma {np.max(np.abs(var - v) / (v * math.sqrt(2.0 / (n - 1)))):.2f}")
    assert 0.8 < acc < 0.999 and stats[:, 2].sum() == 0 and stats[:, 0].min() > 0.9 * n
    assert np.all(np.abs(mean) <= 5.0 * np.sqrt(v / n))
    assert np.all(np.abs(var - v) <= 5.0 * v * math.sqrt(2.0 / (n - 1)))


def _torch_target(eng, mixes, beta):
    """z -> (gradient of the tempered log-target, ll, lp, lq) by torch.autograd on the mixtures written out in torch."""
    tm = [[_dev(eng, np.asarray(a)) for a in m] for m in mixes]

    def logf(m, z):
        logw, mu, prec = m
        t = z[:, None, :] - mu[None]
        return torch.logsumexp(logw[None] - 0.5 * (t * t * prec[None]).sum(-1), dim=1)

    def target(z):
        with torch.enable_grad():
            leaf = z.detach().clone().requires_grad_(True)
            ll, lp, lq = (logf(m, leaf) for m in tm)
            lpt = (1.0 - beta) * lq + beta * (ll + lp)
            g = torch.autograd.grad(torch.where(torch.isfinite(lpt), lpt, torch.zeros_like(lpt)).sum(), leaf)[0]
        return g.contiguous(), ll.detach(), lp.detach(), lq.detach()

    return target


def _split_transition(eng, mixes, x, beta, eps, mass, key, threshold=1000.0, max_doublings=10, dtype=torch.float64):
    """One transition through the split launches themselves (asmc_nuts_begin / select / drift / leaf / merge / finish), the state of
    dtype `dtype`: (x, info, stats) on the host and the number of host reads (merges)."""
    seed, gid0, step = key
    target = _torch_target(eng, mixes, beta)
    xd = _dev(eng, x, dtype)
    n, d = x.shape
    z0 = xd.to(torch.float64)
    g0, ll0, lp0, lq0 = target(z0)
    dens = [ll0.clone(), lp0.clone(), lq0.clone()]
    st = eng.nuts_state(n, d, max_doublings, None if mass is None else _dev(eng, mass), eps, beta, threshold)
    eng.nuts_set_point(st, z0, g0, ll0, lp0, lq0)
    eng.nuts_begin(st, seed, gid0, step)
    merges = 0
    for j in range(max_doublings):
        eng.nuts_select(st)
        for i in range(1 << j):
            eng.nuts_drift(st)
            eng.nuts_leaf(st, i, *target(st.z))
        merges += 1
        if eng.nuts_merge(st, j) == 0:
            break
    info = eng.nuts_finish(st, xd, *dens, 0, want_info=True)
    return SimpleNamespace(x=xd.cpu().numpy(), info=info.cpu().numpy(), stats=eng.nuts_stats(1), merges=merges,
                           dens=[v.cpu().numpy() for v in dens], dens0=[v.cpu().numpy() for v in (ll0, lp0, lq0)])


SPLIT_CASES = {  # mixes, x, beta, step_size, diagonal mass, threshold
    "n4097-d7": lambda: H.split_fused_case()[:4] + (None, 1000.0),
    "divergent-and-turning": lambda: N.divergent_case()[:4] + (None, N.divergent_case()[4]),
    "default-threshold-step3-diag": lambda: N.mix_case(257, 7, 3, 15)[:2] + (0.6, 3.0, N.mix_case(257, 7, 3, 15)[2], 1000.0),
    "n257-d33-diag": lambda: N.mix_case(257, 33, 1, 8)[:2] + (1.0, 0.2, N.mix_case(257, 33, 1, 8)[2], 1000.0),
}


@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_split_launches_against_the_fused_kernel_and_the_restatement(eng, name):
    """The split kernels driven launch by launch around an autograd lambda: every row's depth, leapfrog steps, flags and position
    equal the fused kernel's and the restatement's (rows left out by the 1e-9 rule: at most 1 %), the points lie within the
    restatement's tolerance, the four counters of k_nuts_finish are the column sums of its per-row output and the restatement's
    integers, unmoved rows and their carried densities are untouched, and the host read once per doubling."""
    mixes, x, beta, eps, mass, thr = SPLIT_CASES[name]()
    n = len(x)
    r64, _, tol_x, keep, _ = N.nuts_tolerance(mixes, beta, x, eps, mass, *N.CASE_KEY, threshold=thr)
    assert int((~keep).sum()) <= n // 100
    fused = _launch(eng, mixes, x, beta, eps, mass, N.CASE_KEY, threshold=thr)
    split = _split_transition(eng, mixes, x, beta, eps, mass, N.CASE_KEY, threshold=thr)
    print(f"split {name}: depths {np.bincount(split.info[:, 0]).tolist()}, divergent {int((split.info[:, 2] & 1).sum())}, turning "
          f"{int((split.info[:, 2] & 2).sum()) // 2}, rows left out {int((~keep).sum())}, max |x - ref| "
          f"{np.abs(split.x - r64['x64']).max(axis=1)[keep].max():.3e} (tolerance {tol_x.max():.3e})")
    assert np.array_equal(split.info[keep], r64["info"][keep]) and np.array_equal(split.info[keep], fused.info[keep])
    assert np.all(np.abs(split.x - r64["x64"]).max(axis=1)[keep] <= tol_x[keep])
    moved = split.info[:, 3] != 0
    assert split.stats[0].tolist()[:3] == [int(moved.sum()), int(split.info[:, 1].sum()), int((split.info[:, 2] & 1).sum())]
    _check_stats(split.stats[0], r64, keep)
    assert abs(int(split.stats[0, 3]) - int(fused.stats[0, 3])) <= 2 * int((r64["accfrac"][0] < NEAR_ROUNDING).sum()) + int((~keep).sum()) * (1 << 32)
    assert np.array_equal(split.x[~moved], x[~moved]) and all(np.array_equal(a[~moved], b[~moved]) for a, b in zip(split.dens, split.dens0))
    deepest = int(split.info[:, 0].max())
    assert deepest <= split.merges <= min(10, deepest + 1)  # one host read per doubling that was started


def test_split_launches_with_an_fp32_state(eng):
    """k_nuts_finish<float>: the tree runs in fp64 from the stored fp32 rows, a moved row is rounded once.  Diagnostics against the
    restatement started from the same rows; a stored row is the restatement's point to half an fp32 ulp plus its tolerance."""
    mixes, x, mass = N.mix_case(257, 13, 3, 12)
    x32 = x.astype(np.float32)
    xs = x32.astype(np.float64)
    r64, _, tol_x, keep, _ = N.nuts_tolerance(mixes, 0.6, xs, 0.25, mass, *N.CASE_KEY)
    split = _split_transition(eng, mixes, x32, 0.6, 0.25, mass, N.CASE_KEY, dtype=torch.float32)
    assert keep.all() and split.x.dtype == np.float32 and np.array_equal(split.info, r64["info"])
    moved = split.info[:, 3] != 0
    assert moved.sum() > 200 and np.array_equal(split.x[~moved], x32[~moved])
    half_ulp = 0.5 * np.spacing(np.abs(r64["x64"]).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(split.x.astype(np.float64) - r64["x64"]) <= half_ulp + tol_x[:, None])
    assert split.stats[0].tolist()[:3] == [int(moved.sum()), int(split.info[:, 1].sum()), int((split.info[:, 2] & 1).sum())]
    _check_stats(split.stats[0], r64, keep)
    for got, ref in zip(split.dens, r64["dens"]):  # the carried densities are those of the unrounded point
        np.testing.assert_allclose(got[moved], ref[moved], rtol=1e-11, atol=1e-11)


def test_split_path_against_fused_path(eng):
    """The mixtures of hmc_ref.split_fused_case as built-ins (fused kernel) and wrapped as torch lambdas (autograd gradients between
    the split launches): one transition, n = 4097, d = 7.  Diagnostics equal, points within the restatement's tolerance, the same
    rows left out (at most 1 %)."""
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.history import SMCHistory
    from aspire_amd.samplers.blackjax_smc import HipBlackJAXSMC
    from aspire_amd.targets import DiagGaussianMixture

    mixes, x, beta, eps, _, seed = H.split_fused_case()
    n, d = x.shape
    (lw, mu, pr), (plw, pmu, ppr), (_, qmu, qpr) = mixes
    lik = DiagGaussianMixture(mu, 1.0 / pr, weights=[0.2, 0.3, 0.5])
    prior = DiagGaussianMixture(pmu, 1.0 / ppr)
    r64, rld, tol_x, keep, gap = N.nuts_tolerance(mixes, beta, x, eps, None, seed, 0, 0)
    assert int((~keep).sum()) <= n // 100
    out = {}
    for name, (fl, fp, xp) in {"fused": (lik, prior, np), "split": (lambda s: lik(s.x), lambda s: prior(s.x), torch)}.items():
        flow = GaussianFlow(d, mu=qmu[0], sigma=1.0 / np.sqrt(qpr[0]), engine=eng, seed=1)
        sp = HipBlackJAXSMC(log_likelihood=fl, log_prior=fp, dims=d, prior_flow=flow, xp=xp, engine=eng, rng=np.random.default_rng(0))
        sp.sampler_kwargs = {"algorithm": "nuts", "step_size": eps, "n_steps": 1, "max_num_doublings": 10, "divergence_threshold": 1000.0}
        sp.key, sp._minv, sp.history = 42, None, SMCHistory()
        xd = _dev(eng, x)
        dm = [eng.make_mixture(*m) for m in mixes]
        parts = sp._wrap(xd, *(eng.mixture_logpdf(xd, m) for m in dm), beta)
        new = sp.mutate(parts, beta)
        assert "nuts " + name in sp.last_mutation_path
        out[name] = (new.x.cpu().numpy(), sp.history.mcmc_acceptance[-1], sp.last_nuts)
    for name, (xs, acc, last) in out.items():
        err = np.abs(xs - r64["x64"]).max(axis=1)
        print(f"{name}: max |x - ref| {err[keep].max():.3e} (tolerance {tol_x.max():.3e}), acceptance {acc:.4f}, {last}")
        assert np.all(err[keep] <= tol_x[keep]), name
        assert last["mean_depth"] == pytest.approx(r64["info"][:, 0].mean(), abs=10 * (n - keep.sum()) / n + 1e-9)
    near = int((r64["accfrac"][0] < NEAR_ROUNDING).sum()) + int((~keep).sum()) * (1 << 32)
    assert abs(out["fused"][1] - out["split"][1]) * N.TWO32 * n <= 2 * near + 1
    assert abs(out["fused"][2]["steps_per_transition"] - out["split"][2]["steps_per_transition"]) * n <= 1023 * int((~keep).sum()) + 1e-6
    assert 0.5 < out["fused"][1] < 1.0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _run(eng, d, n, seed, sampler_kwargs, xp=np, lik=None):
    from aspire_amd import Aspire, Samples
    from aspire_amd.targets import DiagGaussianMixture

    lik = lik or DiagGaussianMixture.isotropic(d, normalized=False)
    aspire = Aspire(log_likelihood=lik, log_prior=lik, dims=d, flow_backend="gaussian", engine=eng, seed=seed, xp=xp)
    aspire.fit(Samples(1.5 * np.random.default_rng(seed).normal(size=(5000, d))))
    out, hist = aspire.sample_posterior(sampler="blackjax_smc", n_samples=n, engine=eng, rng=np.random.default_rng(1000 + seed),
                                        rng_key=seed, sampler_kwargs=sampler_kwargs, store_sample_history=False, return_history=True)
    return aspire, out, hist


def test_nuts_logz_d8_eight_seeds(eng):
    d, true = 8, 4.0 * math.log(math.pi)
    z = []
    for s in range(8):
        aspire, out, hist = _run(eng, d, 50_000, s, {"algorithm": "nuts", "step_size": 0.3, "n_steps": 8})
        z.append((float(out.log_evidence) - true) / float(out.log_evidence_error))
        assert hist.beta[-1] == 1.0 and len(hist.mcmc_acceptance) == len(hist.beta) and "nuts fused" in aspire.sampler.last_mutation_path
        assert all(0.5 < a <= 1.0 for a in hist.mcmc_acceptance) and aspire.sampler.last_nuts["divergent_share"] == 0.0
    z = np.array(z)
    print(f"blackjax_smc nuts d=8 N=50000 z-scores: {np.round(z, 2).tolist()}, last mutation {aspire.sampler.last_nuts}")
    assert abs(z.mean()) <= 1.0 and np.sqrt((z**2).mean()) <= 1.6, z


@pytest.mark.parametrize("value", [-np.inf, np.nan, np.inf], ids=["-inf", "nan", "+inf"])
def test_likelihood_hole(eng, value):
    """tests/test_gpu_blackjax_smc.py test_likelihood_hole's construction with algorithm = "nuts" (torch callables: the split path)."""
    from test_likelihood_hole import check_hole_run

    from aspire_amd import Aspire, Samples

    d, n, seed = 2, 4000, 21

    def log_like(samples):
        x = samples.x.to(torch.float64)
        logl = (math.log(1.0 / math.sqrt(2 * math.pi)) - 0.5 * (x - 2.0) ** 2).sum(-1)
        return torch.where(x.norm(dim=1) < 1.0, torch.full_like(logl, value), logl)

    def log_prior(samples):
        x = samples.x.to(torch.float64)
        return torch.where((x >= -10.0) & (x <= 10.0), torch.full_like(x, math.log(1.0 / 20.0)), torch.full_like(x, -math.inf)).sum(-1)

    params = [f"x_{i}" for i in range(d)]
    asp = Aspire(log_likelihood=log_like, log_prior=log_prior, dims=d, parameters=params, prior_bounds={p: [-10, 10] for p in params},
                 bounded_to_unbounded=False, flow_backend="gaussian", engine=eng, seed=seed + 1, xp=torch)
    asp.fit(Samples(np.random.default_rng(seed).normal(2.0, 1.0, size=(500, d)), parameters=params, xp=np))
    kw = {"algorithm": "nuts", "step_size": 0.5, "n_steps": 4, "max_num_doublings": 4}
    out, history = asp.sample_posterior(n_samples=n, sampler="blackjax_smc", return_history=True, engine=eng, sampler_kwargs=kw,
                                        rng=np.random.default_rng(seed + 2))
    assert "nuts split" in asp.sampler.last_mutation_path
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else v  # noqa: E731
    check_hole_run(asp, SimpleNamespace(x=host(out.x), log_likelihood=host(out.log_likelihood), log_prior=host(out.log_prior),
                                        log_evidence=out.log_evidence, log_evidence_error=out.log_evidence_error), history, n)


def test_same_rng_key_same_bits(eng):
    kw = {"algorithm": "nuts", "step_size": 0.3, "n_steps": 4}
    runs = [_run(eng, 8, 20_000, 9, kw) for _ in range(2)]
    assert np.array_equal(np.asarray(runs[0][1].x), np.asarray(runs[1][1].x))
    assert float(runs[0][1].log_evidence) == float(runs[1][1].log_evidence)
    assert runs[0][2].mcmc_acceptance == runs[1][2].mcmc_acceptance and runs[0][0].sampler.last_nuts == runs[1][0].sampler.last_nuts
