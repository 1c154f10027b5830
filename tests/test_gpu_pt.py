"""Parallel tempering on the HIP engine (include/asmc.h asmc_pt_*): the replica exchange against its numpy
restatement (tests/pt_ref.py) - equality everywhere, after asserting that no walker of the fixed inputs lies where a one-ulp
difference of the device's log could flip a decision -, the evidence reductions against a numpy.longdouble evaluation with
tolerances measured from numpy's own fp64 deviation, and the "pt_minipcn" sampler end to end.
"""
import math

import numpy as np
import pytest
import torch

import pt_ref
from pt_ref import gaussian_closed_form, gaussian_targets, pt_z_scores

EPS = np.finfo(np.float64).eps
LADDER = [1.0, 0.55, 0.3, 0.1, 0.0]
SWAP_SHAPES = [(T, W) for T in (2, 3, 5) for W in (1, 7, 257)]


def swap_inputs(T, W):
    """Fixed inputs of a swap case: (ll, lp, two companions [T W], betas [T], seed)."""
    g = np.random.default_rng(100 * T + W)
    ll, lp, c0, c1 = (3.0 * g.normal(size=T * W) for _ in range(4))
    return ll, lp, c0, c1, np.array(LADDER[:T]), int(g.integers(1, 2**63 - 1))


@pytest.mark.parametrize("T,W", SWAP_SHAPES)
def test_no_swap_decision_of_the_fixed_inputs_is_within_four_ulps(T, W):
    """A property of the inputs, checked on the CPU: the device's log may differ from numpy's in the last place."""
    ll, _, _, _, betas, seed = swap_inputs(T, W)
    for rnd in (0, 1, 6, 7):
        assert pt_ref.swap_margin_ulps(ll, betas, seed, rnd) >= 4.0
        rs, acc, _, _ = pt_ref.swap_decisions(ll, betas, seed, rnd)
        if W == 257 and rs:
            assert np.all((acc.sum(axis=1) > 0) & (acc.sum(axis=1) < W))  # every pair of rungs: some walkers exchange, some do not


def dev_rows(eng, x, dtype, shift_bytes=0, guard=3):
    """x [n, d] on the device inside a larger buffer: `guard` rows of a sentinel behind it, the first row `shift_bytes` in."""
    n, d = x.shape
    item = 8 if dtype == torch.float64 else 4
    buf = torch.full((shift_bytes // item + (n + guard) * d,), -777.0, dtype=dtype, device=eng.device)
    view = buf[shift_bytes // item: shift_bytes // item + n * d].view(n, d)
    view.copy_(torch.as_tensor(x, dtype=dtype))
    return buf, view


@pytest.mark.gpu
@pytest.mark.parametrize("T,W", SWAP_SHAPES)
def test_swap_equals_the_restatement(hip_engine, T, W):
    eng = hip_engine
    ll, lp, c0, c1, betas, seed = swap_inputs(T, W)
    betas_d = eng.asarray(betas)
    g = np.random.default_rng(7)
    for rnd in (0, 1, 6, 7):
        assert pt_ref.swap_margin_ulps(ll, betas, seed, rnd) >= 4.0
        for d in (3, 8, 32, 33):
            x64 = g.normal(size=(T * W, d))
            for dtype in (torch.float64, torch.float32):
                x = x64.astype(np.float32 if dtype == torch.float32 else np.float64)
                for n_comp, shift in ((0, 0), (1, 0), (2, 0), (2, 8)):
                    comps = [c0, c1][:n_comp]
                    xo, llo, lpo, co, cnt = pt_ref.swap_ref(x, ll, lp, betas, seed, rnd, comps)
                    buf, xd = dev_rows(eng, x, dtype, shift)
                    lld, lpd = eng.asarray(ll), eng.asarray(lp)
                    cd = [eng.asarray(c) for c in comps] + [None, None]
                    counts = torch.full((max(T - 1, 1),), 5, dtype=torch.int64, device=eng.device)
                    eng.pt_swap(xd, lld, lpd, betas_d, seed, rnd, counts, c0=cd[0], c1=cd[1])
                    what = (T, W, d, dtype, rnd, n_comp, shift)
                    assert xd.cpu().numpy().tobytes() == xo.tobytes(), what
                    assert lld.cpu().numpy().tobytes() == llo.tobytes() and lpd.cpu().numpy().tobytes() == lpo.tobytes(), what
                    for a, b in zip(cd, co):
                        assert a.cpu().numpy().tobytes() == b.tobytes(), what
                    assert np.array_equal(counts.cpu().numpy()[:T - 1] - 5, cnt), what
                    head = shift // x.itemsize
                    rest = torch.cat([buf[:head], buf[head + T * W * d:]]).cpu().numpy()
                    assert np.all(rest == -777.0), what  # rows beyond T W, and the bytes in front of a shifted state
                    unpaired = [r for r in range(T) if r not in [q + k for q in range(rnd & 1, T - 1, 2) for k in (0, 1)]]
                    for r in unpaired:
                        assert np.array_equal(xo[r * W:(r + 1) * W], x[r * W:(r + 1) * W])


@pytest.mark.gpu
def test_swap_leaves_non_finite_pairs_alone(hip_engine):
    """NaN, -inf and +inf in ll on either side of a pair: none is exchanged, none is counted."""
    eng = hip_engine
    T, W, d = 3, 7, 8
    ll, lp, c0, _, betas, seed = swap_inputs(T, W)
    ll = ll.copy()
    ll[0:W] = 50.0  # the hotter side far better: every pair of rungs (0, 1) that is finite on both sides exchanges
    ll[W:2 * W] = 90.0
    for w, (side, value) in enumerate([(0, np.nan), (1, np.nan), (0, -np.inf), (1, -np.inf), (0, np.inf), (1, np.inf)]):
        ll[side * W + w] = value
    x = np.random.default_rng(1).normal(size=(T * W, d))
    xd, lld, lpd, c0d = eng.asarray(x), eng.asarray(ll), eng.asarray(lp), eng.asarray(c0)
    counts = torch.zeros(T - 1, dtype=torch.int64, device=eng.device)
    eng.pt_swap(xd, lld, lpd, eng.asarray(betas), seed, 0, counts, c0=c0d)
    xo, llo, lpo, co, cnt = pt_ref.swap_ref(x, ll, lp, betas, seed, 0, [c0])
    assert list(cnt) == [1, 0] and np.array_equal(counts.cpu().numpy(), cnt)  # only walker 6, whose pair is finite, moves
    got = xd.cpu().numpy()
    assert got.tobytes() == xo.tobytes() and np.array_equal(got[:6], x[:6]) and np.array_equal(got[W:W + 6], x[W:W + 6])
    assert np.array_equal(got[6], x[W + 6]) and np.array_equal(got[W + 6], x[6])
    assert lld.cpu().numpy().tobytes() == llo.tobytes() and c0d.cpu().numpy().tobytes() == co[0].tobytes()


# ---- evidence reductions ------------------------------------------------------------------------------------------------------
def evidence_bounds(rows, coef):
    """Per output of asmc_pt_evidence [T + 1, 4]: the larger of 8 x the deviation of numpy's own fp64 evaluation from the long-double
    one (the kernel sums in another order) and the forward bound of a sum in any order, n eps sum |terms|.  For the per-sample
    trapezoid the terms carry their own rounding, (T eps) sum_r |c_r ll|: (n + T) eps mean_i sum_r |c_r ll| on the mean, and on the
    centred second moment (n + T) eps M2 plus 2 sum_i |ti_i - mean| times that perturbation."""
    T, n = rows.shape
    ld = pt_ref.evidence_table(rows, coef, np.longdouble)
    f64 = pt_ref.evidence_table(rows, coef, np.float64)
    with np.errstate(invalid="ignore"):
        tol = 8.0 * np.abs(f64.astype(np.longdouble) - ld).astype(np.float64)
    fwd = np.zeros((T + 1, 4))
    for r in range(T):
        fwd[r] = (n * EPS * np.sum(np.abs(rows[r])), 0.0, n * EPS * float(ld[r, 2]), n * EPS * float(ld[r, 3]))
    mag = np.sum(np.abs(coef[0][:, None] * rows), axis=0)
    ti = np.sum(coef[0][:, None] * rows, axis=0)
    fwd[T, 1] = (n + T) * EPS * float(np.mean(mag))
    with np.errstate(invalid="ignore"):
        fwd[T, 2] = (n + T) * EPS * float(ld[T, 2]) + 2.0 * float(np.sum(np.abs(ti - np.mean(ti)))) * T * EPS * float(np.max(mag))
    return ld, f64, np.fmax(np.nan_to_num(tol, nan=0.0), np.nan_to_num(fwd, nan=0.0))


EVIDENCE_N = [1, 255, 256, 257, 70001]


@pytest.fixture(scope="module")
def evidence_rows():
    """One fp64 chain [5, 70001 + 5] shared by every case."""
    return -40.0 + 25.0 * np.random.default_rng(11).normal(size=(5, 70006))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [2, 3, 5])
def test_evidence_reductions_against_long_double(hip_engine, evidence_rows, T):
    """Observed on MI355X: the kernel's deviation stays below its bound by the factors printed here."""
    eng = hip_engine
    coef = pt_ref.trapezoid_coefficients(LADDER[:T - 1] + [0.0])
    worst = 0.0
    for n in EVIDENCE_N:
        for offset in (0, 5):
            stride = n + offset
            block = np.ascontiguousarray(evidence_rows[:T, :stride])
            got = eng.pt_evidence(eng.asarray(block.reshape(-1)), T, stride, offset, n, coef)
            rows = block[:, offset:]
            ld, f64, tol = evidence_bounds(rows, coef)
            assert got[T, 0] == n and got[T, 3] == 0.0
            assert np.array_equal(got[1:T, 1], f64[1:T, 1])  # the maxima are exact: one fp64 product per sample, as numpy's
            for r in range(T + 1):
                for j in ((0, 2, 3) if r < T else (1, 2)):
                    if r == 0 and j > 0:
                        continue  # (rung 0 has no stepping stone)
                    dev = abs(float(np.longdouble(got[r, j]) - ld[r, j]))
                    assert dev <= tol[r, j], (T, n, offset, r, j, dev, tol[r, j])
                    if tol[r, j] > 0:
                        worst = max(worst, dev / tol[r, j])
    print(f"T = {T}: largest kernel deviation / bound = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, 70001])
def test_evidence_of_a_constant_chain_is_exact(hip_engine, n):
    from aspire_amd import PTMCMCSamples

    eng = hip_engine
    T, W = 3, 1
    ll = torch.full((T, n, W), -1234.56789, dtype=torch.float64, device=eng.device)
    s = PTMCMCSamples.from_chain(chain=torch.zeros((T, n, W, 2), dtype=torch.float64, device=eng.device), betas=[1.0, 0.3, 0.0],
                                 log_likelihood=ll, xp=torch, engine=eng)
    tab = eng.pt_evidence(ll.reshape(-1), T, n, 0, n, pt_ref.trapezoid_coefficients([1.0, 0.3, 0.0]))
    assert tab[T, 2] == 0.0 and np.all(tab[1:T, 1:] == [[-1234.56789 * 0.7, n, n], [-1234.56789 * 0.3, n, n]])
    logz, err = s.log_evidence_thermodynamic_integration(burn_in_fraction=None)
    assert err == 0.0 and logz == pytest.approx(-1234.56789, rel=max(n, 8) * EPS)  # (the forward bound of a sum of n terms)
    logz, err = s.log_evidence_stepping_stone(burn_in_fraction=None)
    assert logz == pytest.approx(-1234.56789, rel=1e-14) and err == pytest.approx(math.sqrt((T - 1) / n), rel=1e-15)


@pytest.mark.gpu
def test_evidence_propagates_non_finite_values_as_the_reference(hip_engine, evidence_rows):
    """-inf in the hottest rung, a NaN, +inf: the device path returns what the host path (the reference's arithmetic) returns."""
    from aspire_amd import PTMCMCSamples

    eng = hip_engine
    T, S, W = 3, 300, 7
    betas = [1.0, 0.3, 0.0]
    base = evidence_rows[:T, :S * W].reshape(T, S, W)
    for value, rung in ((-np.inf, 2), (np.nan, 1), (np.inf, 2), (-np.inf, 1)):
        ll = base.copy()
        ll[rung, 100, 3] = value
        dev = PTMCMCSamples.from_chain(chain=torch.zeros((T, S, W, 1), dtype=torch.float64, device=eng.device), betas=betas,
                                       log_likelihood=torch.as_tensor(ll, device=eng.device), xp=torch, engine=eng)
        host = PTMCMCSamples.from_chain(chain=np.zeros((T, S, W, 1)), betas=betas, log_likelihood=ll)
        with np.errstate(invalid="ignore"):
            for fn, kw in (("log_evidence_thermodynamic_integration", dict(method="variance")),
                           ("log_evidence_thermodynamic_integration", dict(method="coarse")), ("log_evidence_stepping_stone", {})):
                a, b = getattr(dev, fn)(**kw), getattr(host, fn)(**kw)
                np.testing.assert_allclose(a, b, rtol=S * W * EPS * 8, atol=0, equal_nan=True, err_msg=f"{value} {rung} {fn}")
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))


# ---- the sampler end to end -----------------------------------------------------------------------------------------------------
W_E2E, STEPS, RUNGS = 256, 300, 6


def scalar_tolerances(ll, betas, n):
    """Device evidence against the host path on the same chain: both sum n terms per rung in different orders.  TI: n eps sum_r c_r
    mean |ll_r|; its error and the stepping stone (a log of a sum of positive terms, T - 1 of them): n eps relative."""
    c = pt_ref.trapezoid_coefficients(betas)[0]
    return n * EPS * float(np.sum(c * np.mean(np.abs(ll.reshape(len(betas), -1)), axis=1))), (len(betas) - 1) * n * EPS


def aspire_for(eng, callables):
    """Built-in densities in numpy's namespace, or torch callables behind prior bounds (a box of six prior standard deviations:
    the closed form does not notice it)."""
    from aspire_amd import Aspire, Samples

    lik, pri = gaussian_targets()
    names = [f"x_{i}" for i in range(pt_ref.GAUSS_D)]

    def torch_lik(samples):
        assert isinstance(samples.x, torch.Tensor)
        return lik(samples)

    if callables:
        a = Aspire(log_likelihood=torch_lik, log_prior=lambda smp: pri(smp), dims=pt_ref.GAUSS_D, flow_backend="gaussian", xp=torch,
                   device="cuda", parameters=names, prior_bounds={n: [-12, 12] for n in names}, engine=eng, seed=5)
    else:
        a = Aspire(log_likelihood=lik, log_prior=pri, dims=pt_ref.GAUSS_D, flow_backend="gaussian", xp=np, parameters=names, engine=eng,
                   seed=5)
    a.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, pt_ref.GAUSS_D)), parameters=names, xp=np))
    return a


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.mark.gpu
@pytest.mark.parametrize("callables", [False, True], ids=["mixtures", "callables-bounded"])
def test_sampler_end_to_end(hip_engine, callables):
    """The statistical check of tests/test_pt_sampler.py at 256 walkers, 300 steps, half discarded, through the facade; the device
    evidence against the container's host path on the same chain."""
    from aspire_amd import PTMCMCSamples

    a = aspire_for(hip_engine, callables)
    extra = dict(preconditioning_kwargs={"bounded_to_unbounded": True}) if callables else {}
    out = a.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=hip_engine, rng=np.random.default_rng(3), n_walkers=W_E2E,
                             n_temps=RUNGS, n_steps=STEPS, **extra)
    s = a.sampler
    assert isinstance(out, PTMCMCSamples) and out.chain_shape == (RUNGS, STEPS, W_E2E)
    assert ("asmc_pcn_split" if callables else "asmc_pcn_mutate") in s.last_mutation_path
    assert ("preconditioned" in s.last_mutation_path) == callables
    betas, ll = host(out.betas), host(out.log_likelihood).reshape(out.chain_shape)
    lik, pri = gaussian_targets()
    np.testing.assert_allclose(ll.reshape(-1), lik(host(out.x)), rtol=1e-11, atol=1e-10)  # the densities belong to the recorded rows
    np.testing.assert_allclose(host(out.log_prior), pri(host(out.x)), rtol=1e-11, atol=1e-10)
    mean_ll, logz = gaussian_closed_form(pt_ref.GAUSS_M, pt_ref.GAUSS_SP2, pt_ref.GAUSS_SL2, betas)
    z_mean, z_ti, z_ss = pt_z_scores(ll[:, STEPS // 2:], betas, mean_ll, logz)
    print("callables" if callables else "mixtures", "z(rung means)", np.round(z_mean, 2), "z(TI)", round(z_ti, 2), "z(SS)", round(z_ss, 2),
          "acceptance", np.round(s.rung_acceptance, 2), "swaps", np.round(s.swap_acceptance, 2), s.evidence, "log Z", logz)
    assert np.all(np.abs(z_mean) < 5.0) and abs(z_ti) < 5.0 and abs(z_ss) < 5.0
    assert np.all(s.swap_acceptance > 0.05) and s.swap_acceptance.shape == (RUNGS - 1,)
    ref = PTMCMCSamples.from_chain(chain=host(out.chain), betas=betas, log_likelihood=ll)
    n = (STEPS - int(STEPS * 0.1)) * W_E2E
    tol_ti, tol_rel = scalar_tolerances(ll[:, int(STEPS * 0.1):], betas, n)
    ti, ss = ref.log_evidence_thermodynamic_integration(), ref.log_evidence_stepping_stone()
    got_ti, got_ss = s.evidence["thermodynamic_integration"], s.evidence["stepping_stone"]
    print("device - host: TI", got_ti[0] - ti[0], got_ti[1] - ti[1], "SS", got_ss[0] - ss[0], got_ss[1] - ss[1], "bounds", tol_ti, tol_rel)
    assert abs(got_ti[0] - ti[0]) <= tol_ti and abs(got_ti[1] - ti[1]) <= tol_rel * ti[1] + tol_ti / math.sqrt(n)
    assert abs(got_ss[0] - ss[0]) <= tol_rel and abs(got_ss[1] - ss[1]) <= tol_rel * ss[1]


@pytest.mark.gpu
def test_without_exchange_a_rung_is_the_minipcn_chain_of_its_rows(hip_engine):
    """swap_every = 0: rung r's block of the chain is bit-identical to `HipMiniPCN`-style calls (chain_set, pcn_mutate) on that
    rung's rows alone at beta_r, gid0 = r W."""
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    eng = hip_engine
    W, steps, T = 257, 6, 3
    lik, pri = gaussian_targets()
    s = HipPTMiniPCN(log_likelihood=lik, log_prior=pri, dims=pt_ref.GAUSS_D, prior_flow=GaussianFlow(pt_ref.GAUSS_D, sigma=1.5, engine=eng, seed=9),
                     xp=np, engine=eng, rng=np.random.default_rng(4))
    first, inner = {}, eng.pcn_mutate

    def spy(x, ll, lp, lq, beta, mu, L, Linv, *a, **k):
        first.setdefault(a[4], (x.clone(), ll.clone(), lp.clone(), lq.clone(), beta, mu.clone(), L.clone(), Linv.clone(), a, k))
        return inner(x, ll, lp, lq, beta, mu, L, Linv, *a, **k)

    eng.pcn_mutate = spy
    try:
        out = s.sample(n_walkers=W, n_temps=T, n_steps=steps, swap_every=0)
    finally:
        del eng.pcn_mutate
    assert sorted(first) == [0, W, 2 * W] and np.all(s.swap_acceptance == 0)
    for r in range(T):
        x, ll, lp, lq, beta, mu, L, Linv, a, k = first[r * W]
        assert beta == out.betas[r]
        alone = eng.chain_alloc(steps, W, pt_ref.GAUSS_D)
        eng.chain_set(alone, 0, 1)
        try:
            eng.pcn_mutate(x, ll, lp, lq, beta, mu, L, Linv, *a, **k)
        finally:
            eng.chain_clear()
        assert alone.x.cpu().numpy().tobytes() == np.ascontiguousarray(out.chain[r]).tobytes()
        assert alone.ll.cpu().numpy().tobytes() == np.asarray(out.log_likelihood).reshape(T, steps, W)[r].tobytes()


@pytest.mark.gpu
def test_a_likelihood_hole_does_not_stop_a_run(hip_engine):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.mcmc import HipPTMiniPCN

    eng = hip_engine
    lik, pri = gaussian_targets()
    centre = torch.as_tensor(pt_ref.GAUSS_M, device=eng.device)

    def holed(samples):
        r = (samples.x - centre).norm(dim=1)
        return torch.where(r < 0.4, torch.full_like(r, float("-inf")), lik(samples))

    s = HipPTMiniPCN(log_likelihood=holed, log_prior=lambda smp: pri(smp), dims=pt_ref.GAUSS_D,
                     prior_flow=GaussianFlow(pt_ref.GAUSS_D, sigma=1.5, engine=eng, seed=9), xp=torch, engine=eng, rng=np.random.default_rng(4))
    out = s.sample(n_walkers=258, n_temps=4, n_steps=30, burnin=10)
    ll, x = host(out.log_likelihood), host(out.x)
    assert out.chain_shape == (4, 20, 258) and np.all(np.isfinite(ll)) and np.all(np.linalg.norm(x - pt_ref.GAUSS_M, axis=1) >= 0.4)
    assert np.all(np.isfinite(s.evidence["stepping_stone"])) and s.swap_acceptance.sum() > 0
