"""Neural spline flow on the HIP kernels (include/asmc.h ASMC_FLOW_NSF; csrc/asmc_nsf.hip): density, draw, the flow-proposal
mutation loop and a whole SMC run.

The reference asks zuko for the class (`examples/smc_example.py:82` of the reference, `flow_class="NSF"`); zuko is absent, the
flow is this repository's NSFFlow.  Accuracy is judged against the SAME fp32 parameters evaluated in fp64 (`log_prob_f64`) with
error |got - ref| / max(|ref|, 1).  No fp32 evaluation of a spline reaches the 1e-6 bar of the affine flows (knot positions carry
fp32 rounding into bins whose log J has curvature up to 1e4), so the yardstick is the fp32 torch module itself on the same rows:
the kernel's maximum and 99th-percentile error must each be within 4 times the module's (split-fp16 operands carry 22 mantissa
bits against fp32's 24; the hardware exp / log / rcp / sqrt add about an ulp each), and the module's own maximum error is capped
first (1e-5 at weight scale 0.3, 1e-3 at weight scale 1.0) so that the yardstick cannot hide a failure.
"""
import copy
import math

import numpy as np
import pytest
import torch

import nsf_ref
import pcn_ref as P

pytestmark = pytest.mark.gpu

MARGIN = 4.0


@pytest.fixture(scope="module")
def eng():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=1 << 18, d_max=32)


def _err(got, ref):
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)


def _within_margin(kernel_err, module_err, what):
    print(f"{what}: module max {module_err.max():.3g} p99 {np.percentile(module_err, 99):.3g} | "
          f"kernel max {kernel_err.max():.3g} p99 {np.percentile(kernel_err, 99):.3g}")
    assert kernel_err.max() <= MARGIN * module_err.max(), (what, kernel_err.max(), module_err.max())
    assert np.percentile(kernel_err, 99) <= MARGIN * np.percentile(module_err, 99), (what, np.percentile(kernel_err, 99),
                                                                                     np.percentile(module_err, 99))


DENSITY_CASES = [(32, 3, 64, 4097, torch.float64, 1.0), (32, 3, 64, 1000, torch.float32, 0.3), (32, 1, 32, 1, torch.float64, 0.3),
                 (5, 2, 32, 1000, torch.float64, 0.3), (16, 3, 64, 17, torch.float64, 0.3), (17, 2, 64, 2500, torch.float64, 0.3),
                 (1, 2, 32, 100, torch.float64, 0.3),
                 (8, 2, 32, 15, torch.float64, 0.3), (8, 2, 32, 16, torch.float64, 0.3), (8, 2, 32, 17, torch.float64, 0.3)]  # group edges


def _density_rows(flow, n, d):
    """loc + 1.5 scale N(0, I); from 100 rows on, planted rows: single coordinates at +-B and beyond (standardised units), one NaN
    row, one row scaled by 1e6.  Returns (rows, indices of the rows that must come back NaN)."""
    g = np.random.default_rng(5)
    loc, scale = flow.loc.double().numpy(), flow.scale.double().numpy()
    x = loc + 1.5 * scale * g.normal(size=(n, d))
    nan_rows = []
    if n >= 100:
        for i, u in enumerate((5.0, -5.0, 5.0 + 1e-6, -5.0 - 1e-6, 7.0, -7.0)):
            j = i % d
            x[i, j] = loc[j] + scale[j] * u
        x[6, (d - 1) // 2] = np.nan
        x[7] *= 1e6
        nan_rows = [6, 7]
    return x, nan_rows


@pytest.mark.parametrize("d,n_tr,hidden,n,dtype,wscale", DENSITY_CASES)
def test_nsf_logprob_vs_fp64_within_four_times_the_fp32_module(eng, d, n_tr, hidden, n, dtype, wscale):
    flow = nsf_ref.random_nsf_flow(d, n_tr, hidden, seed=3, scale=wscale)
    dev = flow.device_coupling(eng)
    assert dev.kind == 2 and dev.bins == 8 and eng.lib.asmc_flow_layout(2, d, hidden) == 2
    x, nan_rows = _density_rows(flow, n, d)
    xd = torch.as_tensor(x, device=eng.device).to(dtype).contiguous()
    got = eng.coupling_logprob(xd, dev).cpu().numpy()
    xr = xd.double().cpu()
    keep = np.setdiff1d(np.arange(n), nan_rows)
    assert np.all(np.isnan(got[nan_rows])) and np.all(np.isfinite(got[keep]))
    ref = flow.log_prob_f64(xr[keep]).numpy()
    module = flow.log_prob(xr[keep].float() if dtype == torch.float32 else xr[keep]).double().numpy()
    e_mod, e_ker = _err(module, ref), _err(got[keep], ref)
    assert e_mod.max() <= (1e-3 if wscale == 1.0 else 1e-5), e_mod.max()  # the yardstick's own cap
    _within_margin(e_ker, e_mod, f"density d={d} T={n_tr} h={hidden} n={n}")


def _f32_rounding_shift(flow, x):
    """First-order bound on what rounding every coordinate of x to float32 moves log q by: sum_j |d log q / d x_j| |x_j| 2^-24."""
    layers = copy.deepcopy(flow.layers).to(torch.float64)
    with torch.enable_grad():
        xx = x.detach().double().cpu().clone().requires_grad_(True)
        z = (xx - flow.loc.double().cpu()) / flow.scale.double().cpu()
        ladj = 0.0
        for layer in layers:
            z, lj = layer(z)
            ladj = ladj + lj
        lq = (-0.5 * (z * z).sum(-1) + ladj).sum()
        (grad,) = torch.autograd.grad(lq, xx)
    return (grad.abs() * xx.detach().abs()).sum(-1).numpy() * 2.0**-24


@pytest.mark.parametrize("d,n_tr,hidden,n,dtype", [(32, 3, 64, 20000, torch.float64), (7, 2, 32, 4000, torch.float32),
                                                   (16, 3, 64, 4097, torch.float64)])
def test_nsf_sample_inverts_the_density_pass(eng, d, n_tr, hidden, n, dtype):
    """asmc_coupling_sample with kind = ASMC_FLOW_NSF: the returned log q is the density of the returned rows (fp64 evaluation of
    the same flow) within 4 times what the fp32 module's own `sample_and_log_prob` achieves on its rows; float32 rows add the
    first-order effect of rounding x after the density was formed (measured: see DESIGN 3.24); the rows pushed back through the
    flow are standard normal; a draw does not depend on sharding; another draw_id is another draw."""
    flow = nsf_ref.random_nsf_flow(d, n_tr, hidden, seed=4, scale=0.3)
    dev = flow.device_coupling(eng)
    x, lq = eng.coupling_sample(n, dtype, dev, 1234, 0, 1)
    assert torch.isfinite(x).all() and torch.isfinite(lq).all()
    on_gpu = copy.deepcopy(flow).to(eng.device)  # the fp32 torch modules (no engine attached: they draw and invert themselves)
    ref = on_gpu.log_prob_f64(x.double()).cpu().numpy()
    xm, lqm = on_gpu.sample_and_log_prob(n)
    e_mod = _err(lqm.double().cpu().numpy(), on_gpu.log_prob_f64(xm.double()).cpu().numpy())
    got = lq.cpu().numpy()
    if dtype == torch.float32:
        shift = _f32_rounding_shift(flow, x) / np.maximum(np.abs(ref), 1.0)
        print(f"float32 rows: rounding x moves log q by up to {shift.max():.3g} (relative), {shift.max() / e_mod.max():.2f} x the module's max error")
        e_ker = np.maximum(_err(got, ref) - shift, 0.0)
    else:
        e_ker = _err(got, ref)
    _within_margin(e_ker, e_mod, f"draw d={d} T={n_tr} h={hidden} n={n}")
    z, _ = flow.forward(x.float().cpu())
    z = z.double().numpy()
    assert abs(z.mean()) < 5.0 / math.sqrt(n * d) and abs(z.var() - 1.0) < 0.05, (z.mean(), z.var())
    h = n // 2  # the second shard of a two-rank run draws the rows the one-rank run has there
    x2, lq2 = eng.coupling_sample(n - h, dtype, dev, 1234, h, 1)
    assert torch.equal(x2, x[h:]) and torch.equal(lq2, lq[h:])
    x3, _ = eng.coupling_sample(n, dtype, dev, 1234, 0, 2)
    assert not torch.equal(x3, x)


@pytest.mark.parametrize("d,n_tr,hidden,n", [(32, 3, 64, 4097), (7, 2, 32, 1000)])
def test_nsf_sample_fixed_point_exit_returns_the_d_pass_bits(eng, monkeypatch, d, n_tr, hidden, n):
    """A weakly coupled flow (last layers x 0.02: the shape of a trained flow near its initialisation) leaves the inversion loop
    before its d passes; the rows and log q are the bits of the full d-pass loop (ASMC_NSF_SAMPLE_ALL_PASSES=1)."""
    from aspire_amd.flows import _MaskedLinear

    flow = nsf_ref.random_nsf_flow(d, n_tr, hidden, seed=14, scale=0.3)
    with torch.no_grad():
        for layer in flow.layers:
            last = [m for m in layer.net if isinstance(m, _MaskedLinear)][-1]
            last.weight.mul_(0.02)
    flow._version += 1
    dev = flow.device_coupling(eng)
    eng.profile(True)
    x, lq = eng.coupling_sample(n, torch.float64, dev, 77, 0, 3)
    t_exit = eng.profile_report()["k_nsf_sample"][1]
    monkeypatch.setenv("ASMC_NSF_SAMPLE_ALL_PASSES", "1")
    x2, lq2 = eng.coupling_sample(n, torch.float64, dev, 77, 0, 3)
    rep = eng.profile_report()["k_nsf_sample"]
    eng.profile(False)
    print(f"k_nsf_sample d={d}: {t_exit:.3f} ms with the exit, {2 * rep[1] - t_exit:.3f} ms with all passes")
    assert torch.equal(x, x2) and torch.equal(lq, lq2) and torch.isfinite(lq).all()


@pytest.mark.parametrize("d,n,n_steps,whitened", [(8, 2048, 1, True), (8, 2048, 3, True), (5, 1000, 1, False)])
def test_nsf_mutation_vs_the_host_restatement(eng, d, n, n_steps, whitened):
    """asmc_pcn_mutate_flow with a spline proposal density: the un-padded step loop - register-resident whitened state at d = 8
    (propose, k_nsf_logprob, accept), the x-state loop at d = 5 - against tests/pcn_ref.py's propose + accept fed with
    `log_prob_f64` of the proposals.  Rows whose decision the restatement cannot call within (1 - beta) x the density bound are
    skipped and must stay within razor_cap(n); every other row agrees in position and in the carried densities."""
    beta, rho, seed, gid0, step0 = 0.37, 0.4, 4242, 17, 9
    flow = nsf_ref.random_nsf_flow(d, 2, 32, seed=6, scale=0.3)
    dev = flow.device_coupling(eng)
    x0, ll0, lp0, _, mu, L, Linv, mixes = P.problem(n, d, seed=8)
    t_ll, t_lp = (eng.make_mixture(*m) for m in mixes[:2])
    xd = eng.asarray(x0)
    lld, lpd, lqd = eng.asarray(ll0), eng.asarray(lp0), eng.coupling_logprob(xd, dev)
    eng.profile(True)
    n_acc, _, _ = eng.pcn_mutate_flow(xd, lld, lpd, lqd, beta, eng.asarray(mu), eng.asarray(L), eng.asarray(Linv), t_ll, t_lp, dev,
                                      seed, gid0, rho, n_steps, step0, 0.234, False, "f64", 0.0)
    rep = eng.profile_report()
    eng.profile(False)
    print(f"mutation d={d}: kernels {sorted(rep)}")
    assert rep["k_nsf_logprob"][0] == n_steps and "k_pcn_flow_fused" not in rep, sorted(rep)
    if whitened:  # the register-resident loop
        assert rep["k_pcn_flow_propose"][0] == rep["k_pcn_flow_accept"][0] == n_steps, sorted(rep)
    else:  # the x-state loop: the split path's kernels
        assert rep["k_pcn_accept_flags"][0] == n_steps and "k_pcn_flow_propose" not in rep, sorted(rep)
    # the restatement: whitened state kept between the steps on the register path, x-state otherwise
    f64 = lambda v: flow.log_prob_f64(torch.as_tensor(v)).numpy()  # noqa: E731
    x, ll, lp, lq = x0.copy(), ll0.copy(), lp0.copy(), f64(x0)
    y = (x - mu) @ np.tril(Linv).T if whitened else None
    margins, counts = [], []
    dens_err = MARGIN * float(np.abs(flow.log_prob(torch.as_tensor(x0)).double().numpy() - lq).max())  # (the carried log q of the start rows)
    for t in range(n_steps):
        p = P.propose(None if whitened else x, mu, L, Linv, rho, seed, gid0, step0 + t, y=y)
        nll, nlp, nlq = P.mix_logpdf(mixes[0], p["x1"]), P.mix_logpdf(mixes[1], p["x1"]), f64(p["x1"])
        # the density bound on these very proposals: 4 x the fp32 module's error, in absolute terms
        mod = flow.log_prob(torch.as_tensor(p["x1"])).double().numpy()
        dens_err = max(dens_err, MARGIN * float(np.abs(mod - nlq).max()))
        P.accept(p, ll, lp, lq, nll, nlp, nlq, beta, 0.0, d)
        acc = p["accept"]
        if whitened:
            y = np.where(acc[:, None], p["y1"], y)
        x = np.where(acc[:, None], p["x1"], x)
        ll, lp, lq = np.where(acc, nll, ll), np.where(acc, nlp, lp), np.where(acc, nlq, lq)
        margins.append(p["margin"])
        counts.append(int(acc.sum()))
    if whitened:
        x = mu + y @ np.tril(L).T
    tol_m = (1.0 - beta) * dens_err
    got = dict(x=xd.cpu().numpy(), ll=lld.cpu().numpy(), lp=lpd.cpu().numpy(), lq=lqd.cpu().numpy())
    tol_c = max(dens_err, 1e-9)  # (relative to 1 + |value| >= 1: no tighter than the absolute bound)
    und = P.compare(got, dict(x=x, ll=ll, lp=lp, lq=lq), np.array(margins), 1e-9, tol_c, tol_m, label=f"nsf d={d} steps={n_steps}")
    print(f"mutation d={d} steps={n_steps}: density bound {dens_err:.3g}, razor band {tol_m:.3g}, undecided rows {und}")
    assert np.all(np.abs(np.array(n_acc) - np.array(counts)) <= max(und, 0)) and 0.05 < np.mean(n_acc) / n < 0.95, (n_acc, counts)
    # the carried log q is the kernel's density of the rows the particles ended on
    torch.testing.assert_close(lqd, eng.coupling_logprob(xd, dev), rtol=1e-5, atol=1e-3)


def test_smc_run_with_a_spline_flow_stays_on_the_device(eng):
    """`Aspire(flow_backend="nsf")`-style run at d = 16: trained NSFFlow as the proposal, the initial draw in k_nsf_sample, every
    mutation step propose / k_nsf_logprob / accept on the device - no torch op in the mutation loop, none of the x-state halves -
    and log Z within 3 sigma of the closed form."""
    from aspire_amd.flows import NSFFlow
    from aspire_amd.samplers.smc import HipSMC
    from aspire_amd.targets import DiagGaussianMixture

    d, n, n_steps = 16, 100_000, 8
    flow = NSFFlow(d, n_transforms=3, hidden_features=(64, 64), seed=7, device=eng.device, dtype=torch.float32)
    flow.fit(1.5 * 0.9 * np.random.default_rng(3).normal(size=(8000, d)), n_epochs=6)
    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    sp = HipSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=flow, xp=np, engine=eng, rng=np.random.default_rng(11),
                dtype="float64")
    eng.profile(True)
    out = sp.sample(n, sampler_kwargs=dict(n_steps=n_steps, step_fn="pcn"), store_sample_history=False)
    rep = eng.profile_report()
    eng.profile(False)
    temps = len(sp.history.beta)
    print(f"smc run: {temps} temperatures, k_nsf_logprob x {rep.get('k_nsf_logprob')}, k_nsf_sample x {rep.get('k_nsf_sample')}")
    assert "flow: device-side step loop" in sp.last_mutation_path, sp.last_mutation_path
    assert rep["k_nsf_sample"][0] >= 1
    extra = rep["k_nsf_logprob"][0] - n_steps * temps  # (beyond the steps: an initial evaluation, if any - the draw returns its own log q)
    assert 0 <= extra <= 1, (rep["k_nsf_logprob"][0], n_steps, temps)
    assert rep["k_pcn_flow_propose"][0] == rep["k_pcn_flow_accept"][0] == n_steps * temps
    for name in rep:
        assert not name.startswith(("k_pcn_propose", "k_pcn_accept", "k_pcn_flow_fused", "k_copy_flagged_rows")), name
    z = (float(out.log_evidence) - 0.5 * d * math.log(math.pi)) / float(out.log_evidence_error)
    assert abs(z) < 3.0, z
