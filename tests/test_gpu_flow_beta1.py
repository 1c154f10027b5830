"""asmc_pcn_mutate_flow at beta = 1 exactly: the fused steps run without the flow density and one refresh of log q follows them
(csrc/asmc_pcn_fused.hip: FUSED_MODE_NQ, FUSED_MODE_LQ).  The tempered target there is 0 * lq + (ll + lp), so no accept decision can
read log q, and the refresh evaluates the stored y with the step's own code: every result equals the full step's, bit for bit.

Each case runs the same call twice in one process - the default path and ASMC_FLOW_BETA1=full (the full step at beta = 1, what the
parent commit ran) - and asserts equality of x, ll, lp, lq, the accept counts, the step-size history and the final step size.
A NaN compares unequal to itself, so arrays that may carry one (poisoned rows) are compared as NaN pattern plus values elsewhere.

Inputs as in tools/record_mutation_census.py (n = 193: three full 64-row tiles plus one row; 5 steps; adaptation on)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import random_coupling_flow, random_maf_flow

pytestmark = pytest.mark.gpu

N, STEPS, STEP0, RHO, SEED, GID0 = 193, 5, 7, 0.3, 4242, 17
NQ, LQ, FULL = "k_pcn_flow_fused_nq", "k_pcn_flow_fused_lq", "16k_pcn_flow_fusedI"  # substrings of the mangled kernel symbols


@pytest.fixture(scope="module")
def eng():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=1 << 15, d_max=32)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old


_FLOWS = {}


def _flow(eng, kind, d, layers, hidden):
    key = (id(eng), kind, d, layers, hidden)
    if key not in _FLOWS:
        flow = (random_coupling_flow if kind == "coupling" else random_maf_flow)(d, layers, hidden)
        _FLOWS[key] = (flow, flow.device_coupling(eng))
    return _FLOWS[key][1]


def _inputs(eng, d, T, n, mix):
    g = np.random.default_rng(1000 + d)
    x = torch.as_tensor(0.9 * g.normal(size=(n, d))).to(torch.float64 if T == "f64" else torch.float32).to(eng.device).contiguous()
    a = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.tril(np.linalg.cholesky(0.8 * (np.eye(d) + 0.2 * a @ a.T)))
    mu, Linv = 0.05 * g.normal(size=d), np.tril(np.linalg.inv(L))
    if mix:  # a two-component likelihood
        t_ll = eng.make_mixture(np.log([0.4, 0.6]), 0.3 * g.normal(size=(2, d)), 0.7 + 0.6 * g.random(size=(2, d)))
    else:
        t_ll = eng.make_mixture([0.0], 0.1 * g.normal(size=(1, d)), 0.7 + 0.6 * g.random(size=(1, d)))
    t_lp = eng.make_mixture([0.0], np.zeros((1, d)), np.ones((1, d)))
    return x, eng.asarray(mu), eng.asarray(L), eng.asarray(Linv), t_ll, t_lp


def run(eng, full, *, beta=1.0, d=32, T="f64", kind="coupling", layers=4, hidden=64, nu=0.0, noise="f64", mix=False, deferred=False,
        n=N, steps=STEPS, rho=RHO, adapt=True, calls=1, lq_shift=0.0, poison=0, dev=None):
    """One call (or `calls` consecutive ones) of the flow mutation; full: under ASMC_FLOW_BETA1=full."""
    x, mu, L, Linv, t_ll, t_lp = _inputs(eng, d, T, n, mix)
    ll, lp = eng.mixture_logpdf(x, t_ll), eng.mixture_logpdf(x, t_lp)
    dev = dev if dev is not None else _flow(eng, kind, d, layers, hidden)
    lq = eng.coupling_logprob(x, dev)
    if lq_shift:
        lq += lq_shift
    if poison:
        lq[7:7 + 3 * poison:3] = float("nan")
    ll0, lq0 = ll.clone(), lq.clone()
    out = {"n_acc": [], "rho_hist": []}
    with _env("ASMC_FLOW_BETA1", "full" if full else None):
        torch.cuda.synchronize()
        eng.profile(True)
        for c in range(calls):
            args = (x, ll, lp, lq, beta, mu, L, Linv, t_ll, t_lp, dev, SEED, GID0, rho, steps, STEP0 + c * steps, 0.234, adapt, noise, nu)
            if deferred:
                n_acc, rho_hist, rho = eng.pcn_mutate_flow_result(eng.pcn_mutate_flow_enqueue(*args))
            else:
                n_acc, rho_hist, rho = eng.pcn_mutate_flow(*args)
            out["n_acc"] += [int(v) for v in n_acc]
            out["rho_hist"] += [float(v) for v in rho_hist]
        out["report"] = {k: v[0] for k, v in eng.profile_report().items()}
        out["variants"] = eng.profile_variants()
        eng.profile(False)
    torch.cuda.synchronize()
    out.update(x=x, ll=ll, lp=lp, lq=lq, rho=float(rho), ll0=ll0, lq0=lq0, lq_nan=eng.pcn_lq_nan(), bad=eng.pcn_flow_nonfinite(), dev=dev)
    return out


def _equal(a, b):
    if not (torch.isnan(a).any() or torch.isnan(b).any()):
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _count(variants, sub):
    return sum(v for k, v in variants.items() if sub in k)


def check_same(fast, full, steps):
    """the default path ran the two new kernels, the override the parent's; every result is equal"""
    print(fast["report"], fast["n_acc"], fast["rho"], "| full:", full["report"], full["n_acc"], full["rho"])
    assert fast["report"].get("k_pcn_flow_fused") == steps and _count(fast["variants"], NQ) == steps and _count(fast["variants"], FULL) == 0
    assert full["report"].get("k_pcn_flow_fused") == steps and _count(full["variants"], FULL) == steps
    assert _count(full["variants"], NQ) == 0 and "k_fused_lq_refresh" not in full["report"]
    for key in ("x", "ll", "lp", "lq"):
        assert _equal(fast[key], full[key]), key
    assert fast["n_acc"] == full["n_acc"] and sum(fast["n_acc"]) > 0
    assert fast["rho_hist"] == full["rho_hist"] and fast["rho"] == full["rho"]
    assert fast["lq_nan"] == full["lq_nan"] and fast["bad"] == full["bad"] == 0


VARIANTS = {
    "base-f64": {},
    "base-f32": dict(T="f32"),
    "padded-d6": dict(d=6),
    "padded-d6-f32": dict(d=6, T="f32"),
    "maf-w64": dict(kind="maf", layers=3, hidden=64),
    "coupling-w32": dict(hidden=32),
    "tpcn-nu5.5": dict(nu=5.5),
    "mixture-likelihood": dict(mix=True),
    "noise-f32": dict(noise="f32"),
    "deferred": dict(deferred=True),
    "two-calls": dict(calls=2),
    "n-20000": dict(n=20000),
}


@pytest.mark.parametrize("name", VARIANTS)
def test_beta1_equals_the_full_step(eng, name):
    kw = VARIANTS[name]
    steps = STEPS * kw.get("calls", 1)
    fast, full = run(eng, False, **kw), run(eng, True, **kw)
    check_same(fast, full, steps)
    assert fast["report"].get("k_fused_lq_refresh") == kw.get("calls", 1)


def test_beta1_on_a_second_engine(eng):
    from aspire_amd.engine import HipEngine

    eng2 = HipEngine(0, n_max=1 << 10, d_max=32)
    fast2, full = run(eng2, False), run(eng, True)
    check_same(fast2, full, STEPS)


def test_rows_that_never_move_keep_the_log_q_they_came_with(eng):
    """The incoming lq is deliberately NOT the flow's (1e-3 added): a row that never moved keeps it bit for bit, a row that moved
    carries the density of where it is - as in the full step.  (Bound on `the density of where it is`: the stand-alone density
    kernel reaches x through the un-whitening's other operation order, both are fp32 flows of |log q| ~ 1e2, i.e. a few 1e-5
    apart at the most; half the shift, 5e-4, separates the two readings.)"""
    kw = dict(n=20000, steps=2, rho=0.02, adapt=False, lq_shift=1e-3)
    fast, full = run(eng, False, **kw), run(eng, True, **kw)
    check_same(fast, full, 2)
    stayed = full["ll"] == full["ll0"]  # (ll is written by an accepting lane only; x itself goes through whiten / un-whiten)
    print("rows that never moved:", int(stayed.sum()), "of", kw["n"])
    assert torch.equal(fast["lq"][stayed], fast["lq0"][stayed])
    true_lq = eng.coupling_logprob(fast["x"], fast["dev"])
    err = (fast["lq"][~stayed] - true_lq[~stayed]).abs().max().item()
    print("moved rows: max |lq - log q(x)| =", err)
    assert int((~stayed).sum()) > 0 and err < 5e-4


def test_poisoned_rows_lose_their_nan_as_in_the_full_step(eng):
    """37 rows arrive with lq = NaN (log_p_t = -inf): they take their first proposal and carry a finite log q from then on"""
    fast, full = run(eng, False, poison=37), run(eng, True, poison=37)
    assert int(torch.isnan(fast["lq0"]).sum()) == 37
    check_same(fast, full, STEPS)
    assert fast["lq_nan"] == eng.count_nonfinite(fast["lq"])[0] == int(torch.isnan(fast["lq"]).sum())


@pytest.mark.parametrize("beta", [float(np.nextafter(1.0, 0.0)), 0.5])
def test_any_other_beta_takes_the_full_step(eng, beta):
    a, b = run(eng, False, beta=beta), run(eng, True, beta=beta)
    print(a["report"], a["variants"])
    assert a["report"] == b["report"] and a["variants"] == b["variants"]
    assert a["report"]["k_pcn_flow_fused"] == STEPS and _count(a["variants"], FULL) == STEPS
    assert _count(a["variants"], NQ) == 0 and _count(a["variants"], LQ) == 0
    assert "k_fused_lq_refresh" not in a["report"] and "k_coupling_logprob" not in a["report"]
    for key in ("x", "ll", "lp", "lq"):
        assert torch.equal(a[key], b[key]), key


def test_launches_at_beta1(eng):
    fast, full, below = run(eng, False), run(eng, True), run(eng, False, beta=float(np.nextafter(1.0, 0.0)))
    print(fast["report"], fast["variants"])
    assert fast["report"]["k_pcn_flow_fused"] == STEPS and _count(fast["variants"], NQ) == STEPS
    assert fast["report"]["k_fused_lq_refresh"] == 1 and _count(fast["variants"], LQ) == 1
    assert "k_coupling_logprob" not in fast["report"]
    # the override launches what the parent launched: the census of a call just below beta = 1
    assert full["report"] == below["report"] and full["variants"] == below["variants"]
    extra = dict(fast["report"])
    del extra["k_fused_lq_refresh"]
    assert extra == full["report"]


def test_no_refresh_compiled_for_the_fp32_chain(eng, monkeypatch):
    """ASMC_FLOW_MATH=f32: the fp32-MFMA layers have no refresh instantiation - the full step serves beta = 1"""
    monkeypatch.setenv("ASMC_FLOW_MATH", "f32")
    a, b = run(eng, False), run(eng, True)
    print(a["report"])
    assert a["report"] == b["report"] and a["variants"] == b["variants"]
    assert a["report"]["k_pcn_flow_fused"] == STEPS and _count(a["variants"], NQ) == 0 and "k_fused_lq_refresh" not in a["report"]


def test_out_of_range_flow_at_beta1_is_counted_not_rejected(eng):
    """The flow of test_gpu_parity.py::test_fused_flow_step_reports_non_finite_flow_densities (hidden activations beyond the fp16
    operand range: NaN densities by arithmetic).  At beta = 1 the density is not looked at: such proposals are accepted or rejected
    on the targets alone, the refresh finds their log q non-finite, counts it and stores the NaN, and the call's census of the
    carried log q reports it."""
    d, n = 32, 20000
    flow = random_coupling_flow(d, 4, 64)
    with torch.no_grad():
        lin = [m for m in flow.layers[0].net if isinstance(m, torch.nn.Linear)]
        lin[0].weight.mul_(1e5)
        lin[1].weight.mul_(1e-5)
    flow._version += 1
    dev = flow.device_coupling(eng)
    out = run(eng, False, n=n, steps=2, adapt=False, dev=dev)
    print(out["report"], out["n_acc"], "nonfinite", out["bad"], "lq NaN", out["lq_nan"])
    assert out["report"]["k_fused_lq_refresh"] == 1
    assert out["bad"] > 0 and out["lq_nan"] > 0 and sum(out["n_acc"]) > 0
    assert out["lq_nan"] == int(torch.isnan(out["lq"]).sum())
    assert bool(torch.isfinite(out["x"]).all()) and bool(torch.isfinite(out["ll"]).all())
