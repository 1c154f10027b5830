"""The fused flow-proposal step's LDS image (csrc/asmc_pcn_fused.hip): a mutation call builds it once (k_fused_stage_image runs
the staging code into its own LDS and dumps it) and every step launch copies it, instead of every block of every launch staging
the weights and tables for itself.  The builder runs the code the step runs when it stages inline, so nothing may change: every
case here runs the same call twice in one process - image path, then ASMC_FUSED_STAGE=inline (read per call) - on equal inputs and
compares x, ll, lp, lq, the accept counts and the step-size history with `torch.equal` / `array_equal`.

Populations: n = 64 * 4 + 29 (fewer tiles than waves, ragged last tile) and n = 64 * 2048 + 64 * 5 + 3 (one dealt round of the
256 x 8 waves plus a remainder through the tile counter, ragged last tile).  Three steps with the step-size adaptation on.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = 64 * 4 + 29, 64 * 2048 + 64 * 5 + 3
N_STEPS = 3
COUPLING, MAF = "coupling", "maf"
# every prologue layout: (id, flow kind, dims, hidden width, layers, noise, likelihood components, ASMC_FLOW_MATH)
LAYOUTS = [
    ("w64-noise_f64", COUPLING, 32, 64, 4, "f64", 1, None),  # the headline's instantiation
    ("w64-noise_f32", COUPLING, 32, 64, 4, "f32", 1, None),
    ("w64-mix", COUPLING, 32, 64, 3, "f64", 2, None),  # the MIX instantiation
    ("w64-math_f32", COUPLING, 32, 64, 3, "f64", 1, "f32"),  # HS = false: the fp32 pack, copied
    ("w32", COUPLING, 32, 32, 3, "f64", 1, None),
    ("w128-one-layer", COUPLING, 32, 128, 1, "f64", 1, None),
    ("maf-w64", MAF, 32, 64, 2, "f64", 1, None),
    ("d20-zero-padded", COUPLING, 20, 64, 3, "f64", 1, None),  # tables zero-padded to 32 rows, d_noise = 20
]


@pytest.fixture(scope="module")
def eng():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=1 << 18, d_max=32)


_FLOWS = {}


def _flow(eng, kind, dims, n_layers, hidden, seed=5):
    key = (id(eng), kind, dims, n_layers, hidden, seed)
    if key not in _FLOWS:
        from conftest import random_coupling_flow, random_maf_flow

        flow = random_coupling_flow(dims, n_layers, hidden, seed=seed) if kind == COUPLING else random_maf_flow(dims, n_layers, hidden, seed=seed)
        _FLOWS[key] = flow.device_coupling(eng)
    return _FLOWS[key]


def _reference(eng, d, seed):
    """(mu, L, Linv) of a reference Gaussian, on the device"""
    g = np.random.default_rng(seed)
    a = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.tril(np.linalg.cholesky(0.8 * (np.eye(d) + 0.2 * a @ a.T)))
    return eng.asarray(0.05 * g.normal(size=d)), eng.asarray(L), eng.asarray(np.tril(np.linalg.inv(L)))


def _targets(eng, d, c_ll, seed):
    g = np.random.default_rng(seed)
    if c_ll == 1:
        t_ll = eng.make_mixture([0.0], 0.1 * g.normal(size=(1, d)), 0.7 + 0.6 * g.random(size=(1, d)))
    else:
        t_ll = eng.make_mixture(np.log([0.4, 0.6]), 0.5 * g.normal(size=(2, d)), 0.6 + g.random(size=(2, d)))
    return t_ll, eng.make_mixture([0.0], np.zeros((1, d)), np.ones((1, d)))


def _population(eng, n, d, dtype, dev, t_ll, t_lp, seed):
    import torch

    g = np.random.default_rng(seed)
    x = torch.as_tensor(0.9 * g.normal(size=(n, d))).to(torch.float64 if dtype == "f64" else torch.float32).to(eng.device).contiguous()
    return x, eng.mixture_logpdf(x, t_ll), eng.mixture_logpdf(x, t_lp), eng.coupling_logprob(x, dev)


def _mutate(eng, monkeypatch, stage, pop, beta, ref, t_ll, t_lp, dev, noise, seed=4242, deferred=False, profile=False):
    """one call on clones of `pop`; stage: "image" | "inline"; returns (x, ll, lp, lq, n_acc, rho_hist, rho)[, kernel table]"""
    import torch

    if stage == "inline":
        monkeypatch.setenv("ASMC_FUSED_STAGE", "inline")
    else:
        monkeypatch.delenv("ASMC_FUSED_STAGE", raising=False)
    x, ll, lp, lq = (t.clone() for t in pop)
    args = (x, ll, lp, lq, beta, *ref, t_ll, t_lp, dev, seed, 17, 0.3, N_STEPS, 9, 0.234, True, noise)
    if profile:
        eng.profile(True)
    if deferred:
        handle = eng.pcn_mutate_flow_enqueue(*args)
        eng.coupling_logprob(pop[0], dev)  # something enqueued behind the deferred call
        n_acc, rho_hist, rho = eng.pcn_mutate_flow_result(handle)
    else:
        n_acc, rho_hist, rho = eng.pcn_mutate_flow(*args)
    torch.cuda.synchronize()
    out = (x, ll, lp, lq, np.array(n_acc), np.array(rho_hist), rho)
    if profile:
        rep = eng.profile_report()
        eng.profile(False)
        return out, rep
    return out


def _assert_same(a, b, what):
    import torch

    for name, u, v in zip(("x", "ll", "lp", "lq"), a[:4], b[:4]):
        assert torch.equal(u, v), f"{what}: {name} differs"
    assert np.array_equal(a[4], b[4]), (what, a[4], b[4])
    assert np.array_equal(a[5], b[5]) and a[6] == b[6], (what, a[5], b[5])
    assert 0 < a[4].sum() < len(a[4]) * a[0].shape[0], a[4]  # (steps that moved some particles and not all: the comparison says something)


@pytest.mark.parametrize("n", [N_SMALL, N_LARGE], ids=["n285", "n131395"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[r[0] for r in LAYOUTS])
def test_image_path_equals_inline_staging(eng, monkeypatch, layout, dtype, n):
    _, kind, d, hidden, n_layers, noise, c_ll, math = layout
    if math:
        monkeypatch.setenv("ASMC_FLOW_MATH", math)
    dev = _flow(eng, kind, d, n_layers, hidden)
    ref, (t_ll, t_lp) = _reference(eng, d, 21), _targets(eng, d, c_ll, 22)
    pop = _population(eng, n, d, dtype, dev, t_ll, t_lp, 23)
    got, rep = _mutate(eng, monkeypatch, "image", pop, 0.4, ref, t_ll, t_lp, dev, noise, profile=True)
    want, rep_inline = _mutate(eng, monkeypatch, "inline", pop, 0.4, ref, t_ll, t_lp, dev, noise, profile=True)
    _assert_same(got, want, layout[0])
    # one launch per step under the step's label, exactly one builder launch per call - and none when the steps stage inline
    assert rep["k_pcn_flow_fused"][0] == N_STEPS and rep["k_fused_stage_image"][0] == 1, rep
    assert rep_inline["k_pcn_flow_fused"][0] == N_STEPS and "k_fused_stage_image" not in rep_inline, rep_inline


def test_nothing_survives_a_call(eng, monkeypatch):
    """four consecutive calls on one engine alternate two flows of one shape, two (mu, L), two beta and two target sets: each
    call's image is its own"""
    d, n = 32, N_LARGE
    flows = [_flow(eng, COUPLING, d, 4, 64, seed=s) for s in (5, 6)]
    refs = [_reference(eng, d, s) for s in (31, 32)]
    tgts = [_targets(eng, d, 1, s) for s in (33, 34)]
    betas = [0.3, 0.7]
    pops = [_population(eng, n, d, "f64", flows[k], *tgts[k], 35 + k) for k in (0, 1)]
    calls = [(k & 1) for k in range(4)]
    got = [_mutate(eng, monkeypatch, "image", pops[k], betas[k], refs[k], *tgts[k], flows[k], "f64") for k in calls]
    want = [_mutate(eng, monkeypatch, "inline", pops[k], betas[k], refs[k], *tgts[k], flows[k], "f64") for k in calls]
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_same(a, b, f"call {i}")
    import torch

    assert not torch.equal(got[0][0], got[1][0])  # (the two settings do give different chains)


def test_two_engines_interleaved(eng, monkeypatch):
    from aspire_amd.engine import HipEngine

    eng2 = HipEngine(0, n_max=1 << 12, d_max=32)
    d, n = 32, N_SMALL
    engines = [eng, eng2]
    flows = [_flow(e, COUPLING, d, 4, 64, seed=5 + k) for k, e in enumerate(engines)]
    refs = [_reference(e, d, 41 + k) for k, e in enumerate(engines)]
    tgts = [_targets(e, d, 1, 43 + k) for k, e in enumerate(engines)]
    pops = [_population(e, n, d, "f64", flows[k], *tgts[k], 45 + k) for k, e in enumerate(engines)]
    order = [0, 1, 0, 1]
    got = [_mutate(engines[k], monkeypatch, "image", pops[k], 0.4, refs[k], *tgts[k], flows[k], "f64") for k in order]
    want = [_mutate(engines[k], monkeypatch, "inline", pops[k], 0.4, refs[k], *tgts[k], flows[k], "f64") for k in order]
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_same(a, b, f"engine {order[i]}, call {i}")


@pytest.mark.parametrize("n", [N_SMALL, N_LARGE], ids=["n285", "n131395"])
def test_deferred_form_equals_blocking_call(eng, monkeypatch, n):
    d = 32
    dev = _flow(eng, COUPLING, d, 4, 64)
    ref, (t_ll, t_lp) = _reference(eng, d, 51), _targets(eng, d, 1, 52)
    pop = _population(eng, n, d, "f64", dev, t_ll, t_lp, 53)
    blocking = _mutate(eng, monkeypatch, "image", pop, 0.4, ref, t_ll, t_lp, dev, "f64")
    deferred = _mutate(eng, monkeypatch, "image", pop, 0.4, ref, t_ll, t_lp, dev, "f64", deferred=True)
    inline = _mutate(eng, monkeypatch, "inline", pop, 0.4, ref, t_ll, t_lp, dev, "f64", deferred=True)
    _assert_same(deferred, blocking, "deferred vs blocking")
    _assert_same(deferred, inline, "deferred: image vs inline")
