"""The rung-batched entry points on the HIP engine (include/asmc.h asmc_pt_pack / _steps / _ladder_adapt):
the steps of every rung against `asmc_pcn_mutate` on that rung's rows - existing code, which runs calls of fewer than 4 steps on x
itself, the same kernel body -, the recorder, the number of launches, the ladder kernel against its numpy restatement
(tests/pt_batch_ref.py), and the sampler end to end.
"""
import numpy as np
import pytest
import torch

import pt_ref
from pt_batch_ref import ladder_update_ref
from test_gpu_pt import aspire_for, host
from test_pt_batched import UNEVEN, uneven_check

EPS = np.finfo(np.float64).eps
SENTINEL = -777.0
# (T, W, step_fn, components): every T of 1, 2, 3, 5 and every W of 1, 64, 65, 257 (one tile, its edge, one 256-walker block, its edge)
# with both steps and both mixtures
CASES = [(1, 257, "pcn", 1), (2, 64, "tpcn", 3), (3, 65, "tpcn", 1), (5, 1, "pcn", 3), (5, 257, "tpcn", 3), (2, 1, "tpcn", 1), (3, 64, "pcn", 3),
         (1, 65, "tpcn", 1)]


def guarded(eng, a, dtype=torch.float64, guard=3):
    """`a` on the device with `guard` rows of a sentinel behind it: (buffer, view)."""
    a = np.asarray(a)
    buf = torch.full((a.shape[0] + guard, *a.shape[1:]), SENTINEL, dtype=dtype, device=eng.device)
    buf[:a.shape[0]].copy_(torch.as_tensor(a).to(dtype))
    return buf, buf[:a.shape[0]]


def problem(eng, T, W, d, dtype, step_fn, comps, seed=0):
    """A tempered state with a reference, nu, step size and beta of its own per rung; the betas include 1 and 0.  With tpCN and three
    rungs or more, rung 1 has a Gaussian reference (nu = 0), as a Student-t fit above NU_GAUSSIAN gives."""
    g = np.random.default_rng([seed, T, W, d, comps])
    n = T * W
    mix = lambda scale: eng.make_mixture(np.log(np.full(comps, 1.0 / comps)), scale * g.normal(size=(comps, d)),  # noqa: E731
                                         g.uniform(0.5, 2.0, size=(comps, d)))
    t_ll, t_lp, t_lq = mix(1.0), mix(0.3), mix(0.3)
    refs = []
    for r in range(T):
        L = np.tril(0.2 * g.normal(size=(d, d)), -1) + np.diag(g.uniform(0.7, 1.4, size=d))
        nu = 0.0 if step_fn == "pcn" or (T >= 3 and r == 1) else 3.0 + 2.5 * r
        refs.append((eng.asarray(0.3 * g.normal(size=d)), eng.asarray(L), eng.asarray(np.linalg.inv(L)), nu))
    x = (1.2 * g.normal(size=(n, d))).astype(np.float32 if dtype == torch.float32 else np.float64)
    xb, xd = guarded(eng, x, dtype)
    dens = [guarded(eng, eng.mixture_logpdf(xd.contiguous(), m).cpu().numpy()) for m in (t_ll, t_lp, t_lq)]
    betas = np.linspace(1.0, 0.0, T) if T > 1 else np.ones(1)
    rho = 0.15 + 0.08 * np.arange(T)
    return dict(T=T, W=W, d=d, mixes=(t_ll, t_lp, t_lq), refs=refs, xb=xb, x=xd, dens=dens, betas=betas, rho=rho,
                seed=int(g.integers(1, 2**63 - 1)))


def per_rung(eng, p, state, n_steps, step0, adapt, rho):
    """`asmc_pcn_mutate` on clones of every rung's rows: (x, ll, lp, lq [T W], rho [T], accepted [T])."""
    T, W = p["T"], p["W"]
    out = [v.clone() for v in state]
    rho_out, acc = np.zeros(T), np.zeros(T, dtype=np.int64)
    for r in range(T):
        sl = slice(r * W, (r + 1) * W)
        rows = [v[sl].clone() for v in out]  # (their own allocations: 16-byte aligned, as the register kernels want)
        mu, L, Linv, nu = p["refs"][r]
        n_acc, _, rho_out[r] = eng.pcn_mutate(*rows, float(p["betas"][r]), mu, L, Linv, *p["mixes"], p["seed"], r * W, float(rho[r]), n_steps, step0,
                                              0.234, adapt, "f64", nu)
        acc[r] = n_acc.sum()
        for v, w in zip(out, rows):
            v[sl].copy_(w)
    return out, rho_out, acc


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [4, 8, 16, 32])
def test_steps_equal_the_per_rung_entry_point(hip_engine, d, dtype):
    eng = hip_engine
    for T, W, step_fn, comps in CASES:
        p = problem(eng, T, W, d, dtype, step_fn, comps)
        what = (T, W, d, dtype, step_fn, comps)
        assert eng.pt_steps_supported(p["x"])
        start = [p["x"].clone()] + [v.clone() for _, v in p["dens"]]
        betas_d = eng.asarray(p["betas"])

        def batched(n_steps, adapt):
            for v, s in zip([p["x"]] + [v for _, v in p["dens"]], start):
                v.copy_(s)
            rb, rho_d = guarded(eng, p["rho"])
            ab, acc_d = guarded(eng, np.full(T, 5, dtype=np.int64), torch.int64)
            pack = eng.pt_pack(p["x"], T, p["refs"], *p["mixes"])
            eng.pt_steps(pack, p["x"], *[v for _, v in p["dens"]], betas_d, rho_d, acc_d, p["seed"], n_steps, 0, 0.234, adapt)
            bufs = [p["xb"]] + [b for b, _ in p["dens"]]
            for b in bufs:  # the guard rows behind the state and its scalars
                assert torch.all(b[T * W:] == SENTINEL), what
            assert torch.all(rb[T:] == SENTINEL) and torch.all(ab[T:] == int(SENTINEL)), what
            return [p["x"]] + [v for _, v in p["dens"]], rho_d, acc_d

        for n_steps in (1, 2, 3):  # adaptation on: state, densities, final step sizes and counts
            want, rho_w, acc_w = per_rung(eng, p, start, n_steps, 0, True, p["rho"])
            got, rho_g, acc_g = batched(n_steps, True)
            for a, b in zip(got, want):
                assert same(a, b), (what, n_steps)
            assert rho_g.cpu().numpy().tobytes() == rho_w.tobytes() and np.array_equal(acc_g.cpu().numpy() - 5, acc_w), (what, n_steps)
            assert W < 64 or acc_w.sum() > 0, what
        want, acc_w = start, np.zeros(T, dtype=np.int64)  # adaptation off: one call of 6 steps against 6 one-step calls at step0 = t
        for t in range(6):
            want, rho_w, a = per_rung(eng, p, want, 1, t, False, p["rho"])
            acc_w += a
        got, rho_g, acc_g = batched(6, False)
        for a, b in zip(got, want):
            assert same(a, b), (what, "6 steps")
        assert rho_g.cpu().numpy().tobytes() == p["rho"].tobytes() and np.array_equal(acc_g.cpu().numpy() - 5, acc_w), what


@pytest.mark.gpu
def test_a_plain_mutation_after_a_batched_call_is_undisturbed(hip_engine):
    """The context's step-size cell, counts and variates' batch: a tpCN `pcn_mutate` of 9 steps gives the same bits before and after a
    batched tpCN call at another shape."""
    eng = hip_engine
    p = problem(eng, 1, 300, 8, torch.float64, "tpcn", 1, seed=5)
    start = [p["x"].clone()] + [v.clone() for _, v in p["dens"]]
    before = per_rung(eng, p, start, 9, 3, True, p["rho"])
    q = problem(eng, 3, 65, 16, torch.float64, "tpcn", 3, seed=6)
    pack = eng.pt_pack(q["x"], 3, q["refs"], *q["mixes"])
    eng.pt_steps(pack, q["x"], *[v for _, v in q["dens"]], eng.asarray(q["betas"]), eng.asarray(q["rho"]),
                 torch.zeros(3, dtype=torch.int64, device=eng.device), q["seed"], 5)
    after = per_rung(eng, p, start, 9, 3, True, p["rho"])
    for a, b in zip(before[0], after[0]):
        assert same(a, b)
    assert before[1].tobytes() == after[1].tobytes() and np.array_equal(before[2], after[2])


@pytest.mark.gpu
@pytest.mark.parametrize("W,d", [(1, 4), (65, 4), (1, 32), (65, 32)])
def test_recorder_keeps_every_rungs_state_after_every_step(hip_engine, W, d):
    """Slot t of rung r = the state after step t (a call of t + 1 steps from the same start); the vector path, and the element path
    through a chain that starts 8 bytes off a 16-byte boundary.  Slots of other steps stay untouched."""
    from aspire_amd.engine import DeviceChain

    eng = hip_engine
    T, S, n_steps, slot0 = 3, 5, 3, 1
    for dtype in (torch.float64, torch.float32):
        p = problem(eng, T, W, d, dtype, "tpcn", 1, seed=2)
        state = [p["x"]] + [v for _, v in p["dens"]]
        start = [v.clone() for v in state]
        betas_d = eng.asarray(p["betas"])
        for shift in (0, 8):
            item = 8 if dtype == torch.float64 else 4
            raw = torch.full((shift // item + T * S * W * d + 7,), SENTINEL, dtype=dtype, device=eng.device)
            cx = raw[shift // item: shift // item + T * S * W * d].view(T * S, W, d)
            assert cx.data_ptr() % 16 == shift
            chain = DeviceChain(cx, torch.full((T * S, W), SENTINEL, dtype=torch.float64, device=eng.device),
                                torch.full((T * S, W), SENTINEL, dtype=torch.float64, device=eng.device))
            for v, s in zip(state, start):
                v.copy_(s)
            pack = eng.pt_pack(p["x"], T, p["refs"], *p["mixes"])
            eng.pt_steps(pack, *state, betas_d, eng.asarray(p["rho"]), torch.zeros(T, dtype=torch.int64, device=eng.device), p["seed"], n_steps,
                         0, 0.234, True, chain=chain, n_slots=S, slot0=slot0)
            x4, ll3, lp3 = cx.view(T, S, W, d), chain.ll.view(T, S, W), chain.lp.view(T, S, W)
            for t in range(n_steps):
                want, _, _ = per_rung(eng, p, start, t + 1, 0, True, p["rho"])
                for r in range(T):
                    sl = slice(r * W, (r + 1) * W)
                    assert same(x4[r, slot0 + t].contiguous(), want[0][sl]) and same(ll3[r, slot0 + t].contiguous(), want[1][sl]), (dtype, shift, t, r)
                    assert same(lp3[r, slot0 + t].contiguous(), want[2][sl]), (dtype, shift, t, r)
            assert torch.all(x4[:, 0] == SENTINEL) and torch.all(x4[:, slot0 + n_steps:] == SENTINEL) and torch.all(ll3[:, 0] == SENTINEL)
            assert torch.all(raw[:shift // item] == SENTINEL) and torch.all(raw[shift // item + T * S * W * d:] == SENTINEL)


@pytest.mark.gpu
def test_the_launches_of_a_call_do_not_depend_on_the_number_of_rungs(hip_engine):
    eng = hip_engine
    reports = []
    for T in (2, 5):
        p = problem(eng, T, 65, 8, torch.float64, "tpcn", 1, seed=3)
        for r in range(T):  # (every rung Student-t)
            p["refs"][r] = (*p["refs"][r][:3], 4.0 + r)
        pack = eng.pt_pack(p["x"], T, p["refs"], *p["mixes"])
        chain = eng.chain_alloc(T * 8, 65, 8)
        eng.synchronize()
        eng.profile(True)
        try:
            eng.pt_steps(pack, p["x"], *[v for _, v in p["dens"]], eng.asarray(p["betas"]), eng.asarray(p["rho"]),
                         torch.zeros(T, dtype=torch.int64, device=eng.device), p["seed"], 8, chain=chain, n_slots=8)
            reports.append({k: v[0] for k, v in eng.profile_report().items()})
        finally:
            eng.profile(False)
    print(reports)
    assert reports[0] == reports[1] == {"k_pt_gamma": 1, "k_tpt_reg": 8, "k_pt_close": 8, "k_pt_chain_rows": 8}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [3, 5, 64])
def test_ladder_kernel_against_the_restatement(hip_engine, T):
    """Synthetic counts, five updates in a row.  Relative deviation of 1 / beta_i from the numpy restatement at most (T + 4) eps: one exp
    and one multiply of about an ulp each per gap, a running sum of up to T positive terms on top.  Observed on MI355X: DESIGN.md
    section 3.22."""
    eng = hip_engine
    g = np.random.default_rng(T)
    W = 128
    b0 = np.concatenate(([1.0], np.sort(g.uniform(1e-3, 0.99, T - 2))[::-1], [0.0]))
    betas_d = eng.asarray(b0)
    cb, counts_d = guarded(eng, np.zeros(T - 1, dtype=np.int64), torch.int64)
    sb, snap_d = guarded(eng, np.zeros(T - 1, dtype=np.int64), torch.int64)
    hist = torch.full((7, T), SENTINEL, dtype=torch.float64, device=eng.device)
    hist[0].copy_(betas_d)
    ref, snap, counts, worst = b0.copy(), np.zeros(T - 1, dtype=np.int64), np.zeros(T - 1, dtype=np.int64), 0.0
    for m in range(1, 6):
        counts = counts + g.integers(0, W + 1, T - 1)
        counts_d.copy_(torch.as_tensor(counts))
        before = betas_d.cpu().numpy()
        want, snap = ladder_update_ref(before, counts, snap, W, m, 10.0, 1.0)  # (from the device's own ladder: one update's deviation)
        eng.pt_ladder_adapt(W, counts_d, snap_d, betas_d, hist, m, 10.0, 1.0)
        got = betas_d.cpu().numpy()
        assert got[0] == 1.0 and got[-1] == 0.0 and np.all(np.diff(got) < 0)
        dev = float(np.max(np.abs(1.0 / got[1:-1] - 1.0 / want[1:-1]) / (1.0 / want[1:-1])))
        worst = max(worst, dev)
        assert dev <= (T + 4) * EPS, (T, m, dev / EPS)
        assert np.array_equal(snap_d.cpu().numpy(), counts) and hist[m].cpu().numpy().tobytes() == got.tobytes()
    print("T", T, "largest relative deviation of 1 / beta_i:", worst / EPS, "eps; bound", T + 4)
    assert torch.all(hist[6] == SENTINEL) and hist[0].cpu().numpy().tobytes() == b0.tobytes()
    assert torch.all(cb[T - 1:] == int(SENTINEL)) and torch.all(sb[T - 1:] == int(SENTINEL))


@pytest.mark.gpu
def test_sampler_end_to_end_batched_equals_per_rung_and_adapts(hip_engine):
    """T = 4, W = 257, d = 8, 12 steps through the facade: with swap_every = 1 (segments of one step: both paths step on x) the chain
    of the batched run is the per-rung run's, byte for byte; with adapt_ladder=True the run finishes and returns its final ladder."""
    from aspire_amd import Aspire, Samples
    from test_pt_batched import mixture_targets

    d = 8
    lik, pri = mixture_targets(d)
    names = [f"x_{i}" for i in range(d)]

    def run(**kw):
        a = Aspire(log_likelihood=lik, log_prior=pri, dims=d, flow_backend="gaussian", xp=np, parameters=names, engine=hip_engine, seed=5)
        a.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, d)), parameters=names, xp=np))
        out = a.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=hip_engine, rng=np.random.default_rng(3), n_walkers=257, n_temps=4,
                                 n_steps=12, swap_every=1, **kw)
        return a.sampler, out

    sa, a = run()
    sb, b = run(rung_launch="batched")
    assert "asmc_pt_steps" in sb.last_mutation_path and "asmc_pcn_mutate" in sa.last_mutation_path
    for name in ("chain", "log_likelihood", "log_prior"):
        assert host(getattr(a, name)).tobytes() == host(getattr(b, name)).tobytes(), name
    for name in ("rung_step_size", "rung_acceptance", "swap_acceptance"):
        assert getattr(sa, name).tobytes() == getattr(sb, name).tobytes(), name
    assert sa.evidence == sb.evidence
    sc, c = run(rung_launch="batched", adapt_ladder=True, burnin=6)
    betas = host(c.betas)
    assert c.chain_shape == (4, 6, 257) and sc.ladder_history.shape == (4, 4) and np.array_equal(betas, sc.ladder_history[-1])
    assert betas[0] == 1.0 and betas[-1] == 0.0 and np.all(np.diff(betas) < 0) and not np.array_equal(betas, sc.ladder_history[0])
    assert np.all(np.isfinite(sc.evidence["stepping_stone"])) and np.all(np.isfinite(sc.evidence["thermodynamic_integration"]))


@pytest.mark.gpu
def test_uneven_ladder_evens_out_on_the_device(hip_engine):
    """The statistical check of tests/test_pt_batched.py at 256 walkers, 300 steps, half discarded, through the facade."""
    def run(adapt):
        a = aspire_for(hip_engine, False)
        out = a.sample_posterior(n_samples=None, sampler="pt_minipcn", engine=hip_engine, rng=np.random.default_rng(3), n_walkers=256,
                                 betas=UNEVEN, n_steps=300, burnin=150, swap_every=1, rung_launch="batched", adapt_ladder=adapt)
        return a.sampler, out

    s, out = run(True)
    fixed, _ = run(False)
    assert out.chain_shape == (5, 150, 256) and s.ladder_history.shape == (76, 5)
    uneven_check(s, out, fixed)
