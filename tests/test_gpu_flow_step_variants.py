"""One oracle case per compiled instantiation of the flow-proposal step kernels (k_pcn_flow_fused at d <= 32, csrc/asmc_pcn_fused.hip;
k_pcn_flow16 / k_tpcn_flow16 at 32 < d <= 128, csrc/asmc_flow16.hip).

The library dispatches among 36 + 144 template instantiations of the two kernels (state dtype, hidden width, noise generator, pCN /
tpCN, split-fp16 or fp32 MFMA, flow kind, mixture targets, LDS slot geometry).  A subtly wrong instantiation - a register hazard
next to an MFMA, a noise mode nobody compares - passes every test that never launches it.  VARIANTS below is plain data (no GPU
needed to import it): one row per instantiation, the template arguments it names and the inputs that reach it.  The CPU test
checks that its set equals the compiled set (host symbols of the built library), so a new instantiation without a row fails.

Each GPU case runs `pcn_mutate_flow` for two steps on a small population with a ragged last group / tile, asserts from
`profile_variants()` that exactly the declared instantiation ran at every step, compares with the oracle's restatement of the
whole step (`oracle.pcn_flow_step` / `tpcn_flow_step`, same noise generator, flow kind and targets) at the tolerances
tests/test_gpu_flow16.py and test_gpu_parity.py::test_pcn_fast_noise_vs_oracle justify, checks the carried densities at the
returned rows, and repeats the call on fresh inputs with another kernel in between: the same bits (run-to-run difference is the
signature of a wait-state hazard).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

COUPLING, MAF = 0, 1
NOISE = {"f64": 0, "f32": 1}
TYPE = {"f64": "d", "f32": "f"}
FLOW16_CHUNK_WORDS = 8192  # csrc/asmc_flow16_dev.h
LDS_BYTES = 160 * 1024
MAX_LAYERS = 24  # deepest flow a case builds to force a geometry


def layer_a(kind, D, W):
    """Flow16<KIND, D, W>::LAYER_A (csrc/asmc_flow16_dev.h): words of operand images per layer."""
    cs = D // 4 if kind == MAF else D // 8
    ks1, ks2, nb1, nb3 = cs // 8, W // 32, W // 16, cs // 2
    return nb1 * ks1 * 512 + nb1 * ks2 * 512 + nb3 * ks2 * 512


def flow16_step_lds(kind, D, W, cw, n_layers, c_ll, c_lp, noise):
    """f16_step_lds (csrc/asmc_flow16.hip): the one-kernel step's LDS bytes at slot size `cw` words."""
    nb = D // 16
    blob = 2 * nb * (nb + 1) * 64 + D + (c_ll + c_lp) * D * 2 + (3 * D) // 2
    bias = 2 * W + (D // 4 if kind == MAF else D // 8) * 8
    return blob * 8 + n_layers * bias * 4 + (384 * 16 if noise == "f64" else 0) + 2 * cw * 4 + 16 * 8 + 2 * 8 * 8


def fused_symbol(T, W, noise, hs, kind, mix):
    return f"_Z16k_pcn_flow_fusedI{TYPE[T]}Li{W}ELi{NOISE[noise]}ELb{int(hs)}ELi{kind}ELb{int(mix)}EE"


def flow16_symbol(T, D, W, kind, noise, tp, cw, threads=512):
    return f"_Z12k_pcn_flow16I{TYPE[T]}Li{D}ELi{W}ELi{kind}ELi{NOISE[noise]}ELb{int(tp)}ELi{threads}ELi{cw}EE"


def _flow16_inputs(kind, D, W, cw, noise, c_want):
    """(n_layers, likelihood components) that make launch_pcn_flow16 take slot size `cw`, or the reason no case can: the step
    must fit at 32 KiB slots (asmc_pcn_flow16_ok), and at D = 64 the whole-layer slot is taken whenever two of them fit."""
    def fits(c, m, c_ll):
        return flow16_step_lds(kind, D, W, c, m, c_ll, 1, noise) <= LDS_BYTES

    whole = layer_a(kind, D, W) if D == 64 else None
    for c_ll in dict.fromkeys((c_want, 1)):
        for m in ([2, 1] if cw == whole or whole is None else [2, 1] + list(range(3, MAX_LAYERS + 1))):
            if cw == whole and fits(cw, m, c_ll):
                return m, c_ll
            if cw == FLOW16_CHUNK_WORDS and fits(cw, m, c_ll) and (whole is None or not fits(whole, m, c_ll)):
                return m, c_ll
    if cw == whole:
        return (f"two whole-layer slots ({2 * cw * 4 // 1024} KiB) exceed the {LDS_BYTES // 1024} KiB LDS at any depth: "
                "launch_pcn_flow16 always falls back to 32 KiB slots")
    return (f"the fallback from whole-layer slots: two of those fit below {MAX_LAYERS + 1} layers at every component count, so only "
            "deeper flows or the ASMC_F16_SMALL_SLOTS A/B switch (read once per process) reach it")


def _variants():
    rows, excluded = [], {}
    # ---- k_pcn_flow_fused<T, W, NOISE, HS, KIND, MIX> (launch_pcn_flow_fused's case list)
    fused = [(64, "f64", True, COUPLING, False), (64, "f64", True, COUPLING, True), (64, "f32", True, COUPLING, True)]
    fused += [(w, nz, hs, COUPLING, False) for w in (64, 32, 128) for nz in ("f64", "f32") for hs in (True, False)
              if (w, nz, hs) != (64, "f64", True)]
    fused += [(w, nz, True, MAF, False) for w in (64, 32) for nz in ("f64", "f32")]
    # (a width-128 coupling layer takes 89 KiB of LDS: the fused step holds every layer resident, so one layer - asmc_pcn_flow_fused_ok)
    for i, (w, nz, hs, kind, mix) in enumerate(fused):
        for T in ("f64", "f32"):
            rows.append(dict(symbol=fused_symbol(T, w, nz, hs, kind, mix), kernel="k_pcn_flow_fused", T=T, kind=kind, d=32, dims=32,
                             hidden=w, n_layers=1 if w == 128 else 2 if kind == MAF else 3, noise=nz, nu=0.0, math="split" if hs else "f32",
                             ll_components=2 if mix else 1, lp_components=2 if mix and nz == "f64" else 1, n=64 * 4 + 29,
                             seed=100 + 2 * i + (T == "f32")))
    # ---- k_pcn_flow16<T, D, W, KIND, NOISE, TP, THREADS, CW> (F16_STEP_SHAPES x dtypes x noise x pCN / tpCN; D = 64 tries a
    # whole-layer slot first and falls back to FLOW16_CHUNK_WORDS when the LDS cannot hold two of them)
    k = 0
    for kind in (COUPLING, MAF):
        for D in (64, 128):
            for W in (64, 32, 128):
                for cw in [FLOW16_CHUNK_WORDS] + ([layer_a(kind, D, W)] if D == 64 else []):
                    for T in ("f64", "f32"):
                        for nz in ("f64", "f32"):
                            for tp in (False, True):
                                k += 1
                                sym = flow16_symbol(T, D, W, kind, nz, tp, cw)
                                pick = _flow16_inputs(kind, D, W, cw, nz, 2 if tp else 1)  # (the tpCN rows: two-component likelihood)
                                if isinstance(pick, str):
                                    excluded[sym] = pick
                                    continue
                                n_layers, c_ll = pick
                                dims = D if nz == "f64" else D - 12  # fast-noise rows on a zero-padded problem
                                rows.append(dict(symbol=sym, kernel="k_tpcn_flow16" if tp else "k_pcn_flow16", T=T, kind=kind, d=D,
                                                 dims=dims, hidden=W, n_layers=n_layers, noise=nz, nu=4.0 if tp else 0.0, math="split",
                                                 ll_components=c_ll, lp_components=1, n=16 * 13 + 5, seed=300 + k))
    return rows, excluded


VARIANTS, EXCLUDED = _variants()


def _row_id(r):
    return (f"{r['kernel']}-{'coupling' if r['kind'] == COUPLING else 'maf'}-D{r['d']}-W{r['hidden']}-{r['T']}-noise_{r['noise']}"
            f"-{r['math']}-c{r['ll_components']}{r['lp_components']}-L{r['n_layers']}-{r['symbol'][-12:]}")


def _compiled_step_symbols():
    """template-argument prefixes of every k_pcn_flow_fused / k_pcn_flow16 the library carries: host symbols of the built
    library, or the device assembly when no library is there"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "aspire_amd", "libasmc_hip.so")
    text = None
    if os.path.exists(lib):
        for nm in ("/opt/rocm/llvm/bin/llvm-nm", shutil.which("llvm-nm"), shutil.which("nm")):
            if nm and os.path.exists(nm):
                r = subprocess.run([nm, "-D", "--defined-only", lib], capture_output=True, text=True)
                if r.returncode == 0:
                    text = r.stdout
                    break
    if text is None:
        if not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("neither a built library nor hipcc")
        import importlib.util
        import tempfile

        spec = importlib.util.spec_from_file_location("audit_asm_hazards", os.path.join(root, "tools", "audit_asm_hazards.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with tempfile.TemporaryDirectory() as tmp:
            text = "".join(open(p).read() for p in mod.compile_all([], 2, tmp) if "flow16" in p or "fused" in p)
    return set(re.findall(r"(_Z16k_pcn_flow_fusedI\w+?EE|_Z12k_pcn_flow16I\w+?EE)v", text))


def test_variant_table_covers_every_compiled_step_instantiation():
    """Every compiled instantiation of the two step kernels has exactly one row or one written exclusion, and nothing else is
    listed; the exclusions are the geometries the LDS budget makes unreachable at the depths a case builds."""
    compiled = _compiled_step_symbols()
    listed = [r["symbol"] for r in VARIANTS]
    assert len(listed) == len(set(listed)), "one row per instantiation"
    assert not set(listed) & set(EXCLUDED)
    assert len(compiled) >= 180, len(compiled)
    assert set(listed) | set(EXCLUDED) == compiled, (sorted(compiled - set(listed) - set(EXCLUDED)), sorted((set(listed) | set(EXCLUDED)) - compiled))
    assert all(r and len(r) > 40 for r in EXCLUDED.values())
    assert len(EXCLUDED) <= 40, sorted(EXCLUDED)
    kinds = {(r["kernel"], r["noise"], r["math"], r["T"]) for r in VARIANTS}
    assert ("k_pcn_flow16", "f32", "split", "f64") in kinds and ("k_pcn_flow_fused", "f64", "f32", "f32") in kinds


# ---------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=1 << 12, d_max=128)


@pytest.fixture(scope="module")
def oracle():
    import oracle as O

    return O


_FLOWS = {}


def _flow(kind, dims, n_layers, hidden, eng):
    key = (kind, dims, n_layers, hidden)
    if key not in _FLOWS:
        from conftest import random_coupling_flow, random_maf_flow

        seed = 11 + n_layers + hidden + dims
        flow = random_coupling_flow(dims, n_layers, hidden, seed=seed) if kind == COUPLING else random_maf_flow(dims, n_layers, hidden, seed=seed)
        _FLOWS[key] = (flow, flow.device_coupling(eng), flow.export_layers())
    return _FLOWS[key]


def _targets(r, g):
    d = r["dims"]

    def mix(c, spread):
        if c == 1:
            return ([0.0], spread * g.normal(size=(1, d)), 0.7 + 0.6 * g.random(size=(1, d)))
        return (np.log([0.4, 0.6]), 0.5 * g.normal(size=(2, d)), 0.6 + g.random(size=(2, d)))

    return mix(r["ll_components"], 0.1), (mix(r["lp_components"], 0.0) if r["lp_components"] > 1 else ([0.0], np.zeros((1, d)), np.ones((1, d))))


@pytest.mark.gpu
@pytest.mark.parametrize("r", VARIANTS, ids=_row_id)
def test_flow_step_instantiation_vs_oracle(eng, oracle, r, monkeypatch):
    import torch

    n, d, n_steps, beta, rho, step0 = r["n"], r["dims"], 2, 0.4, 0.3, 9
    if r["math"] == "f32":
        monkeypatch.setenv("ASMC_FLOW_MATH", "f32")  # the fp32-MFMA flow chain (HS = false); the packed flow is the same
    kname = "coupling" if r["kind"] == COUPLING else "maf"
    flow, dev, (ws, bs) = _flow(r["kind"], d, r["n_layers"], r["hidden"], eng)
    g = np.random.default_rng(r["seed"])
    x0 = 0.9 * g.normal(size=(n, d))
    a = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.tril(np.linalg.cholesky(0.8 * (np.eye(d) + 0.2 * a @ a.T)))
    Linv, mu = np.tril(np.linalg.inv(L)), 0.05 * g.normal(size=d)
    m_ll, m_lp = _targets(r, g)
    o_ll, o_lp = oracle.Mixture(*m_ll), oracle.Mixture(*m_lp)
    t_ll, t_lp = eng.make_mixture(*m_ll), eng.make_mixture(*m_lp)
    dt = torch.float64 if r["T"] == "f64" else torch.float32
    x0t = torch.as_tensor(x0).to(dt)
    xr = x0t.double().numpy().copy()
    flp = oracle.coupling_logprob if r["kind"] == COUPLING else oracle.maf_logprob
    llr, lpr, lqr = o_ll.logpdf(xr), o_lp.logpdf(xr), flp(xr, ws, bs, flow.loc.numpy(), flow.scale.numpy())
    ll0, lp0 = llr.copy(), lpr.copy()  # (the oracle steps xr, llr, lpr, lqr in place)
    x0d = x0t.to(eng.device).contiguous()
    lq0 = eng.coupling_logprob(x0d, dev)
    mud, Ld, Lid = eng.asarray(mu), eng.asarray(L), eng.asarray(Linv)

    def run():
        xd, lld, lpd, lqd = x0d.clone(), eng.asarray(ll0), eng.asarray(lp0), lq0.clone()
        eng.profile(True)
        n_acc, _, _ = eng.pcn_mutate_flow(xd, lld, lpd, lqd, beta, mud, Ld, Lid, t_ll, t_lp, dev, 4242, 17, rho, n_steps, step0, 0.234,
                                          False, r["noise"], r["nu"])
        var = eng.profile_variants()
        eng.profile(False)
        torch.cuda.synchronize()
        return xd, lld, lpd, lqd, np.array(n_acc), var

    xd, lld, lpd, lqd, n_acc, var = run()
    # 1. exactly the declared instantiation took every step
    steps = {s: c for s, c in var.items() if s.startswith(("_Z16k_pcn_flow_fused", "_Z12k_pcn_flow16"))}
    assert len(steps) == 1 and next(iter(steps)).startswith(r["symbol"] + "v") and steps[next(iter(steps))] == n_steps, (r["symbol"], var)
    # 2. the oracle's restatement of the whole step
    acc_ref, margins = [], []
    for t in range(n_steps):
        with oracle.accept_margins(n) as m:
            args = (xr, llr, lpr, lqr, beta, mu, L, Linv, rho)
            tail = (o_ll, o_lp, ws, bs, flow.loc.numpy(), flow.scale.numpy(), 4242, 17, step0 + t, r["noise"], 0)
            if r["nu"] > 0:
                acc_ref.append(oracle.tpcn_flow_step(*args, r["nu"], *tail, flow_kind=kname))
            else:
                acc_ref.append(oracle.pcn_flow_step(*args, *tail, flow_kind=kname))
        margins.append(m.copy())
    got = xd.double().cpu().numpy()
    f64 = r["T"] == "f64"
    if r["noise"] == "f64":
        tol, edge = (1e-9, 12) if f64 else (3e-5, max(12, n // 20))
        close = np.all(np.abs(got - xr) <= tol * (1 + np.abs(xr)), axis=1)
        assert (~close).sum() <= edge, (~close).sum()
        if f64:  # rows that ended elsewhere took their other decision at a razor's edge
            razor = np.min(np.abs(np.array(margins)), axis=0)
            assert np.all(razor[~close] <= (1e-4 if r["d"] == 32 else 2e-4)), razor[~close]
    else:  # hardware vs libm Box-Muller: the same moves up to a handful of razor edges, moved rows to fp32 noise accuracy
        edge = 4 if f64 else max(8, n // 25)
        x00 = x0t.double().numpy()  # (a rejected row comes back through the whitened state: equal to rounding, not in bits)
        moved_g, moved_r = (np.any(np.abs(v - x00) > (1e-9 if f64 else 1e-5) * (1 + np.abs(x00)), axis=1) for v in (got, xr))
        assert (moved_g != moved_r).sum() <= edge, (moved_g != moved_r).sum()
        same = moved_g == moved_r
        close = np.all(np.abs(got - xr) <= (1e-5 if f64 else 3e-5) * (1 + np.abs(xr)), axis=1)
        assert (~close[same]).sum() <= edge, (~close[same]).sum()
    assert np.all(np.abs(n_acc - np.array(acc_ref)) <= edge), (n_acc, acc_ref)
    assert 0.02 < n_acc.mean() / n < 0.98, n_acc
    # 3. the carried densities are the targets' and the flow's at the returned rows
    rt, at = (1e-10, 1e-9) if f64 else (1e-4, 3e-3)
    np.testing.assert_allclose(lld.cpu().numpy(), o_ll.logpdf(got), rtol=rt, atol=at)
    np.testing.assert_allclose(lpd.cpu().numpy(), o_lp.logpdf(got), rtol=rt, atol=at)
    torch.testing.assert_close(lqd, eng.coupling_logprob(xd, dev), rtol=1e-5, atol=3e-3)
    # 4. the same call again on fresh inputs, another kernel in between: the same bits
    eng.coupling_logprob(torch.flip(x0d, [0]).contiguous(), dev)
    again = run()
    for u, v in zip((xd, lld, lpd, lqd), again[:4]):
        assert torch.equal(u, v), "run-to-run difference"
    assert np.array_equal(n_acc, again[4])
