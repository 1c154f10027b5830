"""The pCN / tpCN step kernels of csrc/asmc_pcn.hip and asmc_pcn_mm.hip on every dispatch path of asmc_pcn_mutate, asmc_pcn_propose,
asmc_pcn_accept and the asmc_pcn_ysplit_* session, and at the edges, against the plain restatement of tests/pcn_ref.py at float64.

Every case enables profiling, runs, asserts from profile_variants() the template instantiations that ran and how often, and then
compares row by row: positions, the three carried densities, accept counts.  Tolerances: DESIGN.md section 3.19 - the float64
restatement's own error against its longdouble run on the case's inputs is the unit, the device gets pcn_ref.MULT units (plus the
float32 terms where the storage type or the noise mode is fp32); none comes from the device's output.  A row whose accept margin
|log_a - log u| the restatement itself cannot call within that tolerance is skipped from that step on; tests/test_pcn_ref.py shows on
the CPU that every case of the table keeps those rows within pcn_ref.razor_cap.

Which shape takes which path (pcn_mutate_impl in csrc/asmc_pcn_drive.hip; launch_pcn_step behind pcn_step_launch in csrc/asmc_pcn.hip;
asmc_pcn_mm_launch):

  k_pcn_reg<T, D, NOISE, MODE>   d in {4, 8, 16, 32}, 16-byte aligned x.  n_steps < 4 or ASMC_PCN_XSTATE: X_STEP / X_STEP_T;
                                 n_steps >= 4: WHITEN_S, Y_STEP_S / _TS (single Gaussians) or _SG / _TSG (mixtures), UNWHITEN_S
                                 on the coordinate-major scratch; ASMC_PCN_AOS: WHITEN, Y_STEP / Y_STEP_T, UNWHITEN in place
                                 (mixtures: the x-state loop).  One block = four 64-row wave tiles.
  k_pcn_mm<T, D, NOISE, MODE>    d in {64, 128}, aligned x: whiten, n_steps x step, un-whiten; groups of 16 rows, 8 waves
  k_pad_rows / k_pad_tables / k_unpad_rows   any other d <= 128: zero-padded to the next width, noise and |y|^2 on the real d
  k_pcn_step<T, VEC, PHASE>      the generic LDS kernel: x (or x_prop) not 16-byte aligned at a width with kernels of its own, d > 128,
                                 an engine whose d_max is above 128 (no padding), ASMC_PCN_GENERIC, ASMC_PCN_NOPAD.  VEC = 16 / 8 / 4
                                 by the alignment of rows and pointers; PHASE 1 is asmc_pcn_propose.
  k_gamma_draw<F32>              tpCN: one launch per eight steps, cached by (n, seed, gid0, shape, noise, step)
  asmc_pcn_ysplit_*              the whitened-state split session, d in {4, 8, 16, 32}, aligned x: begin = k_pcn_reg<.., WHITEN_S>,
                                 propose / accept = k_pcn_reg_flow<T, D, NOISE, PROPOSE_SX / ACCEPT_S / ACCEPT_SJ> (the only
                                 k_pcn_reg_flow modes reachable without a flow), end = k_pcn_reg<.., UNWHITEN_XS>
"""
import ctypes

import numpy as np
import pytest
import torch

import pcn_ref as P

pytestmark = pytest.mark.gpu

FAMILIES = ("k_pcn_reg", "k_pcn_step", "k_pcn_mm", "k_gamma_draw", "k_pcn_accept_flags", "k_copy_flagged_rows", "k_pad_rows",
            "k_unpad_rows", "k_pad_tables", "k_pcn_pack", "k_pcn_adapt", "k_count_sum")
EXCLUDE = ("k_pcn_reg_flow",)
# k_pcn_reg modes / k_pcn_mm modes (csrc/asmc_pcn_shared.h, asmc_pcn_dev.h)
X_STEP, Y_STEP, WHITEN, UNWHITEN, X_STEP_T, Y_STEP_T, WHITEN_S, Y_STEP_S, Y_STEP_TS, UNWHITEN_S = 0, 1, 2, 3, 5, 6, 7, 8, 9, 10
X_PROPOSE, X_PROPOSE_T, X_PROPOSE_PAD, X_PROPOSE_PAD_T, Y_STEP_SG, Y_STEP_TSG, UNWHITEN_XS = 12, 13, 14, 15, 16, 17, 11
FLOW_ACCEPT_S, FLOW_PROPOSE_SX, FLOW_ACCEPT_SJ = 3, 4, 5  # k_pcn_reg_flow modes of the split session
MM_WHITEN, MM_STEP, MM_UNWHITEN, MM_STEP_T, MM_XPROPOSE, MM_XPROPOSE_T = 0, 1, 2, 3, 4, 5
SENT = 777.25  # guard-band value (exact in fp32)
GUARD = 70     # rows behind row n: more than a tile
SEEN = {}      # symbol prefix -> launches the module's asserted runs have covered


def sym(name, targs=None):
    return f"_Z{len(name)}{name}" + ("" if targs is None else f"I{targs}E")


def reg(T, D, nz, mode):
    return ("k_pcn_reg", f"{T}Li{D}ELi{nz}ELi{mode}E")


def mm(T, D, nz, mode):
    return ("k_pcn_mm", f"{T}Li{D}ELi{nz}ELi{mode}E")


def flow(T, D, nz, mode):
    return ("k_pcn_reg_flow", f"{T}Li{D}ELi{nz}ELi{mode}E")


def gen(T, vec, phase):
    return ("k_pcn_step", f"{T}Li{vec}ELi{phase}E")


def gam(f32):
    return ("k_gamma_draw", f"Lb{int(f32)}E")


def _table():
    """Every instantiation asmc_pcn_mutate, asmc_pcn_propose, asmc_pcn_accept and the asmc_pcn_ysplit_* session can reach without a
    flow (the flow modes have their own module, test_gpu_flow_step_variants.py; of k_pcn_reg_flow only the session's three modes
    are here).  k_pcn_reg<.., UNWHITEN_X> (mode 4) is the row-major un-whitening of asmc_pcn_mutate_flow: no session reaches it."""
    t = set()
    for T in "df":
        for D in (4, 8, 16, 32):
            for nz in (0, 1):
                for mode in (X_STEP, X_STEP_T, Y_STEP, Y_STEP_T, Y_STEP_S, Y_STEP_TS, Y_STEP_SG, Y_STEP_TSG):
                    t.add(reg(T, D, nz, mode))
            for mode in (WHITEN, UNWHITEN, WHITEN_S, UNWHITEN_S, UNWHITEN_XS, X_PROPOSE, X_PROPOSE_T):
                t.add(reg(T, D, 0, mode))
            for nz in (0, 1):
                for mode in (FLOW_PROPOSE_SX, FLOW_ACCEPT_S, FLOW_ACCEPT_SJ):
                    t.add(flow(T, D, nz, mode))
        t.update((reg(T, 32, 0, X_PROPOSE_PAD), reg(T, 32, 0, X_PROPOSE_PAD_T)))
        for D in (64, 128):
            for nz in (0, 1):
                t.update((mm(T, D, nz, MM_STEP), mm(T, D, nz, MM_STEP_T)))
            for mode in (MM_WHITEN, MM_UNWHITEN, MM_XPROPOSE, MM_XPROPOSE_T):
                t.add(mm(T, D, 0, mode))
        for vec in (16, 8, 4):
            for phase in (0, 1):
                if not (T == "d" and vec == 4):  # compiled, unreachable: a double's address and row length are multiples of 8
                    t.add(gen(T, vec, phase))
        t.update((("k_pad_rows", T), ("k_unpad_rows", T), ("k_copy_flagged_rows", T)))
    t.update((gam(0), gam(1), ("k_pad_tables",), ("k_pcn_pack",), ("k_pcn_adapt",), ("k_pcn_accept_flags",),
              ("k_copy_flagged_rows16",)))
    return t


TABLE = _table()


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(scope="module")
def big():
    """An engine above the suite's d_max = 128: it pads nothing, so every width without kernels of its own runs on the generic
    kernel, and d = 140 is within its tables."""
    from aspire_amd.engine import HipEngine

    e = HipEngine(0, n_max=1 << 17, d_max=256)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A HIP fault is sticky: every later call on the device fails with it.  End the session there instead of running on."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device fault: {exc}", returncode=3)


def ran(eng, fn, expect, exclude=EXCLUDE):
    """fn() with the assertion that, of this module's kernel families, exactly the instantiations `expect` ran ({(name, template
    arguments): launches}).  exclude = (): k_pcn_reg_flow counts as well (the split session)."""
    eng.profile(True)
    try:
        out = fn()
        var = {s: c for s, c in eng.profile_variants().items() if any(f in s for f in FAMILIES) and not any(f in s for f in exclude)}
    finally:
        eng.profile(False)
    want = {sym(*k): c for k, c in expect.items()}
    for s in var:
        assert any(s.startswith(p) for p in want), (s, sorted(want))
    for p, cnt in want.items():
        got = sum(c for s, c in var.items() if s.startswith(p))
        assert got == cnt, (p, cnt, var)
    for k in expect:
        assert k in TABLE, k
        SEEN[k] = SEEN.get(k, 0) + expect[k]
    return out


def tdt(store):
    return torch.float64 if store == "f64" else torch.float32


def banded(eng, a, dtype, offset=0):
    """`a` on the device inside a buffer of the sentinel: `offset` elements in front (an offset view: the data pointer moves off
    its 16-byte alignment), GUARD rows behind.  Returns (view, whole buffer)."""
    a = np.ascontiguousarray(a)
    row = a.shape[1] if a.ndim == 2 else 1
    buf = torch.full((offset + a.size + GUARD * row,), SENT, dtype=dtype, device=eng.device)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a).to(dtype))
    return view, buf


def band_intact(view, buf, offset=0):
    n = view.numel()
    return bool((buf[:offset] == SENT).all()) and bool((buf[offset + n:] == SENT).all())


def pick_vec(rowbytes, *tensors):
    a = 0
    for t in tensors:
        a |= t.data_ptr()
    return 16 if rowbytes % 16 == 0 and a % 16 == 0 else 8 if rowbytes % 8 == 0 and a % 8 == 0 else 4


def gamma_launches(step0, n_steps):
    """k_gamma_draw launches of a tpCN call on an empty cache: a launch draws eight steps from the one that missed; a step index
    that wraps past 2^32 misses (the hit test is step >= first && step - first < 8)."""
    launches, first = 0, None
    for t in range(n_steps):
        step = (step0 + t) & 0xFFFFFFFF
        if first is None or not (step >= first and step - first < 8):
            launches, first = launches + 1, step
    return launches


def expected_mutate(c, xd, on_big, step0=5):
    """The instantiations one asmc_pcn_mutate call of case `c` launches: pcn_mutate_impl's dispatch (csrc/asmc_pcn_drive.hip), restated."""
    T, nz, tp, d, s = ("d" if c["store"] == "f64" else "f"), int(c["mode"] == "f32"), c["nu"] > 0, c["d"], c["n_steps"]
    es = 8 if T == "d" else 4
    env = c["env"]
    e = {("k_pcn_adapt",): s}
    if tp:
        e[gam(nz)] = gamma_launches(step0, s)
    D = P.pad_dim(d)
    aligned = xd.data_ptr() % 16 == 0
    generic = env == "ASMC_PCN_GENERIC" or D > 128 or (D != d and (on_big or env == "ASMC_PCN_NOPAD")) or (D == d and not aligned)
    if generic:
        e[gen(T, pick_vec(d * es, xd), 0)] = s
        return e
    if D != d:
        e.update({("k_pad_rows", T): 1, ("k_pad_tables",): 1, ("k_unpad_rows", T): 1})
    if D in (64, 128):
        e.update({mm(T, D, 0, MM_WHITEN): 1, mm(T, D, nz, MM_STEP_T if tp else MM_STEP): s, mm(T, D, 0, MM_UNWHITEN): 1})
        return e
    e[("k_pcn_pack",)] = 1
    if c["state"] == "x":
        e[reg(T, D, nz, X_STEP_T if tp else X_STEP)] = s
    elif env == "ASMC_PCN_AOS":
        e.update({reg(T, D, 0, WHITEN): 1, reg(T, D, nz, Y_STEP_T if tp else Y_STEP): s, reg(T, D, 0, UNWHITEN): 1})
    else:
        step = (Y_STEP_TS if tp else Y_STEP_S) if c["C"] == 1 else (Y_STEP_TSG if tp else Y_STEP_SG)
        e.update({reg(T, D, 0, WHITEN_S): 1, reg(T, D, nz, step): s, reg(T, D, 0, UNWHITEN_S): 1})
    return e


def device_mutate(e, c, inputs, expect=None, adapt=False, gid0=1000, step0=5, seed=None, target=0.234):
    """One asmc_pcn_mutate call of case `c` on engine `e` with guard bands round every buffer: (got dict, counts, rho_hist, rho)."""
    x, ll, lp, lq, mu, L, Linv, mixes = inputs
    xd, xbuf = banded(e, x, tdt(c["store"]), c["offset"])
    cd = [banded(e, v, torch.float64) for v in (ll, lp, lq)]
    dm = [e.make_mixture(*m) for m in mixes]
    mud, Ld, Lid = (e.asarray(v) for v in (mu, L, Linv))
    seed = 4242 + c["seed"] if seed is None else seed
    call = lambda: e.pcn_mutate(xd, cd[0][0], cd[1][0], cd[2][0], c["beta"], mud, Ld, Lid, dm[0], dm[1], dm[2], seed, gid0, c["rho"],
                                c["n_steps"], step0, target, adapt, c["mode"], c["nu"])
    n_acc, hist, rho = ran(e, call, expected_mutate(c, xd, e.d_max > 128, step0) if expect is None else expect(xd))
    torch.cuda.synchronize()
    assert band_intact(xd, xbuf, c["offset"]), "x: written outside its n rows"
    for v, b in cd:
        assert band_intact(v, b), "carried density: written behind row n"
    got = dict(x=xd.double().cpu().numpy(), ll=cd[0][0].cpu().numpy(), lp=cd[1][0].cpu().numpy(), lq=cd[2][0].cpu().numpy())
    return got, np.asarray(n_acc), np.asarray(hist), rho


def check_case(e, c, monkeypatch):
    if c["env"] and c["env"].startswith("ASMC_"):
        monkeypatch.setenv(c["env"], "1")
    inputs, ref, (tx, tc, tm) = P.case_reference(c)
    got, n_acc, hist, rho = device_mutate(e, c, inputs)
    und = P.compare(got, ref, ref["margins"], tx, tc, tm, label=f'{c["store"]} storage, {c["mode"]} noise')
    assert np.all(np.abs(n_acc - ref["counts"]) <= und), (n_acc, ref["counts"], und)
    assert np.all(hist == c["rho"]) and rho == c["rho"]
    if c["state"] == "x":  # a row the restatement never moves comes back bit for bit (the whitened paths: within the tolerance above)
        still = np.all(ref["margins"] < -tm, axis=0) | np.all(np.isnan(ref["margins"]), axis=0)
        x0 = inputs[0]
        assert np.array_equal(got["x"][still], x0[still])
        assert np.array_equal(got["ll"][still], inputs[1][still])


@pytest.mark.parametrize("c", [c for c in P.CASES if c["env"] not in ("big", "session")], ids=P.case_id)
def test_mutate_vs_restatement(eng, c, monkeypatch):
    check_case(eng, c, monkeypatch)


@pytest.mark.parametrize("c", [c for c in P.CASES if c["env"] == "big"], ids=P.case_id)
def test_mutate_without_padding_vs_restatement(big, c, monkeypatch):
    check_case(big, c, monkeypatch)


def test_generic_kernel_second_trip_of_the_tile_loop(big):
    """More tiles than the generic kernel's grid holds: d = 140 in fp64 has one wave per block and one block per CU, the grid is
    capped at two rounds of resident blocks, so n = 64 (2 CUs) + 65 rows sends block 0 and block 1 round the loop again (the
    second with the ragged tile)."""
    cus = torch.cuda.get_device_properties(big.device).multi_processor_count
    per_wave = 64 * (((140 * 8 + 7) & ~7) + 16) + 64 * 8 * 140
    blocks_per_cu = max(1, min(8, (160 * 1024) // (per_wave + 384 * 16)))
    n = 64 * (2 * cus * blocks_per_cu) + 65
    assert n <= big.n_max and n * 140 * 8 < 40e6
    c = dict(P._case(140, n, 1, 0.0, 1, env="big"), state="x")
    c["seed"] = 9
    check_case(big, c, None)


def test_generic_kernel_draws_the_noise_mode_it_is_asked_for(eng):
    """noise = "f32" on a buffer that is not 16-byte aligned (the generic kernel) samples the same stream as the same call on an
    aligned buffer (the register kernel): the parent's generic kernel always drew the fp64 normals (and, for tpCN, mixed them
    with fp32-mode Gamma variates).  Same hardware normals on both paths: the two results differ by operation order alone."""
    c = dict(P._case(8, 257, 1, 5.5, 1, "f64", "f32"), state="x")
    c["seed"] = 77
    inputs, ref, (tx, tc, tm) = P.case_reference(c)
    a, na, _, _ = device_mutate(eng, c, inputs)
    c1 = dict(c, offset=1)
    # (same n, seed, gid0, shape, noise mode and step: the second call finds its Gamma variates drawn - where x lies is no part of the key)
    b, nb, _, _ = device_mutate(eng, c1, inputs, expect=lambda xd: {k: v for k, v in expected_mutate(c1, xd, False).items() if k[0] != "k_gamma_draw"})
    und = P.razor(ref["margins"], tm)
    u64 = P.units(ref, P.run_case(c, np.longdouble)[1], 8)
    np.testing.assert_allclose(a["x"][~und], b["x"][~und], rtol=P.MULT * u64["x"], atol=P.MULT * u64["x"])
    assert abs(int(na[0]) - int(nb[0])) <= und.sum()


@pytest.mark.parametrize("d,mode", [(5, "f64"), (33, "f32")])
def test_generic_kernel_under_the_switches_equals_the_padded_result(eng, d, mode, monkeypatch):
    """ASMC_PCN_NOPAD and ASMC_PCN_GENERIC at a zero-padded width: the same call - inputs, seed, counters - once on the padded
    kernels and once under each switch on the generic kernel, the device results compared with each other directly, within the
    case's tolerance (both are within it of the restatement: the cases of the table)."""
    c = dict(P._case(d, 130, 2, 5.5, 2, mode=mode), state=P.case_state(d, 2, 2))  # (d = 33 pads to a matrix-core width: whitened state)
    c["seed"] = 8000 + d
    inputs, ref, (tx, tc, tm) = P.case_reference(c)
    padded, n_pad, _, _ = device_mutate(eng, c, inputs)
    und = P.compare(padded, ref, ref["margins"], tx, tc, tm)
    for env in ("ASMC_PCN_NOPAD", "ASMC_PCN_GENERIC"):
        ce = dict(c, env=env)
        monkeypatch.setenv(env, "1")
        # (same n, seed, gid0, shape, noise mode and steps as the padded call: the Gamma variates are found drawn)
        got, n_gen, _, _ = device_mutate(eng, ce, inputs, expect=lambda xd: {k: v for k, v in expected_mutate(ce, xd, False).items() if k[0] != "k_gamma_draw"})
        monkeypatch.delenv(env)
        P.compare(got, padded, ref["margins"], tx, tc, tm)
        assert np.all(np.abs(n_gen - n_pad) <= und)


# ---- the split path ---------------------------------------------------------------------------------------------------------------
def device_propose(e, x, xp, mu, L, Linv, rho, nu, seed, gid0, step):
    n, d = x.shape
    q0, q0b = banded(e, np.zeros(n), torch.float64)
    q1, q1b = banded(e, np.zeros(n), torch.float64)
    mud, Ld, Lid = (e.asarray(v) for v in (mu, L, Linv))
    from aspire_amd._lib import check

    check(e.lib.asmc_pcn_propose(e._ctx, n, d, e._xdt(x), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(xp.data_ptr()),
                                 ctypes.c_void_p(q0.data_ptr()), ctypes.c_void_p(q1.data_ptr()), ctypes.c_void_p(mud.data_ptr()),
                                 ctypes.c_void_p(Ld.data_ptr()), ctypes.c_void_p(Lid.data_ptr()), rho, float(nu), seed, gid0, step,
                                 e._stream), "asmc_pcn_propose")
    torch.cuda.synchronize()
    assert band_intact(q0, q0b) and band_intact(q1, q1b)
    return q0.cpu().numpy(), q1.cpu().numpy()


PROPOSE = [  # (d, n, nu, store, x offset, x_prop offset, engine, branch)
    (8, 257, 0.0, "f64", 0, 0, "eng", "reg"), (4, 65, 5.5, "f32", 0, 0, "eng", "reg"), (16, 64, 5.5, "f64", 0, 0, "eng", "reg"),
    (32, 130, 0.0, "f32", 0, 0, "eng", "reg"), (4, 63, 0.0, "f64", 0, 0, "eng", "reg"), (8, 130, 5.5, "f32", 0, 0, "eng", "reg"),
    (16, 130, 0.0, "f32", 0, 0, "eng", "reg"), (32, 257, 5.5, "f64", 0, 0, "eng", "reg"),
    (4, 130, 5.5, "f64", 0, 0, "eng", "reg"), (8, 130, 5.5, "f64", 0, 0, "eng", "reg"), (16, 130, 0.0, "f64", 0, 0, "eng", "reg"),
    (32, 130, 0.0, "f64", 0, 0, "eng", "reg"), (4, 130, 0.0, "f32", 0, 0, "eng", "reg"), (8, 130, 0.0, "f32", 0, 0, "eng", "reg"),
    (16, 130, 5.5, "f32", 0, 0, "eng", "reg"), (32, 130, 5.5, "f32", 0, 0, "eng", "reg"),
    (17, 130, 0.0, "f64", 0, 0, "eng", "pad32"), (31, 65, 5.5, "f64", 0, 0, "eng", "pad32"), (20, 257, 5.5, "f32", 0, 0, "eng", "pad32"),
    (25, 64, 0.0, "f32", 0, 0, "eng", "pad32"),
    (5, 130, 5.5, "f64", 0, 0, "eng", "rowpad"), (9, 65, 0.0, "f32", 0, 0, "eng", "rowpad"), (40, 130, 5.5, "f64", 0, 0, "eng", "rowpad"),
    (100, 65, 0.0, "f32", 0, 0, "eng", "rowpad"), (33, 17, 0.0, "f64", 0, 0, "eng", "rowpad"), (65, 16, 5.5, "f32", 0, 0, "eng", "rowpad"),
    (64, 129, 0.0, "f64", 0, 0, "eng", "mm"), (128, 17, 5.5, "f64", 0, 0, "eng", "mm"), (64, 16, 5.5, "f32", 0, 0, "eng", "mm"),
    (128, 127, 0.0, "f32", 0, 0, "eng", "mm"), (64, 1, 5.5, "f64", 0, 0, "eng", "mm"), (128, 15, 0.0, "f64", 0, 0, "eng", "mm"),
    (64, 128, 0.0, "f32", 0, 0, "eng", "mm"), (128, 130, 5.5, "f32", 0, 0, "eng", "mm"),
    (8, 130, 5.5, "f64", 0, 1, "eng", "generic"), (8, 65, 0.0, "f64", 1, 0, "eng", "generic"), (4, 130, 5.5, "f32", 0, 1, "eng", "generic"),
    (16, 257, 0.0, "f32", 2, 2, "eng", "generic"), (64, 64, 5.5, "f64", 0, 1, "eng", "generic"),
    (5, 130, 5.5, "f64", 0, 0, "big", "generic"), (140, 65, 0.0, "f64", 0, 0, "big", "generic"), (140, 130, 5.5, "f32", 0, 0, "big", "generic"),
]


@pytest.mark.parametrize("k,d,n,nu,store,xo,po,which,branch", [(k, *p) for k, p in enumerate(PROPOSE)])
def test_propose_vs_restatement(eng, big, k, d, n, nu, store, xo, po, which, branch):
    """asmc_pcn_propose on its five branches: x', 2 c(|y|^2) and 2 c(|y'|^2) (c: the reference's correction on the REAL d) of every
    row against the restatement; x_prop, the two outputs and x itself keep their guard bands."""
    e = eng if which == "eng" else big
    st = P.STORE[store]
    x, _, _, _, mu, L, Linv, _ = P.problem(n, d, 300 + d + n, 1, st)
    rho, seed, gid0, step = 0.35, 61 + k, 2**32 - 40, 3  # (a seed per case: see pcn_ref._cases)
    xd, xbuf = banded(e, x, tdt(store), xo)
    xp, pbuf = banded(e, np.zeros_like(x), tdt(store), po)
    T, es, tp = ("d" if store == "f64" else "f"), (8 if store == "f64" else 4), nu > 0
    D = P.pad_dim(d)
    expect = {gam(0): 1} if tp else {}
    if branch == "reg":
        expect.update({reg(T, d, 0, X_PROPOSE_T if tp else X_PROPOSE): 1, ("k_pcn_pack",): 1})
    elif branch == "pad32":
        expect.update({reg(T, 32, 0, X_PROPOSE_PAD_T if tp else X_PROPOSE_PAD): 1, ("k_pcn_pack",): 1})
    elif branch == "mm":
        expect[mm(T, d, 0, MM_XPROPOSE_T if tp else MM_XPROPOSE)] = 1
    elif branch == "rowpad":
        expect.update({("k_pad_rows", T): 1, ("k_pad_tables",): 1, ("k_unpad_rows", T): 1})
        if D in (64, 128):
            expect[mm(T, D, 0, MM_XPROPOSE_T if tp else MM_XPROPOSE)] = 1
        else:
            expect.update({reg(T, D, 0, X_PROPOSE_T if tp else X_PROPOSE): 1, ("k_pcn_pack",): 1})
    else:
        expect[gen(T, pick_vec(d * es, xd, xp), 1)] = 1
    q0, q1 = ran(e, lambda: device_propose(e, xd, xp, mu, L, Linv, rho, nu, seed, gid0, step), expect)
    assert band_intact(xp, pbuf, po) and band_intact(xd, xbuf, xo)
    assert torch.equal(xd.cpu(), torch.as_tensor(x).to(tdt(store)))  # the state is read only
    # (the matrix-core kernels round y' to the storage type in their proposal mode too - |y'|^2 is that y's - where the register
    # and the generic kernel keep it in fp64 until x' is stored: DESIGN.md section 3.19)
    on_mm = branch == "mm" or (branch == "rowpad" and D in (64, 128))
    r64 = P.propose(x, mu, L, Linv, rho, seed, gid0, step, nu, store=st, round_y1=on_mm)
    rld = P.propose(x, mu, L, Linv, rho, seed, gid0, step, nu, ft=np.longdouble, store=st, round_y1=on_mm)
    floor = d * P.EPS64

    def unit(a, b):
        return max(float(np.max(np.abs(a - b) / (1 + np.abs(b)))), floor)

    # fp32 storage: one float32 spacing of x' - and, where y' is rounded as well, of y' through L
    through = float(np.abs(L).sum(axis=1).max()) if on_mm else 0.0
    tol_x = P.MULT * unit(r64["x1"], rld["x1"]) + (P.EPS32 * (1 + through) if store == "f32" else 0.0)
    got = xp.double().cpu().numpy()
    assert np.max(np.abs(got - r64["x1"]) / (1 + np.abs(r64["x1"]))) <= tol_x
    for g, q in ((q0, "q0"), (q1, "q1")):
        want, wl = 2 * P.ref_corr(r64[q], nu, d), 2 * P.ref_corr(rld[q], nu, d)
        assert np.max(np.abs(g - want) / (1 + np.abs(want))) <= P.MULT * unit(want, wl), q


ACCEPT = [  # (d, store, x_prop offset, log-Jacobians, want_count, copy kernel)
    (8, "f64", 0, False, True, "k_copy_flagged_rows16"), (6, "f64", 0, True, False, "k_copy_flagged_rows16"),
    (12, "f32", 0, False, True, "k_copy_flagged_rows16"), (32, "f32", 0, True, True, "k_copy_flagged_rows16"),
    (5, "f64", 0, True, True, "d"), (5, "f32", 0, False, False, "f"), (8, "f64", 1, False, True, "d"), (8, "f32", 2, True, True, "f"),
]


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("d,store,po,jac,want_count,copy", ACCEPT)
def test_accept_vs_restatement(eng, d, store, po, jac, want_count, copy, n):
    """asmc_pcn_accept: the decision on given densities and quadratic forms (second guard with log-Jacobians), the carried values,
    and the flagged row copy - 16-byte pieces with a power-of-two and another piece count per row, the scalar copy for rows that
    are no multiple of 16 bytes or an unaligned x_prop - bit for bit."""
    g = np.random.default_rng(d * 1000 + n + po)
    st = P.STORE[store]
    x = g.normal(size=(n, d)).astype(st).astype(np.float64)
    xq = g.normal(size=(n, d)).astype(st).astype(np.float64)
    old = [g.normal(size=n) * 3 for _ in range(3)]
    new = [g.normal(size=n) * 3 for _ in range(3)]
    new[0][::7], old[1][::5] = -np.inf, -np.inf
    old[0][::11] = np.nan
    new[2][3::13] = np.inf
    q0, q1 = g.chisquare(d, size=n), g.chisquare(d, size=n)
    lj, ljn = (g.normal(size=n), g.normal(size=n)) if jac else (None, None)
    if jac:
        ljn[1::9] = np.inf
    beta, seed, gid0, step = 0.6, 17, 2**40 - 30, 2**32 - 1
    xd, xbuf = banded(eng, x, tdt(store))
    xp, _ = banded(eng, xq, tdt(store), po)
    od = [banded(eng, v, torch.float64) for v in old]
    nd = [eng.asarray(v) for v in new]
    ljd = banded(eng, lj, torch.float64) if jac else (None, None)
    ljnd = eng.asarray(ljn) if jac else None
    T = "d" if store == "f64" else "f"
    expect = {("k_pcn_accept_flags",): 1, (("k_copy_flagged_rows16",) if copy == "k_copy_flagged_rows16" else ("k_copy_flagged_rows", T)): 1}
    nacc = ran(eng, lambda: eng.pcn_accept(xd, xp, od[0][0], od[1][0], od[2][0], nd[0], nd[1], nd[2], eng.asarray(q0), eng.asarray(q1),
                                           beta, seed, gid0, step, ljd[0], ljnd, want_count), expect)
    torch.cuda.synchronize()
    p = dict(q0=q0, q1=q1, log_u=np.log(P.H.accept_uniforms(seed, gid0, n, step)))
    P.accept(p, *old, *new, beta, 0.0, d, lj, ljn)  # (nu = 0: the correction is q / 2, and the entry point takes 2 c)
    pl = dict(q0=q0.astype(np.longdouble), q1=q1.astype(np.longdouble), log_u=np.log(P.H.accept_uniforms(seed, gid0, n, step).astype(np.longdouble)))
    P.accept(pl, *[v.astype(np.longdouble) for v in old], *[v.astype(np.longdouble) for v in new], beta, 0.0, d,
             None if lj is None else lj.astype(np.longdouble), None if ljn is None else ljn.astype(np.longdouble))
    with np.errstate(invalid="ignore"):
        dm = np.abs(p["margin"] - pl["margin"].astype(np.float64))
    tm = P.MULT * max(float(np.nanmax(np.where(np.isfinite(dm), dm, 0.0))), 8 * P.EPS64)
    und = P.razor(p["margin"], tm)
    assert und.sum() <= P.razor_cap(n)
    acc, ok = p["accept"], ~und
    gx = xd.double().cpu().numpy()
    assert np.array_equal(gx[ok & acc], xq[ok & acc]) and np.array_equal(gx[ok & ~acc], x[ok & ~acc])
    for (v, b), o, nw in zip(od, old, new):
        assert band_intact(v, b)
        assert np.array_equal(v.cpu().numpy()[ok], np.where(acc, nw, o)[ok], equal_nan=True)
    if jac:
        assert np.array_equal(ljd[0].cpu().numpy()[ok], np.where(acc, ljn, lj)[ok]) and band_intact(*ljd)
    assert band_intact(xd, xbuf)
    assert acc[ok].any() and (~acc[ok]).any() or n == 1
    if want_count:
        assert abs(nacc - int(acc.sum())) <= und.sum()
    else:
        assert nacc is None


# ---- the whitened-state split session ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in P.CASES if c["env"] == "session"], ids=P.case_id)
def test_session_vs_restatement(eng, c):
    """asmc_pcn_ysplit_begin / propose / accept / end: two steps, the caller's densities evaluated at the stored x' in between, the
    second step with carried and proposed log-Jacobians (+inf planted: the second guard).  Every call's instantiations are
    asserted; x is the session's until it ends; the state, the carried values and the counts against the restatement."""
    inputs, ref, (tx, tc, tm) = P.case_reference(c)
    x, ll, lp, lq, mu, L, Linv, mixes = inputs
    n, d, tp = c["n"], c["d"], c["nu"] > 0
    T, nz = ("d" if c["store"] == "f64" else "f"), int(c["mode"] == "f32")
    xd, xbuf = banded(eng, x, tdt(c["store"]))
    cd = [banded(eng, v, torch.float64) for v in (ll, lp, lq)]
    ljd = banded(eng, P.session_logj(c), torch.float64)
    mud, Ld, Lid = (eng.asarray(v) for v in (mu, L, Linv))
    sess = ran(eng, lambda: eng.pcn_ysplit_begin(xd, c["beta"], mud, Ld, Lid, 4242 + c["seed"], 1000, c["rho"], 0.234, False, c["nu"], c["mode"]),
               {("k_pcn_pack",): 1, reg(T, d, 0, WHITEN_S): 1})
    assert sess is not None
    x0 = xd.clone()
    for t in range(2):
        want = {flow(T, d, nz, FLOW_PROPOSE_SX): 1}
        if tp and t == 0:  # (one draw holds the eight steps from the first)
            want[gam(nz)] = 1
        xp = ran(eng, lambda: eng.pcn_ysplit_propose(sess, 5 + t), want, exclude=())
        xpn = xp.double().cpu().numpy()
        new = [eng.asarray(P.mix_logpdf(m, xpn)) for m in mixes]
        kw = dict(logj=ljd[0], logj_new=eng.asarray(P.sin_jac(xpn))) if t else {}
        ran(eng, lambda: eng.pcn_ysplit_accept(sess, 5 + t, cd[0][0], cd[1][0], cd[2][0], *new, n, t, **kw),
            {flow(T, d, nz, FLOW_ACCEPT_SJ if t else FLOW_ACCEPT_S): 1, ("k_pcn_adapt",): 1}, exclude=())
    assert torch.equal(xd, x0)  # the session owns the state until it ends
    n_acc, hist, rho = ran(eng, lambda: eng.pcn_ysplit_end(sess, 2), {("k_pcn_pack",): 1, reg(T, d, 0, UNWHITEN_XS): 1})
    torch.cuda.synchronize()
    assert band_intact(xd, xbuf) and band_intact(*ljd) and all(band_intact(v, b) for v, b in cd)
    got = dict(x=xd.double().cpu().numpy(), ll=cd[0][0].cpu().numpy(), lp=cd[1][0].cpu().numpy(), lq=cd[2][0].cpu().numpy())
    und = P.compare(got, ref, ref["margins"], tx, tc, tm, label=f'session, {c["store"]} storage, {c["mode"]} noise')
    ok = ~P.razor(ref["margins"], tm)
    glj, rlj = ljd[0].cpu().numpy()[ok], ref["lj"][ok]
    assert np.all(np.isfinite(glj)) and np.max(np.abs(glj - rlj) / (1 + np.abs(rlj))) <= tc
    assert np.all(np.abs(np.asarray(n_acc) - ref["counts"]) <= und), (n_acc, ref["counts"], und)
    assert np.all(np.asarray(hist) == c["rho"]) and rho == c["rho"]
    assert 0 < ref["counts"][1] < n


def test_session_begins_at_its_own_widths_only(eng):
    """asmc_pcn_ysplit_begin returns UNSUPPORTED (the wrapper: None), and launches nothing, at every width but the register
    kernels' own, and at those for an x that is not 16-byte aligned; the set it accepts is pcn_ref.SESSION_DIMS."""
    accepted = set()
    for d in list(range(1, 41)) + [63, 64, 65, 127, 128]:
        for store in ("f64", "f32"):
            x, _, _, _, mu, L, Linv, _ = P.problem(8, d, 1, 1, P.STORE[store])
            xd, _ = banded(eng, x, tdt(store))
            mud, Ld, Lid = (eng.asarray(v) for v in (mu, L, Linv))
            want = {("k_pcn_pack",): 1, reg("d" if store == "f64" else "f", d, 0, WHITEN_S): 1} if d in P.SESSION_DIMS else {}
            sess = ran(eng, lambda: eng.pcn_ysplit_begin(xd, 0.5, mud, Ld, Lid, 1, 0, 0.3), want)
            assert (sess is not None) == (d in P.SESSION_DIMS), (d, store)
            if sess is not None:
                accepted.add(d)
    assert accepted == set(P.SESSION_DIMS)
    x, _, _, _, mu, L, Linv, _ = P.problem(8, 8, 1, 1)
    xd, _ = banded(eng, x, torch.float64, 1)
    assert ran(eng, lambda: eng.pcn_ysplit_begin(xd, 0.5, *(eng.asarray(v) for v in (mu, L, Linv)), 1, 0, 0.3), {}) is None


# ---- Gamma variates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_gamma_draw_batches_and_cache_key(eng, mode, monkeypatch):
    """Nine tpCN steps draw their variates in two launches (eight steps, then one); a call with another n redraws, and so does the
    first n again (the cache holds one (n, seed, gid0, shape, noise, steps) at a time) - each result against the restatement."""
    for n, steps, draws in ((257, 9, 2), (130, 1, 1), (257, 2, 1)):
        c = dict(P._case(8, n, 1, 5.5, steps, "f64", mode, env="ASMC_PCN_XSTATE"), state="x")
        c["seed"] = 31
        inputs, ref, (tx, tc, tm) = P.case_reference(c)
        exp = {("k_pcn_adapt",): steps, gam(mode == "f32"): draws, ("k_pcn_pack",): 1, reg("d", 8, int(mode == "f32"), X_STEP_T): steps}
        monkeypatch.setenv("ASMC_PCN_XSTATE", "1")
        got, n_acc, _, _ = device_mutate(eng, c, inputs, expect=lambda xd: exp)
        und = P.compare(got, ref, ref["margins"], tx, tc, tm)
        assert np.all(np.abs(n_acc - ref["counts"]) <= und)


# ---- edges ------------------------------------------------------------------------------------------------------------------------
PATHS = {  # name -> (d, n_steps, x offset): x-state register, coordinate-major whitened, matrix-core, generic
    "xreg": (8, 1, 0), "soa": (8, 4, 0), "mm": (64, 1, 0), "generic": (8, 1, 1)}


def edge_case(path, n=130, nu=0.0, C=1, **over):
    d, steps, off = PATHS[path]
    c = P._case(d, n, C, nu, steps, offset=off)
    c.update(over)
    c["state"] = P.case_state(d, steps, C, "offset" if off else None)
    c["seed"] = 500 + d + steps + off
    return c


def edge_run(eng, c, change=None, gid0=1000, step0=5, mixes=None):
    """Device and restatement of case `c` with `change(inputs)` applied to the carried values first: (got, ref, inputs, tolerances)."""
    st = P.STORE[c["store"]]
    inputs = list(P.problem(c["n"], c["d"], c["seed"], c["C"], st))
    if mixes is not None:
        inputs[7] = mixes
    if change:
        change(inputs)
    kw = dict(nu=c["nu"], mode=c["mode"], store=st, state=c["state"])
    x, ll, lp, lq, mu, L, Linv, mx = inputs
    seed = 4242 + c["seed"]
    ref = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, c["rho"], mx, seed, gid0, c["n_steps"], step0, **kw)
    rld = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, c["rho"], mx, seed, gid0, c["n_steps"], step0, ft=np.longdouble, **kw)
    tol = P.case_tolerances(c, inputs, ref, rld)
    got, n_acc, _, _ = device_mutate(eng, c, inputs, gid0=gid0, step0=step0)
    und = P.compare(got, ref, ref["margins"], *tol)
    assert np.all(np.abs(n_acc - ref["counts"]) <= und)
    return got, ref, inputs, tol


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_edge_carried_minus_infinity_goes_through_the_guard(eng, path, beta):
    """beta = 0 with ll = -inf (0 * -inf = NaN) and beta = 1 with lq = -inf: the row's old log-target is -inf through the guard and
    its finite proposal is accepted; a carried NaN likewise."""
    def change(inp):
        inp[1 if beta == 0.0 else 3][::3] = -np.inf
        inp[1][1::9] = np.nan

    c = edge_case(path, beta=beta)
    got, ref, inputs, _ = edge_run(eng, c, change)
    hit = np.zeros(c["n"], dtype=bool)
    hit[::3] = True
    assert np.all(ref["margins"][0][hit] == np.inf)  # (the restatement: accepted at the first step, whatever log u)
    assert np.all(np.isfinite(got["ll"][hit])) and np.all(np.isfinite(got["lq"][hit]))
    assert np.all(np.any(got["x"][hit] != inputs[0][hit], axis=1))


@pytest.mark.parametrize("path", ["xreg", "generic", "soa"])
def test_edge_proposal_with_zero_density_is_rejected(eng, path):
    """A likelihood whose quadratic form overflows at every proposal (d = 4, centre 1e200: log-density -inf, cleanly): every row is
    rejected - bit-unchanged on the x-state paths - and rows whose old log-target is -inf as well (both -inf) are rejected too."""
    d = 4
    lik = (np.array([0.0]), np.full((1, d), 1e200), np.ones((1, d)))
    c = dict(P._case(d, 130, 1, 0.0, PATHS[path][1], offset=PATHS[path][2]), beta=0.5)
    c["state"] = P.case_state(d, c["n_steps"], 1, "offset" if c["offset"] else None)
    c["seed"] = 41

    def change(inp):
        inp[7] = [lik, inp[7][1], inp[7][2]]
        inp[1][:] = -3.0     # a finite carried likelihood: the old state wins
        inp[1][::4] = -np.inf  # ... and rows where both sides are -inf

    got, ref, inputs, _ = edge_run(eng, c, change)
    assert ref["counts"].sum() == 0
    if c["state"] == "x":
        assert np.array_equal(got["x"], inputs[0]) and np.array_equal(got["ll"], inputs[1])


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("rho", [1.0, 1e-4])
def test_edge_step_sizes(eng, path, rho):
    """rho = 1: a = 0, nothing of the old state reaches y' (the restatement multiplies by an exact zero too); rho = 1e-4."""
    edge_run(eng, edge_case(path, rho=rho, nu=5.5 if rho == 1.0 else 0.0))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("nu", [1.0, 1e6])
def test_edge_degrees_of_freedom(eng, path, nu):
    """nu = 1 (the heaviest tails the entry point accepts) and nu = 1e6, where the Student-t correction is the Gaussian one to
    q^2 / (4 nu) and the scale still comes from the Gamma variate."""
    got, ref, inputs, (tx, tc, tm) = edge_run(eng, edge_case(path, nu=nu))
    if nu == 1e6:
        q = np.array([1.0, 30.0, 200.0])
        assert np.all(np.abs(P.ref_corr(q, nu, PATHS[path][0]) - 0.5 * q) <= q * q / (4 * nu) + PATHS[path][0] * q / (2 * nu))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("gid0,step0", [(2**32 - 3, 5), (2**40, 5), (1000, 2**32 - 1), (2**64 - 70, 7)])
def test_edge_counter_words(eng, path, gid0, step0):
    """gid0 = 2^32 - 3: the counter's high word changes inside the first tile; 2^40; 2^64 - 70: the index itself wraps inside the
    second tile; step = 2^32 - 1: the four-step path goes on at step 0 (32-bit arithmetic, on the device and in the restatement)."""
    edge_run(eng, edge_case(path, nu=5.5), gid0=gid0, step0=step0)


# ---- adaptation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adapt,n_steps", [(0, 3), (0, 4), (1, 5), (2, 5), (2, 6), (3, 5), (3, 7)])
@pytest.mark.parametrize("path", list(PATHS))
def test_adaptation_vs_restatement(eng, path, adapt, n_steps, monkeypatch):
    """Off, after every step, and lagged by blocks of k = 2, 3 steps (no exchange hook), with calls that end inside a block: accept
    counts, the step size every step used and the one returned, against the restatement and samplers.smc.pcn_adapt ("soa": the
    coordinate-major whitened loop from four steps on).  Step sizes to pcn_ref.rho_tol."""
    from aspire_amd.samplers.smc import pcn_adapt

    d, _, off = PATHS[path]
    c = P._case(d, 300, 1, 5.5 if adapt == 2 else 0.0, n_steps, offset=off, env="ASMC_PCN_XSTATE" if path == "xreg" else None)
    c["state"] = P.case_state(d, n_steps, 1, "offset" if off else c["env"])
    c["seed"] = 900 + 100 * list(PATHS).index(path) + 10 * n_steps + adapt  # (a seed per case: see pcn_ref._cases)
    st = P.STORE[c["store"]]
    inputs = P.problem(c["n"], d, c["seed"], 1, st)
    x, ll, lp, lq, mu, L, Linv, mx = inputs
    kw = dict(nu=c["nu"], store=st, state=c["state"], target=0.3, adapt=adapt)
    ref = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, c["rho"], mx, 4242 + c["seed"], 1000, n_steps, 5, **kw)
    rld = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, c["rho"], mx, 4242 + c["seed"], 1000, n_steps, 5, ft=np.longdouble, **kw)
    tol = P.case_tolerances(c, inputs, ref, rld)
    assert not P.razor(ref["margins"], tol[2]).any()  # (seeds chosen on the CPU: no row the restatement cannot call)
    if c["env"]:
        monkeypatch.setenv(c["env"], "1")
    got, n_acc, hist, rho = device_mutate(eng, c, inputs, adapt=adapt, target=0.3)
    P.compare(got, ref, ref["margins"], *tol)
    assert np.array_equal(n_acc, ref["counts"])
    rt = P.rho_tol(ref["rho_hist"])
    np.testing.assert_allclose(hist, ref["rho_hist"], rtol=rt, atol=0)
    assert rho == pytest.approx(ref["rho"], rel=rt, abs=0)
    if adapt == 1:
        r = c["rho"]
        for t in range(n_steps):
            assert hist[t] == pytest.approx(r, rel=rt, abs=0)
            r = pcn_adapt(r, n_acc[t] / c["n"], 0.3, t)
    if adapt >= 2:
        for t in range(n_steps):
            assert hist[t] == hist[t - t % adapt]


@pytest.mark.parametrize("rho0,target,lo", [(0.985, 0.0, False), (1.0002e-4, 1.0, True)])
def test_adaptation_clips(eng, rho0, target, lo):
    """The adapted step size stops at 0.99 and at 1e-4."""
    c = dict(P._case(8, 130, 1, 0.0, 2, rho=rho0), state="x")
    c["seed"] = 5
    inputs = list(P.problem(130, 8, 5, 1))
    if lo:
        inputs[1] = inputs[1] + np.where(np.arange(130) % 2 == 0, 50.0, 0.0)  # half the rows sit on a target no proposal reaches
        c["beta"] = 1.0
    x, ll, lp, lq, mu, L, Linv, mx = inputs
    ref = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, rho0, mx, 4242 + c["seed"], 1000, 2, 5, target=target, adapt=1)
    rld = P.mutate(x, ll, lp, lq, c["beta"], mu, L, Linv, rho0, mx, 4242 + c["seed"], 1000, 2, 5, ft=np.longdouble, target=target, adapt=1)
    tol = P.case_tolerances(c, inputs, ref, rld)
    assert not P.razor(ref["margins"], tol[2]).any()  # (seed chosen on the CPU: no row the restatement cannot call)
    got, n_acc, hist, rho = device_mutate(eng, c, inputs, adapt=True, target=target)
    assert ref["rho"] == (1e-4 if lo else 0.99) and rho == ref["rho"] and hist[1] == ref["rho"]
    assert np.array_equal(n_acc, ref["counts"])
    P.compare(got, ref, ref["margins"], *tol)


# ---- error returns ----------------------------------------------------------------------------------------------------------------
def _mutate_error(e, n, d, store="f64", rho=0.4, nu=0.0, n_steps=1, match=None):
    from aspire_amd._lib import AsmcError

    x = torch.zeros((n, d), dtype=tdt(store), device=e.device)
    z = [torch.zeros(n, dtype=torch.float64, device=e.device) for _ in range(3)]
    eye = e.asarray(np.eye(d))
    mix = e.make_mixture([0.0], np.zeros((1, d)), np.ones((1, d)))
    e.profile(True)
    try:
        with pytest.raises(AsmcError, match=match):
            e.pcn_mutate(x, *z, 0.5, e.asarray(np.zeros(d)), eye, eye, mix, mix, mix, 1, 0, rho, n_steps, 0, 0.234, False, "f64", nu)
        var = {s: c for s, c in e.profile_variants().items() if any(f in s for f in FAMILIES)}
    finally:
        e.profile(False)
    assert not var, var  # nothing was launched
    assert bool((x == 0).all())


def test_error_returns_launch_nothing(eng, big):
    for kw in (dict(rho=0.0), dict(rho=1.5), dict(nu=0.5), dict(nu=1e-9), dict(n_steps=0), dict(n_steps=2049)):
        _mutate_error(eng, 65, 8, match=r"rc=-1", **kw)
    _mutate_error(big, big.n_max + 1, 8, match=r"rc=-1")
    # the smallest d whose generic tile does not fit LDS, from the launcher's own expression: UNSUPPORTED, with and without a
    # Gamma draw in front
    budget = 160 * 1024 - 1024 - 384 * 16
    for store, es in (("f64", 8), ("f32", 4)):
        per_wave = lambda d: 64 * (((d * es + 7) & ~7) + 16) + 64 * 8 * d
        d_bad = next(d for d in range(129, 257) if per_wave(d) > budget)
        assert d_bad == {"f64": 153, "f32": 203}[store] and per_wave(d_bad - 1) <= budget
        for nu in (0.0, 5.5):
            _mutate_error(big, 65, d_bad, store, nu=nu, match=r"rc=-4")
            _propose_error(big, 65, d_bad, store, nu)


def _propose_error(e, n, d, store, nu):
    """asmc_pcn_propose at a width whose generic tile does not fit LDS: UNSUPPORTED (-4) with nothing launched - the parent drew
    a tpCN call's Gamma variates first - and x_prop untouched."""
    x = torch.zeros((n, d), dtype=tdt(store), device=e.device)
    xp = torch.full((n, d), SENT, dtype=tdt(store), device=e.device)
    q = [torch.zeros(n, dtype=torch.float64, device=e.device) for _ in range(2)]
    eye, mu = e.asarray(np.eye(d)), e.asarray(np.zeros(d))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    e.profile(True)
    try:
        rc = e.lib.asmc_pcn_propose(e._ctx, n, d, e._xdt(x), ptr(x), ptr(xp), ptr(q[0]), ptr(q[1]), ptr(mu), ptr(eye), ptr(eye), 0.4,
                                    float(nu), 1, 0, 0, e._stream)
        var = {s: c for s, c in e.profile_variants().items() if any(f in s for f in FAMILIES)}
    finally:
        e.profile(False)
    assert rc == -4 and not var, (rc, var)
    assert bool((xp == SENT).all())


def test_largest_width_that_fits_lds_runs(big):
    """d = 152 in fp64: the last width below the limit above, one wave per block."""
    c = dict(P._case(152, 65, 1, 5.5, 1, env="big"), state="x")
    c["seed"] = 3
    check_case(big, c, None)


# ---- closing: every reachable instantiation of the table ran ----------------------------------------------------------------------
def test_every_instantiation_of_the_table_ran():
    print(f"{len(TABLE)} instantiations in the table; worst device error over its tolerance, (positions, densities):")
    for label, w in sorted(P.WORST.items(), key=str):
        print(f"  {label}: {w[0]:.3g}, {w[1]:.3g}")
    missing = sorted(k for k in TABLE if k not in SEEN)
    assert not missing, missing
    assert set(SEEN) <= TABLE
