"""The stand-alone flow kernels of csrc/asmc_flow.hip and csrc/asmc_flow16.hip - density (asmc_coupling_logprob) and draw
(asmc_coupling_sample) of coupling and autoregressive flows - on every dispatch path and at the edges, row by row against the same
fp32 parameters evaluated in fp64 (tests/flow_ref.py; tolerances: its header and DESIGN.md section 3.25, none from a device's output).

Every case enables profiling, runs, asserts from profile_variants() the template instantiation that ran and how often, and keeps a
sentinel band behind everything the kernels write.  The closing test asserts that the cases together saw every reachable instantiation.

Which shape takes which kernel (dispatch_flow, dispatch_maf, asmc_coupling_sample in csrc/asmc_flow.hip; asmc_flow_layout,
asmc_flow16_logprob, asmc_flow16_sample in csrc/asmc_flow16.hip):

  layout 0, coupling: even d <= 32   k_coupling_logprob<16, W, XT, 512, TPW, HS>, k_coupling_sample<16, W, XT, 512>; W = 32 / 64 / 128.
                                     H = 16 for EVERY supported d (flow_half_pad(d <= 32) = 16): a 32-row tile per wave, eight waves.
                                     d = 32 reads its rows with 16-byte vector loads, every other d coordinate by coordinate.  The
                                     layers stay in LDS while they fit 150 KB (width 64: up to 5 layers, two blocks per CU up to 2;
                                     width 128: one layer), otherwise the density streams them layer by layer and the draw refuses.
  layout 0, autoregressive: d <= 32, W = 32 / 64
                                     k_maf_logprob<32, W, XT, 512, HS>, k_maf_sample<32, W, XT, 512>; both affine forms (a run-time
                                     argument of the density kernel's layers, a compile-time one inside them)
  layout 1: coupling 32 < d <= 128 (even), autoregressive 32 < d <= 128 and width 128 at ANY d
                                     k_flow16_logprob<KIND, D, W, XT, 512>, k_flow16_sample<KIND, D, W, XT, 512>; D = 64 for d <= 64,
                                     else 128; 16-row groups, weights streamed through two LDS slots

Switches: XT = double / float by the rows' type.  ASMC_FLOW_MATH=f32 (read at every launch) selects HS = false, the fp32-MFMA chain, in
k_coupling_logprob and k_maf_logprob; the draws and layout 1 have split-fp16 layers only and refuse.  ASMC_FLOW_TPW=2 (read once per
process: a child process here) selects k_coupling_logprob<16, 32 | 64, XT, 512, 2, false>: two tiles per wave, no prefetch, fp32 MFMA.
ASMC_MAF_SAMPLE_ALL_PASSES takes the fixed-point exit out of the autoregressive draws (a kernel argument, not an instantiation).

Compiled but unreachable: k_coupling_logprob<32, ..> and k_coupling_sample<32, ..> (flow_supported admits d <= 32 and flow_half_pad
then gives 16), and k_maf_logprob / k_maf_sample<32, 128, ..> (width 128 takes layout 1 at any d).  The spline flow has its own
kernels and its own module (test_gpu_nsf.py) and is not in this table.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import flow_ref as F

pytestmark = pytest.mark.gpu

FAMILIES = ("k_coupling_logprob", "k_coupling_sample", "k_maf_logprob", "k_maf_sample", "k_flow16_logprob", "k_flow16_sample")
SENT = 777.25  # guard-band value (exact in fp32)
GUARD = 70     # elements (rows of x) behind row n: more than a tile
SEEN = {}      # (kernel, template arguments) -> launches the module's asserted runs have covered
TABLE = F.reachable()


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A HIP fault is sticky: every later call on the device fails with it.  End the session there instead of running on."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device fault: {exc}", returncode=3)


def sym(name, targs):
    return f"_Z{len(name)}{name}I{targs}E"


def ran(eng, fn, expect):
    """fn() with the assertion that, of the six flow kernels, exactly the instantiations `expect` ran ({(name, template arguments):
    launches}; {} = nothing was launched)."""
    eng.profile(True)
    try:
        out = fn()
        var = {s: c for s, c in eng.profile_variants().items() if any(f"{len(f)}{f}I" in s for f in FAMILIES)}
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


def tdt(dt):
    return torch.float64 if dt == "f64" else torch.float32


def banded(eng, shape, dtype):
    """A zero tensor of `shape` on the device inside a buffer of the sentinel, GUARD rows behind it: (view, whole buffer)."""
    numel = int(np.prod(shape))
    row = shape[1] if len(shape) == 2 else 1
    buf = torch.full((numel + GUARD * row,), SENT, dtype=dtype, device=eng.device)
    view = buf[:numel].view(shape)
    view.zero_()
    return view, buf


def band_intact(view, buf):
    return bool((buf[view.numel():] == SENT).all())


def kind_of(key):
    return F.COUPLING if key[0] == "coupling" else F.MAF


def device_flow(eng, p):
    dev = p.flow.device_coupling(eng)
    assert dev.kind == kind_of(p.key) and dev.affine == int(p.key[0] == "softclip")
    assert eng.lib.asmc_flow_layout(dev.kind, dev.dims, dev.hidden) == F.layout(dev.kind, dev.dims, dev.hidden)
    return dev


def logprob_rc(eng, dev, xd, out, x_dtype=None):
    cs = dev.c_struct()
    return eng.lib.asmc_coupling_logprob(eng._ctx, xd.shape[0], eng._xdt(xd) if x_dtype is None else x_dtype, ctypes.c_void_p(xd.data_ptr()),
                                         ctypes.byref(cs), ctypes.c_void_p(out.data_ptr()), eng._stream)


def sample_rc(eng, dev, n, x, lq, seed, gid0, draw_id, x_dtype=None):
    cs = dev.c_struct()
    return eng.lib.asmc_coupling_sample(eng._ctx, n, eng._xdt(x) if x_dtype is None else x_dtype, ctypes.byref(cs), seed, gid0, draw_id,
                                        ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(lq.data_ptr()), eng._stream)


def device_logprob(eng, dev, x, dt, expect):
    """asmc_coupling_logprob through the ABI: the rows in a buffer that ends at row n, `out` inside the sentinel."""
    from aspire_amd._lib import check

    xd = torch.as_tensor(x, dtype=tdt(dt)).to(eng.device).contiguous()
    assert xd.numel() == x.size and np.array_equal(xd.double().cpu().numpy(), x, equal_nan=True)  # (the pool's rows are exact in the row type)
    out, buf = banded(eng, (x.shape[0],), torch.float64)
    ran(eng, lambda: check(logprob_rc(eng, dev, xd, out), "asmc_coupling_logprob"), expect)
    torch.cuda.synchronize()
    assert band_intact(out, buf), "log q: written behind row n"
    return out.cpu().numpy()


def device_sample(eng, dev, n, dt, seed, gid0, draw_id, expect):
    from aspire_amd._lib import check

    x, xbuf = banded(eng, (n, dev.dims), tdt(dt))
    lq, lbuf = banded(eng, (n,), torch.float64)
    ran(eng, lambda: check(sample_rc(eng, dev, n, x, lq, seed, gid0, draw_id), "asmc_coupling_sample"), expect)
    torch.cuda.synchronize()
    assert band_intact(x, xbuf), "x: written behind row n"
    assert band_intact(lq, lbuf), "log q: written behind row n"
    return x.double().cpu().numpy(), lq.cpu().numpy()


def check_density(p, got, x, ref, big, label):
    """Row by row against the judge: the NaN rows are the judge's (plus the out-of-range row of the split-fp16 paths), an infinite
    log q is the judge's, every other row is within the bound - the neighbours of the planted rows among them."""
    yard = F.yardstick(p)
    assert yard[0] <= F.YARD_CAP, (label, yard)
    nan_want = np.isnan(ref)
    if big is not None:
        nan_want[big] = True
    assert np.array_equal(np.isnan(got), nan_want), (label, np.flatnonzero(np.isnan(got) != nan_want))
    inf = np.isinf(ref) & ~nan_want
    assert np.array_equal(got[inf], ref[inf]), (label, got[inf], ref[inf])
    keep = ~nan_want & ~inf
    return F.check_errors(F.err(got[keep], ref[keep]), yard, F.DENSITY_FLOOR, label)


def density_case(eng, key, dt, wide, n, math, rows=F.POOL_ROWS, expect_tpw=1):
    p = F.pool(*key, rows=rows, dtype=dt, wide=wide)
    dev = device_flow(eng, p)
    hs = math == "split" and expect_tpw == 1
    x, big = p.x[:n], None
    if n >= 128:
        x, big = F.plant(x, p.flow, hs)
        if dt == "f32":
            x = x.astype(np.float32).astype(np.float64)
        if hs:  # the row times 1e6 is out of the fp16 operand range in a coordinate every flow here conditions on
            assert abs(x[big, 0] - float(p.flow.loc[0])) > 1e5 * float(p.flow.scale[0])
        ref = p.ref[:n].copy()
        ref[100:104] = F.judge(p.flow, x[100:104])
    else:
        ref = p.ref[:n]
    r = F.route(dev.kind, dev.dims, dev.hidden, "logprob", "d" if dt == "f64" else "f", math, expect_tpw)
    got = device_logprob(eng, dev, x, dt, {r: 1})
    return check_density(p, got, x, ref, big, f"density {r[0]}<{r[1]}> {p.label} n={n}")


@pytest.mark.parametrize("case", F.density_cases(), ids=F.case_id)
def test_density_vs_fp64(eng, monkeypatch, case):
    """One case per reachable instantiation of the three density kernels and more: widths, row types, split-fp16 and fp32-MFMA
    chains, both affine forms, resident and streamed layers, both load branches, padded dims, wide scales; row counts round one
    tile, group and block.  From 128 rows on with planted NaN, +inf, -inf and out-of-range rows."""
    key, dt, wide, n, math = case
    if math == "f32":
        monkeypatch.setenv("ASMC_FLOW_MATH", "f32")
    density_case(eng, key, dt, wide, n, math)


def num_cu(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


@pytest.mark.parametrize("name", [k for k in F.SECOND_ROUND if "logprob" in k])
def test_density_second_round_of_the_grid_stride_loop(eng, name):
    """One round of the capped grid plus 4097 rows: every block goes round its loop again, the last round is ragged and leaves
    most waves without a tile (k_coupling_logprob: the prefetch guard; streamed: the block-wide barriers of a wave without rows;
    k_flow16_logprob: the shared weight stream at the round seam).  Every row is compared."""
    key, dt = F.SECOND_ROUND[name]
    kernel = name.split()[0]
    n = F.rows_per_round(kernel, F.build_flow(*key), num_cu(eng)) + F.TAIL
    if kernel == "k_coupling_logprob":
        assert F.coupling_resident(key[2], key[3]) == ("resident" in name)
    assert n <= eng.n_max and n <= 150_000
    density_case(eng, key, dt, False, n, "split", rows=n)


def test_density_two_tiles_per_wave_in_a_child_process(eng, tmp_path):
    """ASMC_FLOW_TPW is read once per process: a fresh child runs widths 32 and 64, both row types, 63 / 64 / 65 / 4099 rows, asserts
    the TPW = 2 instantiation and compares with the judge itself; its census and measurements join this process's."""
    path = str(tmp_path / "tpw2.json")
    env = dict(os.environ, ASMC_FLOW_TPW="2")
    env.pop("ASMC_FLOW_MATH", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tpw2-child", path], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    child = json.load(open(path))
    for name, targs, cnt in child["seen"]:
        assert (name, targs) in TABLE and targs.endswith("Li2ELb0E")
        SEEN[(name, targs)] = SEEN.get((name, targs), 0) + cnt
    assert len(child["seen"]) == 4 and all(cnt == len(F.TPW_ROWS) for _, _, cnt in child["seen"]), child["seen"]
    for line in child["record"]:
        print(line)
    F.RECORD.extend(child["record"])


# ---- draws -------------------------------------------------------------------------------------------------------------------------
def check_draw(p, dt, x, lq, seed, gid0, draw_id, label, rows=None):
    """x against the fp64 inverse at the restated latent (rows: on these rows only), log q against the judge at the returned rows."""
    n, d = x.shape
    f32 = dt == "f32"
    kind = kind_of(p.key)
    z = F.latent(seed, gid0, n, draw_id, d, kind=kind, rows=rows)
    x_ref, _ = F.draw_ref(p.flow, z)
    worst = F.compare_draw(x if rows is None else x[rows], x_ref, F.x_tolerance(p), f32=f32, label=label)
    assert np.all(np.isfinite(lq)), label
    ref = F.judge(p.flow, x)
    e = F.err(lq, ref)
    if f32:  # the density was formed before x was rounded
        e = np.maximum(e - F.f32_rounding_shift(p.flow, x) / np.maximum(np.abs(ref), 1.0), 0.0)
    dy = F.draw_yardstick(p)
    assert dy[0] <= F.YARD_CAP, (label, dy[:2])
    F.check_errors(e, dy[:2], F.DRAW_FLOOR, f"{label} [x: {worst:.2f} of its tolerance]")


@pytest.mark.parametrize("case", F.draw_cases(), ids=F.case_id)
def test_draw_vs_the_generator_and_fp64(eng, case):
    """Every reachable instantiation of the three draw kernels: the returned rows are the fp64 inverse of the flow at the latent the
    counter-based generator gives particle gid0 + i (coordinate j = element j % 4 of quad j / 4), the returned log q is the fp64
    density at the returned rows; particle indices above 2^32 and across the wrap of 2^64, draw ids 0 and 2^32 - 1."""
    key, dt, wide, n, (gid0, draw_id) = case
    p = F.pool(*key, dtype=dt, wide=wide)
    dev = device_flow(eng, p)
    r = F.route(dev.kind, dev.dims, dev.hidden, "sample", "d" if dt == "f64" else "f")
    x, lq = device_sample(eng, dev, n, dt, F.DRAW_SEED, gid0, draw_id, {r: 1})
    check_draw(p, dt, x, lq, F.DRAW_SEED, gid0, draw_id, f"draw {r[0]}<{r[1]}> {p.label} n={n} gid0={gid0} id={draw_id}")


def weakened(flow):
    """The flow with its transforms' last layers x 0.02: the shape of a trained flow near its initialisation, whose fixed-point
    iteration ends long before d passes."""
    import copy

    from aspire_amd.flows import _MaskedLinear

    f = copy.deepcopy(flow)
    with torch.no_grad():
        for layer in f.layers:
            [m for m in layer.net if isinstance(m, _MaskedLinear)][-1].weight.mul_(0.02)
    f._version += 1
    f._packed = None
    return f


@pytest.mark.parametrize("name", [k for k in F.SECOND_ROUND if "sample" in k])
def test_draw_second_round_of_the_grid_stride_loop(eng, monkeypatch, name):
    """One round of the capped grid plus 4097 rows.  log q on every row; x on the first tile, the rows either side of every block
    boundary of round one and of the round seam, and the last 100 rows (the autoregressive fp64 inverse is sequential in d).
    Autoregressive flows: the fixed-point exit (wave-wide in k_maf_sample, block-wide in k_flow16_sample, whose waves then redirect
    the shared weight stream) returns the bits of ASMC_MAF_SAMPLE_ALL_PASSES, for the pool's flow and for a weakly coupled one."""
    key, dt = F.SECOND_ROUND[name]
    kernel = name.split()[0]
    per_round = F.rows_per_round(kernel, F.build_flow(*key), num_cu(eng))
    n = per_round + F.TAIL
    assert n <= eng.n_max and n <= 150_000
    p = F.pool(*key, rows=n, dtype=dt)
    dev = device_flow(eng, p)
    r = F.route(dev.kind, dev.dims, dev.hidden, "sample", "d" if dt == "f64" else "f")
    gid0, draw_id = F.DRAW_KEYS[2]  # the particle index wraps inside the first tile
    x, lq = device_sample(eng, dev, n, dt, F.DRAW_SEED, gid0, draw_id, {r: 1})
    block = 8 * (16 if kernel.startswith("k_flow16") else 32)
    edges = np.arange(block, per_round, block)
    rows = np.unique(np.concatenate([np.arange(32), edges - 1, edges, np.arange(per_round - 2, per_round + 2), np.arange(n - 100, n)]))
    assert rows.size <= 2500
    check_draw(p, dt, x, lq, F.DRAW_SEED, gid0, draw_id, f"draw, second round {r[0]}<{r[1]}> {p.label} n={n}", rows=rows)
    if key[0] == "coupling":
        return
    weak = weakened(p.flow).device_coupling(eng)
    xw, lqw = device_sample(eng, weak, n, dt, F.DRAW_SEED, gid0, draw_id, {r: 1})
    assert np.all(np.isfinite(lqw)) and not np.array_equal(xw, x)
    monkeypatch.setenv("ASMC_MAF_SAMPLE_ALL_PASSES", "1")
    xa, lqa = device_sample(eng, dev, n, dt, F.DRAW_SEED, gid0, draw_id, {r: 1})
    xwa, lqwa = device_sample(eng, weak, n, dt, F.DRAW_SEED, gid0, draw_id, {r: 1})
    assert np.array_equal(xa, x) and np.array_equal(lqa, lq), "the fixed-point exit changed the draw"
    assert np.array_equal(xwa, xw) and np.array_equal(lqwa, lqw), "the fixed-point exit changed the draw of the weakly coupled flow"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refused(eng, call, rc_want, text):
    rc = ran(eng, call, {})
    assert rc == rc_want, (rc, eng.lib.asmc_last_error())
    assert text in eng.lib.asmc_last_error().decode(), eng.lib.asmc_last_error()


REFUSED_DRAWS = [(("coupling", 18, 2, 32), "fp32 MFMA chain was asked for"), (("maf", 17, 2, 32), "fp32 MFMA chain was asked for"),
                 (("coupling", 66, 2, 32), "ASMC_FLOW_MATH=f32 is not available there"), (("maf", 12, 2, 128), "ASMC_FLOW_MATH=f32 is not available there")]


@pytest.mark.parametrize("key,text", REFUSED_DRAWS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_a_draw_under_the_fp32_chain_is_refused(eng, monkeypatch, key, text):
    dev = device_flow(eng, F.pool(*key))
    x, xbuf = banded(eng, (40, dev.dims), torch.float64)
    lq, lbuf = banded(eng, (40,), torch.float64)
    monkeypatch.setenv("ASMC_FLOW_MATH", "f32")
    refused(eng, lambda: sample_rc(eng, dev, 40, x, lq, 1, 0, 0), -4, text)
    assert not x.any() and not lq.any() and band_intact(x, xbuf) and band_intact(lq, lbuf)


@pytest.mark.parametrize("key", [("coupling", 66, 2, 32), ("maf", 65, 2, 32), ("maf", 12, 2, 128)], ids=lambda k: "-".join(map(str, k)))
def test_layout_1_density_under_the_fp32_chain_is_refused(eng, monkeypatch, key):
    p = F.pool(*key)
    dev = device_flow(eng, p)
    xd = eng.asarray(p.x[:40])
    out, buf = banded(eng, (40,), torch.float64)
    monkeypatch.setenv("ASMC_FLOW_MATH", "f32")
    refused(eng, lambda: logprob_rc(eng, dev, xd, out), -4, "ASMC_FLOW_MATH=f32 is not available there")
    assert not out.any() and band_intact(out, buf)


def test_other_refusals(eng):
    """A coupling draw whose layers exceed the resident limit (width 64, 6 layers: the density streams them, the draw does not), a
    row type that is neither, the soft-clipped affine form on a coupling flow: the documented error, nothing launched."""
    p = F.pool("coupling", 32, 6, 64)
    dev = device_flow(eng, p)
    assert not F.coupling_resident(6, 64)
    x, _ = banded(eng, (40, 32), torch.float64)
    lq, _ = banded(eng, (40,), torch.float64)
    refused(eng, lambda: sample_rc(eng, dev, 40, x, lq, 1, 0, 0), -4, "must be resident in LDS together")
    xd = eng.asarray(p.x[:40])
    for key in (("coupling", 18, 2, 32), ("maf", 17, 2, 32), ("coupling", 66, 2, 32)):
        q = F.pool(*key)
        dv = device_flow(eng, q)
        xq, _ = banded(eng, (40, dv.dims), torch.float64)
        refused(eng, lambda: logprob_rc(eng, dv, xq, lq, x_dtype=7), -1, "bad x_dtype")
        refused(eng, lambda: sample_rc(eng, dv, 40, xq, lq, 1, 0, 0, x_dtype=7), -1, "bad x_dtype")
    import copy

    soft = copy.copy(device_flow(eng, F.pool("coupling", 18, 2, 32)))
    soft.affine = 1
    x18, _ = banded(eng, (40, 18), torch.float64)
    refused(eng, lambda: logprob_rc(eng, soft, x18, lq), -1, "bad affine form")
    refused(eng, lambda: sample_rc(eng, soft, 40, x18, lq, 1, 0, 0), -1, "bad affine form")
    assert not lq.any() and not xd.isnan().any()


# ---- census ------------------------------------------------------------------------------------------------------------------------
def test_census_every_reachable_instantiation_ran():
    """Closing test: the cases above, this process's and the child's, saw every instantiation some shape, row type or switch reaches."""
    missing = sorted(TABLE - set(SEEN))
    print(f"flow kernels: {len(SEEN)} of {len(TABLE)} reachable instantiations ran, {sum(SEEN.values())} asserted launches")
    assert not missing, missing


# ---- the ASMC_FLOW_TPW=2 child -----------------------------------------------------------------------------------------------------
def _tpw2_child(path):
    from aspire_amd.engine import HipEngine

    assert os.environ.get("ASMC_FLOW_TPW") == "2"
    e = HipEngine(0, n_max=1 << 16, d_max=32)
    for key, dt in F.TPW_CASES:
        for n in F.TPW_ROWS:
            density_case(e, key, dt, False, n, "split", rows=max(F.TPW_ROWS), expect_tpw=2)
    torch.cuda.synchronize()
    json.dump(dict(seen=[[k[0], k[1], c] for k, c in SEEN.items()], record=F.RECORD), open(path, "w"))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--tpw2-child":
    _tpw2_child(sys.argv[2])
