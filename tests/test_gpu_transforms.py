"""asmc_transform_forward / _inverse (csrc/asmc_transform.hip) on every dispatch path and at the edges of the domain, against the
host restatement of the reference's CompositeTransform (tests/transform_ref.py: an fp64 run, which is the reference's own
arithmetic, and an mpmath run) and the C oracle.

Shape -> path (launch_transform; s = bytes per element, a row is d s bytes; the cases that go through `launch` assert the
instantiation that ran, from profile_variants):

  flat   k_transform_flat<T, DIR, HINTS>   d s / 16 a power of two <= 64, 16-byte aligned rows:
                                           fp64 d = 2, 8, 32, 128; fp32 d = 4, 32, 256; HINTS = the table's ASMC_TR_NO_* bits or 0
  tiled  k_transform<T, 16, DIR, 0>        d s % 16 == 0 otherwise: fp64 d = 6, 48, 100, 126 (4, 2, 1, 1 waves per block);
                                           fp32 d = 12, 96, 252
         k_transform<T, 8, DIR, 0>         d s % 8 == 0 otherwise: fp64 d = 1, 3, 33; fp32 d = 2, 6; 8-byte aligned views of rows that
                                           would take 16
         k_transform<T, 4, DIR, 0>         the rest: fp32 d = 1, 7, 33; 4-byte aligned views
         k_transform<T, 16, DIR, d>        ASMC_TRANSFORM_TILED=1 at d = 8, 16, 32, 64, 128 (fp64 d = 128 has no tile: an error)
         k_transform<T, 16, DIR, 0>        ... with ASMC_TRANSFORM_GENERIC=1 as well
  error  "row too long for one LDS tile"   a tiled row of more than 1008 bytes: fp64 d = 127, 130, 255, 256; fp32 d = 254

Tolerances.  Against the oracle and the fp64 run (bulk shapes): 1e-12 relative + 1e-12 on values, 1e-12 + 1e-11 on log|det J|, as
test_gpu_parity.py has them.  Against the mpmath run (edge groups): with E the largest gap, in fp64 ulps of the mpmath value,
between the fp64 run and the mpmath run over the case's inputs - the conditioning of the expression plus the error of numpy's own
functions - an element may differ from the mpmath value by 8 E + 4 ulps, and a row's log|det J| by 8 E_lj + 4 d ulps of
sum |terms| + |constants|, E_lj measured on the row sums in the same unit.  fp32 storage: the restatement runs on the fp32-rounded
inputs and an element may differ by half an fp32 ulp more (one rounding of an fp64-accurate value); the Jacobians are fp64.  No
tolerance comes from the device's output.  Every case prints its E, its tolerance and the device's largest error (pytest -s).
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import transform_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = R.EPS
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def make(eng, tab, hints=None):
    kind, per, lo, up, mean, std = tab
    unit, aff = R.constants(kind, lo, up, std)
    t = eng.make_transform(kind, per, lo, up, mean, std, EPS, float(unit), float(aff))
    return t if hints is None else dataclasses.replace(t, hints=hints)


def flat_sym(dt, inverse, hints):
    return f"_Z16k_transform_flatI{'d' if dt == F64 else 'f'}Li{int(inverse)}ELi{hints}EEv"


def tiled_sym(dt, inverse, vec, dcomp=0):
    return f"_Z11k_transformI{'d' if dt == F64 else 'f'}Li{vec}ELi{int(inverse)}ELi{dcomp}EEv"


def launch(eng, xt, t, inverse, symbol):
    """The transform of xt through the engine, with the assertion that exactly the instantiation `symbol` ran."""
    eng.profile(True)
    try:
        out, lj = (eng.transform_inverse if inverse else eng.transform_forward)(xt, t)
        var = {s: c for s, c in eng.profile_variants().items() if "k_transform" in s}
    finally:
        eng.profile(False)
    assert len(var) == 1 and next(iter(var)).startswith(symbol) and next(iter(var.values())) == 1, (symbol, var)
    return out.double().cpu().numpy(), lj.cpu().numpy()


def rounded(x, dt):
    """x as the device sees it (rounded to the storage type), as an fp64 array and as a device-ready tensor."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dt)
    return xt.double().numpy(), xt


def half_ulp32(ref):
    """Half the fp32 spacing at the fp64 magnitude of ref: 2^(floor(log2 |ref|) - 24), fp32's subnormal spacing below 2^-126."""
    with np.errstate(all="ignore"):
        a = np.abs(np.asarray(ref, dtype=np.float64))
        e = np.where(np.isfinite(a) & (a > 0), np.frexp(np.where(np.isfinite(a) & (a > 0), a, 1.0))[1] - 1, -126)
        return np.where(np.isfinite(a), np.ldexp(1.0, np.maximum(e, -126) - 24), 0.0)


def check_bulk(got, got_lj, ref, ref_lj, dt, what):
    """1e-12 / 1e-11 against an fp64 reference, the same non-finite pattern; fp32 storage: half an fp32 ulp more."""
    assert R.same_nonfinite(got, ref) and R.same_nonfinite(got_lj, ref_lj), what
    fin, finj = np.isfinite(ref), np.isfinite(ref_lj)
    tol = 1e-12 * np.abs(ref[fin]) + 1e-12 + (half_ulp32(ref[fin]) if dt == F32 else 0.0)
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= tol), (what, float(np.max(err - tol)))
    np.testing.assert_allclose(got_lj[finj], ref_lj[finj], rtol=1e-12, atol=1e-11, err_msg=what)


def check_hp(got, got_lj, tab, x, inverse, dt, what, rows=slice(None)):
    """The 8 E + 4 rule of the module docstring against the mpmath run, on x[rows]."""
    kind, per, lo, up, mean, std = tab
    d = len(kind)
    x, got, got_lj = x[rows], got[rows], got_lj[rows]
    y64, lj64, _ = R.composite(x, *tab, EPS, inverse)
    yh, ljh, th = R.composite(x, *tab, EPS, inverse, ft=LD)
    assert R.same_nonfinite(got, y64) and R.same_nonfinite(got_lj, lj64), (what, "non-finite pattern")
    fin, finj = np.isfinite(yh), np.isfinite(ljh)
    E = R.gap_ulps(y64, yh)
    tol = (8 * E + 4) * R.ulp64(yh) + (half_ulp32(yh) if dt == F32 else 0.0)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - yh).astype(np.float64)
    unit, aff = R.constants(kind, lo, up, std, ft=LD)
    mag = R.ulp64(np.abs(np.where(np.isfinite(th), th, 0)).sum(-1) + abs(unit) + abs(aff))
    E_lj = R.gap_ulps(lj64, ljh, unit=mag)
    tol_lj = (8 * E_lj + 4 * d) * mag
    with np.errstate(all="ignore"):
        err_lj = np.abs(got_lj.astype(LD) - ljh).astype(np.float64)
    worst = float(np.max(err[fin] / R.ulp64(yh)[fin])) if fin.any() else 0.0
    worst_lj = float(np.max(err_lj[finj] / mag[finj])) if finj.any() else 0.0
    print(f"TOL {what}: E={E:.3g} allowed={8 * E + 4:.3g} device={worst:.3g} ulps | log|J|: E={E_lj:.3g} "
          f"allowed={8 * E_lj + 4 * d:.3g} device={worst_lj:.3g} ulps of sum|terms|")
    assert np.all(err[fin] <= tol[fin]), (what, "values", worst, 8 * E + 4)
    assert np.all(err_lj[finj] <= tol_lj[finj]), (what, "log|J|", worst_lj, 8 * E_lj + 4 * d)
    return np.where(fin, tol, 0.0), np.where(finj, tol_lj, 0.0)


def path_of(d, dt):
    """(kind of path, VEC) launch_transform takes for aligned rows of d elements."""
    rb = d * (8 if dt == F64 else 4)
    pieces = rb // 16
    if rb % 16 == 0 and 1 <= pieces <= 64 and pieces & (pieces - 1) == 0:
        return "flat", 16
    return "tiled", 16 if rb % 16 == 0 else 8 if rb % 8 == 0 else 4


def symbol_for(t, d, dt, inverse, vec=None, dcomp=None):
    path, v = path_of(d, dt)
    if dcomp is not None:
        return tiled_sym(dt, inverse, 16, dcomp)
    if vec is not None:
        return tiled_sym(dt, inverse, vec)
    return flat_sym(dt, inverse, t.hints & 7) if path == "flat" else tiled_sym(dt, inverse, v)


def both_directions(eng, oracle, tab, n, dt, hints=None, edges=True, view=None, vec=None, dcomp=None, seed=0):
    """Forward and inverse of a table at [n, d] against the fp64 run and the oracle; returns the device results."""
    d = len(tab[0])
    t = make(eng, tab, hints)
    out = []
    for inverse in (False, True):
        x, xt = rounded(R.interior_x(tab, n, inverse, seed=seed, edges=edges), dt)
        xd = xt.to(eng.device) if view is None else view(xt)
        got, got_lj = launch(eng, xd, t, inverse, symbol_for(t, d, dt, inverse, vec, dcomp))
        what = f"d={d} n={n} {dt} inverse={inverse}"
        y, lj, _ = R.composite(x, *tab, EPS, inverse)
        check_bulk(got, got_lj, y, lj, dt, what + " vs fp64 run")
        yo, ljo = oracle.transform(x, *tab, EPS, inverse=inverse)
        check_bulk(got, got_lj, yo, ljo, dt, what + " vs oracle")
        out.append((got, got_lj))
    return out


# ---- (a) every dispatch path ------------------------------------------------------------------------------------------------------
FLAT = [(2, F64), (8, F64), (32, F64), (128, F64), (4, F32), (32, F32), (256, F32)]
TILED16 = [(6, F64), (48, F64), (100, F64), (126, F64), (12, F32), (96, F32), (252, F32)]
TILED8 = [(1, F64), (3, F64), (33, F64), (2, F32), (6, F32)]
TILED4 = [(1, F32), (7, F32), (33, F32)]


def _ids(shapes):
    return [f"{'f64' if dt == F64 else 'f32'}-d{d}" for d, dt in shapes]


@pytest.mark.parametrize("mix", ["logit_mix", "probit_mix"])
@pytest.mark.parametrize("d,dt", FLAT + TILED16 + TILED8 + TILED4, ids=_ids(FLAT + TILED16 + TILED8 + TILED4))
def test_every_default_path_vs_fp64_run_and_oracle(eng, oracle, d, dt, mix):
    """Bounded, periodic and untouched coordinates side by side with the affine stage, interior points and finite edge values,
    n = 257 (five tiles, the last one ragged)."""
    assert path_of(d, dt) == ("flat", 16) if (d, dt) in FLAT else path_of(d, dt)[0] == "tiled"
    both_directions(eng, oracle, R.table(mix, d), 257, dt)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("d,dt", [(8, F64), (4, F32), (6, F64), (3, F64), (7, F32)], ids=_ids([(8, F64), (4, F32), (6, F64), (3, F64), (7, F32)]))
def test_row_counts_around_one_tile(eng, oracle, d, dt, n):
    both_directions(eng, oracle, R.table("logit_mix", d), n, dt)


@pytest.mark.parametrize("zero_hints", [False, True], ids=["hints", "hints0"])
@pytest.mark.parametrize("name", ["logit", "probit", "periodic", "affine", "logit_mix", "probit_affine"])
@pytest.mark.parametrize("d,dt", [(8, F64), (32, F32)], ids=_ids([(8, F64), (32, F32)]))
def test_flat_kernel_table_compositions(eng, oracle, d, dt, name, zero_hints):
    """Each composition selects another HINTS instantiation of the flat kernel (branches compiled out); hints = 0 runs the same table
    through the instantiation with every branch, and the two must agree bit for bit."""
    tab = R.table(name, d)
    t = make(eng, tab)
    want = {"logit": 1 | 4, "probit": 1 | 2, "periodic": 2 | 4, "affine": 7, "logit_mix": 4, "probit_affine": 1 | 2}[name]
    assert t.hints == want
    res = both_directions(eng, oracle, tab, 257, dt, hints=0 if zero_hints else None)
    if zero_hints:
        ref = both_directions(eng, oracle, tab, 257, dt)
        for (a, alj), (b, blj) in zip(res, ref):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(alj, blj)


def _offset_view(eng, off):
    def view(xt):
        n, d = xt.shape
        buf = torch.empty(n * d + off, dtype=xt.dtype, device=eng.device)
        v = buf[off:].view(n, d)
        v.copy_(xt)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v

    return view


@pytest.mark.parametrize("d,dt,off,vec", [(3, F64, 3, 8), (3, F32, 3, 4), (6, F64, 1, 8), (8, F64, 1, 8), (12, F32, 2, 8), (12, F32, 1, 4),
                                         (4, F32, 1, 4)])
def test_misaligned_rows_take_the_narrower_copies(eng, oracle, d, dt, off, vec):
    """Rows that start `off` elements into a 16-byte aligned buffer (off = d = 3: the rows x[1:] of a tensor): the 16-byte copies and
    the flat kernel are ruled out by the pointer, not by the row length."""
    both_directions(eng, oracle, R.table("logit_mix", d), 257, dt, view=_offset_view(eng, off), vec=vec)


DT_SHAPES = [(d, dt) for d in (8, 16, 32, 64, 128) for dt in (F64, F32) if (d, dt) != (128, F64)]


@pytest.mark.parametrize("generic", [False, True], ids=["compile-time-d", "generic"])
@pytest.mark.parametrize("d,dt", DT_SHAPES, ids=_ids(DT_SHAPES))
def test_tiled_forms_behind_the_environment_switches(eng, oracle, monkeypatch, d, dt, generic):
    """ASMC_TRANSFORM_TILED=1 (read at every launch) sends flat-kernel shapes to the tiled kernel with d as a compile-time
    constant; ASMC_TRANSFORM_GENERIC=1 on top of it to the run-time-d form."""
    monkeypatch.setenv("ASMC_TRANSFORM_TILED", "1")
    if generic:
        monkeypatch.setenv("ASMC_TRANSFORM_GENERIC", "1")
    both_directions(eng, oracle, R.table("probit_mix" if d == 16 else "logit_mix", d), 257, dt, dcomp=0 if generic else d)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_flat_compile_time_d_and_generic_forms_agree(eng, monkeypatch, dt):
    """One input with NaN and +-inf in it through the three kernels that serve d = 32: each within the 8 E + 4 rule of the mpmath
    run and within twice that of each other, and the same non-finite pattern."""
    d = 32
    tab = R.table("logit_mix", d)
    t = make(eng, tab)
    for inverse in (False, True):
        x, xt = rounded(R.poke_nonfinite(R.interior_x(tab, 64, inverse, edges=True)), dt)
        res = [launch(eng, xt.to(eng.device), t, inverse, flat_sym(dt, inverse, t.hints))]
        with monkeypatch.context() as m:
            m.setenv("ASMC_TRANSFORM_TILED", "1")
            res.append(launch(eng, xt.to(eng.device), t, inverse, tiled_sym(dt, inverse, 16, d)))
            m.setenv("ASMC_TRANSFORM_GENERIC", "1")
            res.append(launch(eng, xt.to(eng.device), t, inverse, tiled_sym(dt, inverse, 16, 0)))
        for name, (got, got_lj) in zip(("flat", "compile-time-d", "generic"), res):
            tol, tol_lj = check_hp(got, got_lj, tab, x, inverse, dt, f"three-forms {name} {dt} inverse={inverse}")
            assert R.same_nonfinite(got, res[0][0]) and R.same_nonfinite(got_lj, res[0][1])
        for (a, alj), (b, blj) in ((res[0], res[1]), (res[0], res[2]), (res[1], res[2])):
            fin, finj = np.isfinite(a), np.isfinite(alj)
            a, b, alj, blj = (np.where(np.isfinite(v), v, 0.0) for v in (a, b, alj, blj))  # (the patterns are equal: checked above)
            assert np.all(np.abs(a - b)[fin] <= 2 * tol[fin]) and np.all(np.abs(alj - blj)[finj] <= 2 * tol_lj[finj])


def _raw(eng, inverse, xt, out, lj, t):
    cs = t.c_struct()
    fn = eng.lib.asmc_transform_inverse if inverse else eng.lib.asmc_transform_forward
    return fn(eng._ctx, xt.shape[0], eng._xdt(xt), ctypes.c_void_p(xt.data_ptr()), ctypes.c_void_p(out.data_ptr()),
              ctypes.c_void_p(lj.data_ptr()), ctypes.byref(cs), eng._stream)


@pytest.mark.parametrize("d,dt,tiled", [(127, F64, False), (130, F64, False), (255, F64, False), (256, F64, False), (254, F32, False),
                                       (128, F64, True)])
def test_rows_too_long_for_a_tile_are_refused(eng, monkeypatch, d, dt, tiled):
    """A host-side argument check before any launch: the library's error, "row too long" in asmc_last_error, nothing written.
    (fp64 d = 128 is served by the flat kernel alone: ASMC_TRANSFORM_TILED=1 leaves it without a kernel.)"""
    from aspire_amd._lib import AsmcError

    if tiled:
        monkeypatch.setenv("ASMC_TRANSFORM_TILED", "1")
    tab = R.table("logit", d)
    t = make(eng, tab)
    xt = rounded(R.interior_x(tab, 65, False), dt)[1].to(eng.device)
    for inverse in (False, True):
        out, lj = torch.full_like(xt, -7.0), torch.full((65,), -7.0, dtype=F64, device=eng.device)
        assert _raw(eng, inverse, xt, out, lj, t) != 0
        assert "row too long" in eng.lib.asmc_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((lj == -7.0).all())
        with pytest.raises(AsmcError, match="row too long"):
            (eng.transform_inverse if inverse else eng.transform_forward)(xt, t)


# ---- (b) the second pass of each grid-stride loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,mix", [(128, "logit_mix"), (6, "probit_mix")], ids=["flat-d128", "tiled-d6"])
def test_second_pass_of_the_grid_stride_loop(eng, oracle, d, mix):
    """More rows than one pass of the capped grid covers (flat: num_cu * 32 blocks of 256 threads, 64 threads per d = 128 row;
    tiled: num_cu * 8 blocks of 4 tiles of 64 rows), twice over plus a ragged tail: every row against the oracle, the last 128 -
    second pass and tail - against the mpmath run."""
    num_cu = torch.cuda.get_device_properties(eng.device).multi_processor_count
    per_pass = num_cu * 32 * 256 // 64 if d == 128 else num_cu * 8 * 4 * 64
    n = 2 * per_pass + 37
    tab = R.table(mix, d)
    t = make(eng, tab)
    for inverse in (False, True):
        x = R.interior_x(tab, n, inverse)
        got, got_lj = launch(eng, torch.as_tensor(x).to(eng.device), t, inverse, symbol_for(t, d, F64, inverse))
        yo, ljo = oracle.transform(x, *tab, EPS, inverse=inverse)
        check_bulk(got, got_lj, yo, ljo, F64, f"second pass d={d} inverse={inverse}")
        check_hp(got, got_lj, tab, x, inverse, F64, f"second-pass d={d} inverse={inverse}", rows=slice(n - 128, n))


# ---- (c), (e) edge values against the mpmath run ------------------------------------------------------------------------------------
EDGE_SHAPES = [(8, F64), (6, F64), (4, F32), (12, F32)]  # flat, tiled, flat, tiled
EDGE_NAMES = sorted(R.edge_cases(2))


@pytest.mark.parametrize("name", EDGE_NAMES)
@pytest.mark.parametrize("d,dt", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_edge_values_vs_mpmath(eng, d, dt, name):
    """On, outside and within eps of the bounds; far, negative and +-0 periodic arguments; saturating and clamped inverse
    arguments; probit tails; mixed-sign affine tables over six decades; NaN and +-inf in one coordinate of rows 3, 20 and 37, where
    the non-finite pattern must be the restatement's, the other coordinates and the neighbouring rows correct (the flat kernel
    sums a row's Jacobian terms across lanes) and the neighbours' Jacobians finite."""
    tab, x, inverse = R.edge_cases(d)[name]
    x, xt = rounded(x, dt)
    t = make(eng, tab)
    got, got_lj = launch(eng, xt.to(eng.device), t, inverse, symbol_for(t, d, dt, inverse))
    check_hp(got, got_lj, tab, x, inverse, dt, f"{name} d={d} {'f64' if dt == F64 else 'f32'}")
    if "nonfinite" in name:
        clean = np.ones(len(x), dtype=bool)
        clean[[r for r, _ in R.NONFINITE]] = False
        assert np.isfinite(got[clean]).all() and np.isfinite(got_lj[clean]).all()


# ---- (d) bit-exact claims ----------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


SPECIALS = [0.0, -0.0, 5e-324, -2.2250738585072014e-308, 1.7976931348623157e308, np.inf, -np.inf, np.nan, 1.0, -1e-30]


@pytest.mark.parametrize("d,dt", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_untouched_coordinates_pass_through_bit_for_bit(eng, d, dt):
    """kind 0, not periodic, no affine stage - next to coordinates that are transformed (logit_mix without its affine stage) and
    in a table that touches nothing - in both directions, zeros' signs, denormals, infinities and NaN included."""
    g = np.random.default_rng(d)
    for name in ("logit_mix", "none"):
        tab = R.table(name, d)[:4] + (None, None)
        idle = (tab[0] == 0) & (tab[1] == 0)
        assert idle.any()
        t = make(eng, tab)
        for inverse in (False, True):
            x = R.interior_x(tab, 70, inverse)
            x[:, idle] = np.where(g.uniform(size=(70, int(idle.sum()))) < 0.3, g.choice(SPECIALS, size=(70, int(idle.sum()))), x[:, idle])
            xt = torch.as_tensor(x).to(dt).to(eng.device)
            out, _ = (eng.transform_inverse if inverse else eng.transform_forward)(xt, t)
            np.testing.assert_array_equal(_bits(out.cpu().numpy()[:, idle]), _bits(xt.cpu().numpy()[:, idle]))


@pytest.mark.parametrize("d", [8, 6], ids=["flat", "tiled"])
def test_periodic_wrap_equals_numpys_bit_for_bit(eng, d):
    """lower + np.mod(x - lower, w): fmod is exact, the rest is one subtraction and one addition."""
    tab = R.table("periodic", d)
    lo, up = tab[2], tab[3]
    g = np.random.default_rng(3)
    x = np.concatenate([R.periodic_edge_x(lo, up), lo + (up - lo) * g.uniform(-3, 3, size=(200, d)),
                        lo + (up - lo) * g.integers(-5, 5, size=(40, d)), 10.0 ** g.uniform(-20, 20, size=(40, d)) * g.choice([-1, 1], size=(40, d))])
    t = make(eng, tab)
    for inverse in (False, True):
        out, lj = (eng.transform_inverse if inverse else eng.transform_forward)(torch.as_tensor(x).to(eng.device), t)
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(lo + np.mod(x - lo, up - lo)))
        assert bool((lj == 0.0).all())


@pytest.mark.parametrize("d", [128, 126], ids=["flat", "tiled"])
def test_affine_forward_quotient_is_numpys_bit_for_bit(eng, d):
    """(v - mean) / std: the flat kernel's three-FMA quotient from the stored reciprocal claims correct rounding, the tiled kernel
    divides.  25 tables of d divisors x 32 rows: > 100 000 quotients, |a / b| and |b| log-uniform in [1e-100, 1e100], both signs;
    every other table with mean = 0, so that the numerator is the input itself."""
    g = np.random.default_rng(d)
    sign = lambda s: g.choice([-1.0, 1.0], size=s)  # noqa: E731
    kind = per = np.zeros(d, dtype=np.int32)
    total = 0
    for k in range(25):
        std = sign(d) * 10.0 ** g.uniform(-100, 100, size=d)
        q = sign((32, d)) * 10.0 ** g.uniform(-100, 100, size=(32, d))
        mean = np.zeros(d) if k % 2 == 0 else sign(d) * 10.0 ** g.uniform(-100, 100, size=d)
        x = q * std + mean
        t = make(eng, (kind, per, np.zeros(d), np.ones(d), mean, std))
        assert path_of(d, F64)[0] == ("flat" if d == 128 else "tiled")
        out, _ = eng.transform_forward(torch.as_tensor(x).to(eng.device), t)
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits((x - mean) / std))
        total += x.size
    assert total >= 100_000


# ---- (f) in place --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dt", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_in_place_equals_out_of_place_bit_for_bit(eng, d, dt):
    """include/asmc.h: "z_dev == x_dev is allowed"."""
    tab = R.table("logit_mix", d)
    t = make(eng, tab)
    for inverse in (False, True):
        xt = rounded(R.interior_x(tab, 257, inverse, edges=True), dt)[1].to(eng.device)
        out, lj = (eng.transform_inverse if inverse else eng.transform_forward)(xt, t)
        buf, lj2 = xt.clone(), torch.empty(257, dtype=F64, device=eng.device)
        assert _raw(eng, inverse, buf, buf, lj2, t) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(buf.cpu().numpy()), _bits(out.cpu().numpy()))
        np.testing.assert_array_equal(_bits(lj2.cpu().numpy()), _bits(lj.cpu().numpy()))
