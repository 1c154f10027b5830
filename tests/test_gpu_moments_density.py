"""The population moments (asmc_colsum, asmc_centered_gram, asmc_mean_gram*, asmc_colsum_dev, asmc_centered_gram_dev), the device-side
reference fit (asmc_reference_factor*) and the built-in densities (asmc_mixture_logpdf, asmc_mixture_logpdf_premap,
asmc_gaussian_draw) of csrc/asmc_moments.hip, csrc/asmc_density.hip and csrc/asmc_pcn_mm.hip on every dispatch path and at the edges, against the long-double
restatement of tests/moments_ref.py.

Shape -> path (s = bytes per element; every case that names an instantiation asserts, from profile_variants, that it ran):

  Gram  k_gram_stream<T, 32 | 64>     d = 32, 64, 16-byte aligned rows (default)
        k_gram_mm<T, 128>             d = 128, aligned
        k_pad_rows<T> + one of those  every other d <= 128: the zero-padded copy (d = 1 .. 127; views at any offset)
        k_gram_rb<T, 4>               ASMC_GRAM_GENERIC=1, d s % 16 == 0, d <= 32: fp64 d = 2, 12, 32; fp32 d = 4, 12, 32
        k_gram_rb<T, 8>               ... 32 < d <= 128: fp64 d = 48, 64, 100 (four quadrants), 128 (two waves); fp32 d = 36, 100, 128
        k_gram<T>                     misaligned d = 32, 64 (default); ASMC_GRAM_GENERIC=1 and d s % 16 != 0, d <= 64
        k_gram_mm<T, 32 | 64>         ASMC_GRAM_LDS32=1 (read once per process: a child process)
        error                         misaligned d = 128; fp64 d = 65 under ASMC_GRAM_GENERIC=1
  sums  k_colsum<T>                   every d <= 256 (d > 128: an engine with d_max = 256)
  mixture  k_mixture_flat<T, 1 | 4>   d s / 16 a power of two <= 64, aligned, C = 1 | C <= 4: fp64 d = 2, 8, 32, 128; fp32 d = 4, 32, 256
           k_mixture_logpdf<T, 16>    d s % 16 == 0 otherwise, C > 4 or ASMC_MIXTURE_TILED=1: fp64 d = 6, 48, 100, 256; fp32 d = 12, 96
           k_mixture_logpdf<T, 8>     d s % 8 == 0: fp64 d = 1, 3, 33 and 8-byte-offset views; fp32 d = 2, 6
           k_mixture_logpdf<float, 4> fp32 d = 1, 7, 33 and 4-byte-offset views
           premap                     the flat kernel only; anything else is ASMC_ERR_UNSUPPORTED
  draw  k_gaussian_draw<T>, k_gaussian_logq<T>   any d <= 256
  fit   k_ref_factor                  d <= 128: 256 threads for d <= 32, 1024 above

Tolerances (moments_ref.py; none comes from the device's output): column sum j: n u sum_i |x_ij|; Gram entry
(j, k): (n + 4) u sum_i |a_ij| |a_ik| with a = fl(x - c); mean_gram: plus the exact effect of a centre off by the column sum's
tolerance / n_mean; mixture row: (d + 8) u max_c (|logw_c| + q_c / 2) + 4 ulp of the result (+ with a premap one ulp of a x + b per
coordinate through 2 |t - mu| prec + 2 |h t|, and sum |h| t^2 inside the magnitude); reference factor: 8 E + 4 ulps per entry, E the
gap between numpy's fp64 factor and the long-double one on the same covariance.  u = 2^-53.  fp32 rows are the restatement's input
as the device stores them; the outputs are fp64 and earn nothing extra.  The non-finite pattern of every output must be the
restatement's exactly, and every finite element is compared.  Every case prints its tolerance and the device's worst error in
units of it (pytest -s).

Measured on an MI355X, worst error in units of its tolerance: column sums 0.22; Gram 0.24 at n <= 65, 3.8e-4 .. 1.5e-3 at n >= 5003 on
every kernel, 3.0e-3 at the 1e6 offset, 4.9e-4 with the device's own centre; mixture 0.17 .. 0.21 on every kernel, with and without a
premap; Gaussian draw 1.0 for fp32 rows (the rounding to fp32 itself), 0.027 for fp64, its log q 0.11; reference factor at condition
1e10: E = 1.0e8 .. 4.2e10 (L), 7.9e7 .. 5.5e11 (Linv) ulps for d = 4 .. 128, the device at 0.58 (L) and 0.20 (Linv) of 8 E + 4; on the
jitter ladder 0.68 / 0.43 (E = 17 .. 6.6e5 for d > 1), with a negative mean(diag) 0.29 / 0.46; mu 0.50 of its one ulp.  The LDS-tile form has
the stream kernel's bits at d = 32 and at d = 64, n = 5003; at d = 64, n = 70001 the two run on different grids and the bits differ.
Total time of the module: 16 s for 361 cases (the child process 3.6 s).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import moments_ref as M

pytestmark = pytest.mark.gpu
LD = M.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_gram", "k_colsum", "k_pad_rows", "k_mixture", "k_gaussian", "k_ref_factor")


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(scope="module")
def eng256():
    """Column sums above d = 128 need a ctx of that width: a small one of its own."""
    from aspire_amd.engine import HipEngine

    e = HipEngine(0, n_max=1 << 16, d_max=256)
    yield e
    e.close()


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def tname(f32):
    return "f" if f32 else "d"


def sym_stream(f32, d):
    return f"_Z13k_gram_streamI{tname(f32)}Li{d}EEv"


def sym_mm(f32, d):
    return f"_Z9k_gram_mmI{tname(f32)}Li{d}EEv"


def sym_rb(f32, blk):
    return f"_Z9k_gram_rbI{tname(f32)}Li{blk}EEv"


def sym_gram(f32):
    return f"_Z6k_gramI{tname(f32)}Ev"


def sym_pad(f32):
    return f"_Z10k_pad_rowsI{tname(f32)}Ev"


def sym_colsum(f32):
    return f"_Z8k_colsumI{tname(f32)}Ev"


def sym_flat(f32, cmax):
    return f"_Z14k_mixture_flatI{tname(f32)}Li{cmax}EEv"


def sym_tiled(f32, vec):
    return f"_Z16k_mixture_logpdfI{tname(f32)}Li{vec}EEv"


def sym_mm_for(f32, d):
    """The matrix-core kernel of an aligned d in {32, 64, 128} in the default environment."""
    return sym_mm(f32, 128) if d == 128 else sym_stream(f32, d)


def ran(eng, fn, expect):
    """fn() with the assertion that, of the kernel families of this module, exactly the instantiations `expect` ran, each once
    (a symbol prefix -> launches)."""
    eng.profile(True)
    try:
        out = fn()
        var = {s: c for s, c in eng.profile_variants().items() if any(f in s for f in FAMILIES) and "reduce" not in s}
    finally:
        eng.profile(False)
    for s, c in var.items():
        assert any(s.startswith(e) for e in expect), (s, expect)
    for e, cnt in expect.items():
        assert sum(c for s, c in var.items() if s.startswith(e)) == cnt, (e, cnt, var)
    return out


def dev(eng, x, f32, off=0):
    """x on the device in its storage type; off > 0: rows that start `off` elements into an aligned buffer."""
    import torch

    xt = torch.as_tensor(x).to(torch.float32 if f32 else torch.float64)
    if not off:
        v = xt.to(eng.device).contiguous()
        assert v.data_ptr() % 16 == 0
        return v
    n, d = xt.shape
    buf = torch.empty(n * d + off, dtype=xt.dtype, device=eng.device)
    v = buf[off:].view(n, d)
    v.copy_(xt)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@functools.lru_cache(maxsize=None)
def gram_ref(n, d, kind, f32):
    x = M.population(n, d, kind, f32=f32)
    c = M.centre(x)
    g, mag, s1 = M.centered_gram(x, c)
    s, sa = M.colsum(x)
    return x, c, g, mag, s1, s, sa


def ids(f32):
    return "f32" if f32 else "f64"


def gram_case(eng, n, d, f32, expect, kind="bulk", off=0):
    x, c, g, mag, _, _, _ = gram_ref(n, d, kind, f32)
    xd = dev(eng, x, f32, off)
    got = ran(eng, lambda: eng.centered_gram(xd, c), expect)
    M.compare(got, g, M.tol_gram(n, mag), f"gram {kind} {n}x{d} {ids(f32)} off={off} {sorted(expect)}")
    return got


BOTH = pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])


# ---- (a) Gram paths -------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("d", [32, 64, 128])
def test_gram_stream_and_matrix_core_kernels(eng, d, f32):
    gram_case(eng, 5003, d, f32, {sym_mm_for(f32, d): 1})


@BOTH
@pytest.mark.parametrize("n", [1, 3, 4, 5, 31, 32, 33, 63, 64, 65])
def test_gram_row_counts_around_one_group_and_one_tile(eng, n, f32):
    """Fewer rows than one MFMA group (4) or one 32-row tile, and one more: the kernel's zero-filled tail."""
    gram_case(eng, n, 32, f32, {sym_stream(f32, 32): 1})


@BOTH
@pytest.mark.parametrize("n,d", [(70001, 32), (70001, 64), (20001, 128)])
def test_gram_second_grid_stride_pass(eng, n, d, f32):
    """More rows than one pass of the capped grid covers on 256 CUs: 8 blocks per CU of 32 rows at d = 32 / 64 (65 536 rows), 2 per
    CU at d = 128 (16 384)."""
    gram_case(eng, n, d, f32, {sym_mm_for(f32, d): 1})


@BOTH
@pytest.mark.parametrize("d", [1, 2, 3, 12, 31, 33, 48, 65, 100, 127])
def test_gram_zero_padded_copy(eng, d, f32):
    D = 32 if d <= 32 else 64 if d <= 64 else 128
    gram_case(eng, 5003, d, f32, {sym_pad(f32): 1, sym_mm_for(f32, D): 1})


@BOTH
@pytest.mark.parametrize("d", [12, 100])
def test_gram_zero_padded_copy_of_offset_views(eng, d, f32):
    """Rows one element (8 bytes, 4 for fp32) into an aligned buffer: the copy reads them element by element."""
    D = 32 if d <= 32 else 128
    gram_case(eng, 5003, d, f32, {sym_pad(f32): 1, sym_mm_for(f32, D): 1}, off=1)


@pytest.mark.parametrize("d,f32", [(2, False), (12, False), (32, False), (4, True), (12, True), (32, True)])
def test_gram_register_blocked_4(eng, monkeypatch, d, f32):
    monkeypatch.setenv("ASMC_GRAM_GENERIC", "1")
    gram_case(eng, 5003, d, f32, {sym_rb(f32, 4): 1})


@pytest.mark.parametrize("d,f32", [(48, False), (64, False), (100, False), (128, False), (36, True), (100, True), (128, True)])
def test_gram_register_blocked_8(eng, monkeypatch, d, f32):
    """d = 100: two quadrants a side, the last one padded; d = 128: two waves per block."""
    monkeypatch.setenv("ASMC_GRAM_GENERIC", "1")
    gram_case(eng, 5003, d, f32, {sym_rb(f32, 8): 1})


@BOTH
@pytest.mark.parametrize("d", [32, 64])
def test_gram_generic_kernel_serves_misaligned_rows(eng, d, f32):
    gram_case(eng, 5003, d, f32, {sym_gram(f32): 1}, off=1)


@pytest.mark.parametrize("d,f32", [(1, False), (3, False), (33, False), (63, False), (1, True), (7, True), (33, True), (62, True)])
def test_gram_generic_kernel_behind_the_switch(eng, monkeypatch, d, f32):
    monkeypatch.setenv("ASMC_GRAM_GENERIC", "1")
    gram_case(eng, 5003, d, f32, {sym_gram(f32): 1})


def test_gram_shapes_without_a_kernel_are_refused(eng, monkeypatch):
    from aspire_amd._lib import AsmcError

    x, c = gram_ref(65, 128, "bulk", False)[:2]
    with pytest.raises(AsmcError, match="unaligned rows are supported for d <= 64 only"):
        eng.centered_gram(dev(eng, x, False, off=1), c)
    monkeypatch.setenv("ASMC_GRAM_GENERIC", "1")
    x, c = gram_ref(65, 65, "bulk", False)[:2]
    with pytest.raises(AsmcError, match="unaligned rows are supported for d <= 64 only"):
        eng.centered_gram(dev(eng, x, False), c)


@BOTH
@pytest.mark.parametrize("d", [32, 48, 128])
def test_gram_of_offset_data(eng, d, f32):
    """x = 1e6 + N(0, 1): the same tolerance formula - the centred products are of order one, an uncentred kernel's are 1e12."""
    D = 32 if d <= 32 else 64 if d <= 64 else 128
    gram_case(eng, 5003, d, f32, {sym_mm_for(f32, D): 1, **({sym_pad(f32): 1} if D != d else {})}, kind="offset")


LDS32_CASES = [(n, d, f32) for n in (5003, 70001) for d in (32, 64) for f32 in (False, True)]


def lds32_child(path):
    """The body of the child process of the test below (ASMC_GRAM_LDS32 is read once per process)."""
    from aspire_amd.engine import HipEngine

    eng = HipEngine(0, n_max=1 << 17, d_max=128)
    out = {}
    for n, d, f32 in LDS32_CASES:
        x, c = gram_ref(n, d, "bulk", f32)[:2]
        xd = dev(eng, x, f32)
        out[f"g_{n}_{d}_{int(f32)}"] = ran(eng, lambda: eng.centered_gram(xd, c), {sym_mm(f32, d): 1})
    np.savez(path, **out)


def test_gram_lds_tile_form_in_a_child_process(eng, tmp_path):
    """k_gram_mm<T, 32> and <T, 64> behind ASMC_GRAM_LDS32=1, against the restatement and against the default path's
    k_gram_stream, whose comment claims the same bits where both run on the same grid."""
    path = str(tmp_path / "lds32.npz")
    env = dict(os.environ, ASMC_GRAM_LDS32="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lds32-child", path], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    child = np.load(path)
    num_cu = __import__("torch").cuda.get_device_properties(eng.device).multi_processor_count
    for n, d, f32 in LDS32_CASES:
        x, c, g, mag = gram_ref(n, d, "bulk", f32)[:4]
        lds = child[f"g_{n}_{d}_{int(f32)}"]
        M.compare(lds, g, M.tol_gram(n, mag), f"gram LDS-tile form {n}x{d} {ids(f32)}")
        stream = gram_case(eng, n, d, f32, {sym_stream(f32, d): 1})
        same = bool(np.array_equal(lds.view(np.int64), stream.view(np.int64)))
        # the same grid: always at d = 32; at d = 64 while 2 blocks per CU (the LDS form's cap) hold every 32-row tile
        same_grid = d == 32 or (n + 31) // 32 <= 2 * num_cu
        print(f"LDS32 {n}x{d} {ids(f32)}: bit-identical to k_gram_stream: {same} (same grid: {same_grid})")
        if same_grid:
            assert same, (n, d, f32)
        elif num_cu == 256:  # other grids, other block partials: the comment on k_gram_stream says the last bits differ there
            assert not same, (n, d, f32)


@BOTH
@pytest.mark.parametrize("d", [32, 64, 128, 48])
def test_mean_gram_against_the_restatement(eng, d, f32):
    """The centre is the device's own sum / n_mean: against the restatement around ITS centre, with the effect of the centres'
    difference added to the tolerance.  n_mean != n (a shard of a larger population)."""
    n, n_mean = 5003, 6007
    x, _, _, _, _, s, sa = gram_ref(n, d, "bulk", f32)
    xd = dev(eng, x, f32)
    D = d if d in (32, 64, 128) else 64
    expect = {sym_colsum(f32): 1, sym_mm_for(f32, D): 1, **({sym_pad(f32): 1} if D != d else {})}
    gs, gg = ran(eng, lambda: eng.mean_gram(xd, n_mean), expect)
    M.compare(gs, s, M.tol_colsum(n, sa), f"mean_gram sums {n}x{d} {ids(f32)}")
    c_ref = (s / LD(n_mean)).astype(np.float64)
    g, mag, s1 = M.centered_gram(x, c_ref)
    M.compare(gg, g, M.tol_mean_gram(n, n_mean, mag, s1, sa), f"mean_gram gram {n}x{d} {ids(f32)}")


@BOTH
@pytest.mark.parametrize("d", [32, 64, 128])
def test_device_resident_moments_against_the_restatement(eng, d, f32):
    n, n_mean = 5003, 6007
    x, _, _, _, _, s, sa = gram_ref(n, d, "bulk", f32)
    xd = dev(eng, x, f32)
    s_d = ran(eng, lambda: eng.colsum_dev(xd), {sym_colsum(f32): 1})
    M.compare(s_d.cpu().numpy(), s, M.tol_colsum(n, sa), f"colsum_dev {n}x{d} {ids(f32)}")
    g_d = ran(eng, lambda: eng.centered_gram_dev(xd, s_d, n_mean), {sym_mm_for(f32, d): 1})
    c_ref = (s / LD(n_mean)).astype(np.float64)
    g, mag, s1 = M.centered_gram(x, c_ref)
    M.compare(g_d.cpu().numpy(), g, M.tol_mean_gram(n, n_mean, mag, s1, sa), f"centered_gram_dev {n}x{d} {ids(f32)}")


# ---- (b) column sums ------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [1, 7, 5003])
@pytest.mark.parametrize("d", [1, 3, 32, 100, 128, 129, 200, 256])
def test_colsum(eng, eng256, d, n, f32):
    e = eng if d <= 128 else eng256
    x = M.population(n, d, f32=f32)
    s, sa = M.colsum(x)
    xd = dev(e, x, f32)
    got = ran(e, lambda: e.colsum(xd), {sym_colsum(f32): 1})
    M.compare(got, s, M.tol_colsum(n, sa), f"colsum {n}x{d} {ids(f32)}")


# ---- (c) mixture paths ----------------------------------------------------------------------------------------------------------------
def mixture_path(d, f32, C, off=0, tiled=False):
    """The instantiation mixture_logpdf_impl picks."""
    rb = d * (4 if f32 else 8)
    pieces = rb // 16
    if rb % 16 == 0 and not off and pieces & (pieces - 1) == 0 and 1 <= pieces <= 64 and C <= 4 and not tiled:
        return sym_flat(f32, 1 if C == 1 else 4)
    ob = off * (4 if f32 else 8)
    vec = 16 if rb % 16 == 0 and ob % 16 == 0 else 8 if rb % 8 == 0 and ob % 8 == 0 else 4
    return sym_tiled(f32, vec)


def mixture_case(eng, n, d, f32, C, want, off=0, premap=None, zero_weights=(None, "one", "all"), seed=0):
    """One shape through asmc_mixture_logpdf (or _premap) with the edge rows of moments_ref.mixture_rows, for the plain mixture, one
    component of weight zero and every component of weight zero.  Returns the last device result."""
    assert mixture_path(d, f32, C, off, tiled=bool(os.environ.get("ASMC_MIXTURE_TILED"))) == want
    import torch

    got = None
    for zw in zero_weights:
        logw, mu, prec = M.mixture_params(d, C, seed=seed, zero_weight=zw)
        x, nan_rows = M.mixture_rows(n, d, mu, prec, seed=seed, f32=f32, premap=premap)
        ref, mag, sens = M.mixture_logpdf(x, logw, mu, prec, premap=premap)
        assert np.isnan(ref[nan_rows].astype(np.float64)).all() and np.isnan(ref.astype(np.float64)).sum() >= len(nan_rows)
        xd, mix = dev(eng, x, f32, off), eng.make_mixture(logw, mu, prec)
        if premap is None:
            got = ran(eng, lambda: eng.mixture_logpdf(xd, mix), {want: 1}).cpu().numpy()
        else:
            pm = torch.as_tensor(np.stack(premap)).to(eng.device).contiguous()
            got = ran(eng, lambda: eng.mixture_logpdf_premap(xd, pm, mix), {want: 1}).cpu().numpy()
        M.compare(got, ref, M.tol_mixture(d, mag, ref, sens),
                  f"mixture {n}x{d} {ids(f32)} C={C} off={off} weights-zero={zw} premap={premap is not None} {want}")
    return got


def shapes(*groups):
    return [(d, f32) for f32, ds in groups for d in ds]


FLAT = shapes((False, (2, 8, 32, 128)), (True, (4, 32, 256)))
TILED16 = shapes((False, (6, 48, 100, 256)), (True, (12, 96)))
TILED8 = shapes((False, (1, 3, 33)), (True, (2, 6)))
TILED4 = shapes((True, (1, 7, 33)))


def sid(sh):
    return [f"{ids(f32)}-d{d}" for d, f32 in sh]


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("d,f32", FLAT + TILED16 + TILED8 + TILED4, ids=sid(FLAT + TILED16 + TILED8 + TILED4))
def test_mixture_every_default_path(eng, d, f32, C):
    """fp64 d = 256 is the largest row: 132 KB of LDS, one wave per block."""
    mixture_case(eng, 5003, d, f32, C, mixture_path(d, f32, C))
    assert (mixture_path(d, f32, C).startswith("_Z14k_mixture_flat")) == ((d, f32) in FLAT)


# (d, fp32, C): k_mixture_flat<T, 4>, k_mixture_flat<T, 1>, k_mixture_logpdf<double, 16 | 8>, k_mixture_logpdf<float, 16 | 8 | 4>
ONE_PER_KERNEL = [(8, False, 2), (4, True, 2), (8, False, 1), (4, True, 1), (6, False, 2), (3, False, 2), (12, True, 2), (6, True, 2),
                  (7, True, 2)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("d,f32,C", ONE_PER_KERNEL, ids=[f"{ids(f32)}-d{d}-C{C}" for d, f32, C in ONE_PER_KERNEL])
def test_mixture_row_counts_around_one_tile(eng, d, f32, C, n):
    """(n = 1 is one clean row: the edge rows need a population of at least three.)"""
    mixture_case(eng, n, d, f32, C, mixture_path(d, f32, C))


@BOTH
def test_mixture_offset_views_take_the_narrower_copies(eng, f32):
    """d = 32 one element into an aligned buffer: the pointer, not the row length, rules out the flat kernel and the 16-byte copies."""
    mixture_case(eng, 5003, 32, f32, 2, sym_tiled(f32, 4 if f32 else 8), off=1)


@BOTH
@pytest.mark.parametrize("C", [5, 8])
def test_mixture_more_than_four_components_take_the_tiled_kernel(eng, C, f32):
    mixture_case(eng, 5003, 32, f32, C, sym_tiled(f32, 16))


@BOTH
@pytest.mark.parametrize("C", [1, 4])
def test_mixture_tiled_switch_agrees_with_the_flat_kernel(eng, monkeypatch, C, f32):
    flat = mixture_case(eng, 5003, 32, f32, C, sym_flat(f32, 1 if C == 1 else 4), zero_weights=(None,))
    monkeypatch.setenv("ASMC_MIXTURE_TILED", "1")
    tiled = mixture_case(eng, 5003, 32, f32, C, sym_tiled(f32, 16), zero_weights=(None,))
    logw, mu, prec = M.mixture_params(32, C)
    x, _ = M.mixture_rows(5003, 32, mu, prec, f32=f32)
    ref, mag, _ = M.mixture_logpdf(x, logw, mu, prec)
    assert M.same_nonfinite(flat, tiled)
    fin = np.isfinite(flat)
    assert np.all(np.abs(flat - tiled)[fin] <= 2 * M.tol_mixture(32, mag, ref)[fin])  # each within one tolerance of the restatement


@pytest.mark.parametrize("n,d,want", [(40001, 128, sym_flat(False, 4)), (140001, 100, sym_tiled(False, 16))], ids=["flat", "tiled"])
def test_mixture_second_grid_stride_pass(eng, n, d, want):
    """On 256 CUs the flat kernel's capped grid covers 32 768 rows of 64 pieces per pass, the tiled kernel's 131 072 rows of 800
    bytes (1024 blocks of two 64-row tiles)."""
    mixture_case(eng, n, d, False, 2, want, zero_weights=(None,))


@pytest.mark.parametrize("zero_h", [False, True], ids=["h", "h0"])
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("d,f32", FLAT, ids=sid(FLAT))
def test_mixture_premap_on_every_flat_shape(eng, d, f32, C, zero_h):
    """Bounded and unbounded coordinates side by side, rows exactly on and just beyond the clamp ends, a NaN in a bounded and in an
    unbounded coordinate: the clamp must let it through (numpy's clip)."""
    mixture_case(eng, 5003, d, f32, C, sym_flat(f32, 1 if C == 1 else 4), premap=M.premap_table(d, zero_h=zero_h))


def test_mixture_premap_refusals(eng, monkeypatch):
    import torch

    from aspire_amd._lib import ASMC_ERR_UNSUPPORTED, AsmcError

    def refused(d, C, off=0):
        logw, mu, prec = M.mixture_params(d, C)
        x, _ = M.mixture_rows(65, d, mu, prec)
        pm = torch.as_tensor(np.stack(M.premap_table(d))).to(eng.device)
        with pytest.raises(AsmcError, match=rf"rc={ASMC_ERR_UNSUPPORTED}\)"):
            eng.mixture_logpdf_premap(dev(eng, x, False, off), pm, eng.make_mixture(logw, mu, prec))

    refused(6, 2)  # not a power-of-two number of 16-byte pieces
    refused(32, 5)  # more than four components
    refused(32, 2, off=1)  # a misaligned view
    monkeypatch.setenv("ASMC_MIXTURE_TILED", "1")
    refused(32, 2)


# ---- (d) Gaussian draw ----------------------------------------------------------------------------------------------------------------
DRAW_N, DRAW_SEED, DRAW_GID0, DRAW_ID = 4099, 1234, 10, 3


@functools.lru_cache(maxsize=None)
def oracle_normals(d):
    import oracle as O

    O.build()
    return np.stack([O.pcn_noise(DRAW_SEED, DRAW_GID0 + i, DRAW_ID, d)[0] for i in range(DRAW_N)])


@BOTH
@pytest.mark.parametrize("d", [1, 5, 32, 256])
def test_gaussian_draw(eng, d, f32):
    import torch

    dt = torch.float32 if f32 else torch.float64
    mu, sigma = np.linspace(-1, 1, d), np.linspace(0.5, 2, d)
    mud, sigd = eng.asarray(mu), eng.asarray(sigma)
    draw = {f"_Z15k_gaussian_drawI{tname(f32)}Ev": 1, f"_Z15k_gaussian_logqI{tname(f32)}Ev": 1}
    x, lq = ran(eng, lambda: eng.gaussian_draw(DRAW_N, d, dt, mud, sigd, DRAW_SEED, DRAW_GID0, DRAW_ID), draw)
    xn, lqn = x.double().cpu().numpy(), lq.cpu().numpy()
    ref = mu + sigma * oracle_normals(d)
    tol = 1e-12 * np.abs(ref) + 1e-13 + (M.half_ulp32(ref) if f32 else 0.0)  # test_philox_normals_match_oracle_and_are_normal's
    M.compare(xn, ref, tol, f"gaussian draw x d={d} {ids(f32)}")
    rq, mag = M.gaussian_logq(xn, mu, sigma)
    M.compare(lqn, rq, M.tol_mixture(d, mag, rq), f"gaussian draw log q d={d} {ids(f32)}")
    # a shard: rows k .. of the whole draw, bit for bit
    k, m = 1027, 513
    xs, lqs = eng.gaussian_draw(m, d, dt, mud, sigd, DRAW_SEED, DRAW_GID0 + k, DRAW_ID)
    assert torch.equal(xs, x[k:k + m]) and torch.equal(lqs, lq[k:k + m])


# ---- (e) reference factor -------------------------------------------------------------------------------------------------------------
def fit(eng, d, sums, cov):
    """asmc_reference_factor on (sums, cov x (n_cov - 1)) - exact for n_cov - 1 = 4096 - as numpy arrays, with the status.
    (k_ref_factor is defined inside the library's extern "C" block: its symbol is not mangled.)"""
    import torch

    mu, L, Li = ran(eng, lambda: eng.reference_factor(d, M.N_MEAN, M.N_COV, moments=(sums, cov * (M.N_COV - 1))), {"k_ref_factor": 1})
    torch.cuda.synchronize()
    return mu.cpu().numpy(), L.cpu().numpy(), Li.cpu().numpy(), eng.reference_factor_status()


def check_factor(d, got, sums, cov, what, want_tries):
    mu, L, Li, status = got
    rmu, rL, rLi, tries, a = M.reference_fit(sums, cov * (M.N_COV - 1), M.N_MEAN, M.N_COV)
    assert tries == want_tries and status == tries, (what, status, tries)
    M.compare(mu, rmu, M.ulp64(rmu), f"{what} mu")
    assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(Li, 1) == 0)  # exactly zero above the diagonal
    EL, ELi = M.fit_gaps(a)
    low = np.tril(np.ones((d, d), dtype=bool))
    wL = M.compare(L[low], rL[low], (8 * EL + 4) * M.ulp64(rL[low]), f"{what} L (E = {EL:.3g})")
    wLi = M.compare(Li[low], rLi[low], (8 * ELi + 4) * M.ulp64(rLi[low]), f"{what} Linv (E = {ELi:.3g})")
    E = max(EL, ELi)
    resid = np.abs(Li.astype(LD) @ L.astype(LD) - np.eye(d)).astype(np.float64).max()
    bound = d * (8 * E + 4) * 2.0**-52 * np.linalg.norm(Li, 2) * np.linalg.norm(L, 2)
    print(f"TOL {what}: |Linv L - I| = {resid:.3g}, allowed {bound:.3g}")
    assert resid <= bound
    return wL, wLi


@pytest.mark.parametrize("d", M.FIT_DIMS)
def test_reference_factor_accuracy_at_condition_1e10(eng, d):
    cov, sums = M.spd_with_condition(d, 1e10), np.linspace(-3.0, 7.0, d) * M.N_MEAN / 3
    check_factor(d, fit(eng, d, sums, cov), sums, cov, f"fit d={d} cond=1e10", 0)


@pytest.mark.parametrize("lowest,tries", [(-3e-7, 4), (-3e-3, 6)])
@pytest.mark.parametrize("d", M.FIT_DIMS)
def test_reference_factor_jitter_ladder(eng, d, lowest, tries):
    """One eigenvalue at `lowest` x mean(diag): the try before the expected one is short of it by a factor of 30, the expected one
    clears it by 3.3 (test_moments_ref.py); the factor is that of cov + jitter mean(diag) I.  d = 1 has no such matrix - its one
    eigenvalue is mean(diag) - and takes the 1 x 1 matrix (`lowest`): the scale is 1 and the counts are the same."""
    cov, sums = M.with_lowest_eigenvalue(d, lowest, relative=d > 1), np.zeros(d)
    check_factor(d, fit(eng, d, sums, cov), sums, cov, f"fit d={d} lowest={lowest}", tries)


@pytest.mark.parametrize("d", M.FIT_DIMS)
def test_reference_factor_jitter_scale_is_one_for_a_non_positive_mean_diagonal(eng, d):
    cov, sums = M.all_negative(d), np.ones(d)
    check_factor(d, fit(eng, d, sums, cov), sums, cov, f"fit d={d} mean(diag) < 0", 4)


@pytest.mark.parametrize("what", ["eigenvalue -1e9", "+inf entry"])
@pytest.mark.parametrize("d", M.FIT_DIMS)
def test_reference_factor_failure_poisons_the_factors(eng, d, what):
    sums = np.linspace(1.0, 2.0, d)
    if what == "+inf entry":
        cov = M.spd_with_condition(d, 10.0)
        cov[(1, 0) if d > 1 else (0, 0)] = cov[(0, 1) if d > 1 else (0, 0)] = np.inf
    else:
        cov = M.with_lowest_eigenvalue(d, -1e9, relative=False)
    assert M.reference_fit(sums, cov * (M.N_COV - 1), M.N_MEAN, M.N_COV)[3] == -1
    fit(eng, d, sums, M.spd_with_condition(d, 10.0))  # a good factor in the buffers first: the failure must overwrite it
    fit(eng, d, sums, M.spd_with_condition(d, 10.0))  # (two buffers in turn)
    mu, L, Li, status = fit(eng, d, sums, cov)
    assert status == -1
    assert np.isnan(L).all() and np.isnan(Li).all()
    M.compare(mu, M.reference_fit(sums, cov * (M.N_COV - 1), M.N_MEAN, M.N_COV)[0], M.ulp64(sums / M.N_MEAN), f"failed fit d={d} mu")


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--lds32-child":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    lds32_child(sys.argv[2])
