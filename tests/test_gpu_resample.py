"""The resampling kernels of csrc/asmc_cdf.hip and csrc/asmc_resample.hip on every dispatch path and at the edges, against the plain restatement of
tests/resample_ref.py (tolerance of the fast cdf: its docstring and DESIGN.md section 3.17; it does not come from the device's output).
The exact cdf has its own bitwise tests (tests/test_gpu_parity.py); here it only serves as the cdf the searches run on.

Shape -> path (every case asserts, from profile_variants, the symbol that ran):

  k_tile_sum / k_scan_tiles<true> / k_tile_scan   the fast cdf; tiles of 2048, a second trip of k_scan_tiles above 1024 tiles
                                                  (n = 1024 2048 + 1, on an engine of its own); <false> is the exact mode's hint pass
  k_divide, k_divide_dev                          grid = min(ceil(n / 1024), 2048) blocks of 256: a further trip above 4 256 2048
  k_search                                        n < 2^17, or n_out < n / 8, or ASMC_SEARCH_PLAIN (child process)
  k_guide_build + k_search_guided                 n >= 2^17 and n_out >= n / 8; nb = n / 4 buckets
  k_search_pcg (asmc_importance_step)             guide of nb = n buckets, filled by k_exact_tile_write, under the same condition
  k_pcg64_uniforms                                65536 threads: a second draw per thread above that
  k_gather16_pow2<SH, CS>                         rows of 2^SH 16-byte pieces, SH = 3, 4, 5; CS: fp64 rows of 16, 32, 64 (column sums
                                                  ride along); four pieces per lane and trip: a second trip above 4 x 4096 x 256 pieces
  k_gather16                                      other rows of whole 16-byte pieces (and every such row under ASMC_GATHER_PLAIN)
  k_gather_elem<double | float>                   rows or pointers that are not 16-byte multiples
  k_pack_records                                  n_in >= 2^16 and n_out >= n_in / 4: the gather reads (ll, lp, lq) as one record
  k_valid_count / k_scan_tiles_ll / k_compact_scatter<double | float>   tiles of 2048; k_scan_tiles_ll carries between chunks of 64 tiles
  k_range_count / k_range_scatter<false> / k_range_info, k_range_count_shard / k_range_scatter<true>   the range selection

Everything but the fast cdf and the column sums is compared bit for bit.  Every case prints the fast cdf's worst error in units of
its tolerance (pytest -s).

Measured on an MI355X (DESIGN.md section 3.17 has the full list): fast cdf, worst error in units of the tolerance 0.152 (`equal`, n =
300 001; per law 0.02 - 0.15), 0.104 on the second trip of the tile scan (A = 59); column sums behind a gather 0.0054 of the moments
tolerance; everything else equal.  Against the parent's kernels 15 of the 81 cases fail, with the scan's symbol taken as the parent
names it: the fast-cdf contract for smooth, tiny_first, equal (last element is not the total: 25 of 132 populations counted), heavy,
ties, zeros70, dominant, zeros_tail and the second trip (decreases: 1.0 - 1.7 % of zeros70's elements; the prefix in front of a dominant
weight lost), the three smooth seeds, a search that answered n for a draw below 1 on the fast cdf, the search's clamp, and the closing
test.  Total time of the module: 17 s for 81 tests (the three child processes 2 s each).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import moments_ref as M
import resample_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_tile_", "k_scan_tiles", "k_divide", "k_search", "k_guide_build", "k_pcg64_uniforms", "k_systematic", "k_pack_records",
            "k_gather", "k_valid_count", "k_compact_scatter", "k_range_")
RAN = set()  # (kernel name, template arguments) an asserted launch has covered (test_every_kernel_symbol_ran closes the module)
SEARCH_LAWS = ("smooth", "zeros70", "heavy", "zeros_tail", "first_only", "last_only")
FAST = {("k_tile_sum",): 1, ("k_scan_tiles", "Lb1"): 1, ("k_tile_scan",): 1}
EXACT = {("k_tile_sum",): 1, ("k_scan_tiles", "Lb0"): 1}


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(scope="module")
def big():
    """An engine above the suite's 2^21: the second trip of k_scan_tiles (more than 1024 tiles) and of k_divide."""
    from aspire_amd.engine import HipEngine

    e = HipEngine(0, n_max=(1 << 21) + 4096, d_max=1)
    yield e
    e.close()


def sym(name, targs=None):
    return f"_Z{len(name)}{name}" + ("" if targs is None else f"I{targs}E")


def ran(eng, fn, expect):
    """fn() with the assertion that, of this module's kernel families, exactly the symbols `expect` ran ({(name, template
    arguments or None): launches, None = any positive number})."""
    eng.profile(True)
    try:
        out = fn()
        var = {s: c for s, c in eng.profile_variants().items() if any(f in s for f in FAMILIES)}
    finally:
        eng.profile(False)
    want = {sym(*k): c for k, c in expect.items()}
    bare = {k[0]: sym(*k) for k in expect if len(k) == 1}  # (k_range_info sits inside the file's extern "C" block: its symbol is its name)
    var = {bare.get(s, s): c for s, c in var.items()}
    for s in var:  # (the length in front of a mangled name keeps k_search and k_search_guided apart)
        assert any(s.startswith(p) for p in want), (s, want)
    for p, cnt in want.items():
        got = sum(c for s, c in var.items() if s.startswith(p))
        assert cnt is None and got > 0 or got == cnt, (p, cnt, var)
    RAN.update((k[0], k[1] if len(k) > 1 else None) for k in expect)
    return out


def dev(eng, *arrs):
    return tuple(eng.asarray(np.ascontiguousarray(a, dtype=np.float64)) for a in arrs)


def same_nan(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(np.asarray(ref, dtype=np.float64)))


# ---- the fast cdf ------------------------------------------------------------------------------------------------------------------------
def _check_fast(eng, w, carry, label):
    """The fast cdf of w behind `carry`, plain and normalised, against the contract; returns the worst error in units of the
    tolerance."""
    wd = eng.asarray(w)
    cdf, total = ran(eng, lambda: eng.cdf(wd, "fast", carry), FAST)
    got = cdf.cpu().numpy()
    ref, tol = R.fast_tol(w, carry)
    assert same_nan(got, ref), label
    worst = R.units(got, ref, tol)
    assert np.all(np.diff(got) >= 0), (label, "decreases at", np.flatnonzero(np.diff(got) < 0)[:5])
    assert total == got[-1], (label, total, got[-1])
    fused, total2 = ran(eng, lambda: eng.cdf(wd, "fast", carry, normalize=True), FAST)
    fn = fused.cpu().numpy()
    assert total2 == total, label
    with np.errstate(all="ignore"):
        assert np.array_equal(fn, got / total, equal_nan=True), (label, "fused normalisation is not the division by the total")
    refn, toln = R.fast_tol(w, carry, normalize=True)
    if total > 0 and np.isfinite(total):
        assert fn[-1] == 1.0 and np.all(np.diff(fn) >= 0), (label, fn[-1])
        worst = max(worst, R.units(fn, refn, toln))
    else:  # nothing to normalise by: NaN everywhere, in both modes
        exact, _ = ran(eng, lambda: eng.cdf(wd, "exact", carry, normalize=True), EXACT)
        assert np.all(np.isnan(fn)) and np.all(np.isnan(exact.cpu().numpy())), label
    return worst


@pytest.mark.parametrize("law", R.LAWS)
def test_fast_cdf_contract_every_law_and_size(eng, law):
    worst = {}
    for n in (1, 7, 2047, 2048, 2049, 100003, 300001):
        for carry in (0.0, 0.37):
            w = R.weights(law, n, 11)
            worst[n, carry] = _check_fast(eng, w, carry, f"{law} n={n} carry={carry}")
    if law == "dominant":  # the prefix in front of the dominant weight is there, to its own relative accuracy
        n = 2049
        w = R.weights(law, n, 11)
        got = eng.cdf(eng.asarray(w), "fast", 0.0)[0].cpu().numpy()
        k = R.dominant_index(n)
        assert np.all(got[:k] > 0) and np.all(np.abs(got[:k] / (np.arange(1, k + 1) * 1e-30) - 1) < 1e-13)
    top = max(worst, key=worst.get)
    print(f"fast cdf {law}: worst error {worst[top]:.3g} of the tolerance (A = {R.fast_additions(300001)}) at n, carry = {top}")
    assert worst[top] < 1, worst


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fast_cdf_last_element_is_the_total_on_smooth_weights(eng, seed):
    """The populations on which the order of additions the kernels had before gave cdf[-1] != total (a search could then
    return n for a draw below 1)."""
    for n in (100003, 300001, 1 << 20):
        w = R.weights("smooth", n, seed)
        assert _check_fast(eng, w, 0.0, f"smooth n={n} seed={seed}") < 1


def test_fast_cdf_second_chunk_of_the_tile_scan(big):
    n = 1024 * 2048 + 1
    assert R.fast_additions(n) == 59
    for law in ("smooth", "zeros70", "heavy", "dominant", "last_only"):
        w = R.weights(law, n, 13)
        worst = _check_fast(big, w, 0.37 if law == "smooth" else 0.0, f"{law} n={n}")
        print(f"fast cdf {law} n={n}: worst error {worst:.3g} of the tolerance (A = 59)")
        assert worst < 1


def test_divide_is_numpys_division(eng, big):
    import torch

    for e, n in ((eng, 7), (big, 4 * 256 * 2048 + 3)):
        w = R.weights("smooth", n, 5) * 0.37
        cdf, total = ran(e, lambda: e.cdf(e.asarray(w), "exact", 0.0), EXACT)
        c = cdf.cpu().numpy()
        assert total == c[-1]
        out = torch.zeros(3, dtype=torch.float64, device=e.device)
        e.cdf_total_dev(out[1:])
        assert out.cpu().numpy().tolist() == [0.0, total, 0.0]
        got = ran(e, lambda: e.cdf_normalize_last(cdf.clone()), {("k_divide_dev",): 1}).cpu().numpy()
        assert R.bits_equal(got, c / total) and got[-1] == 1.0
        for last in (total, 3.0, 1e-300):
            got = ran(e, lambda: e.cdf_normalize(cdf.clone(), last), {("k_divide",): 1}).cpu().numpy()
            assert R.bits_equal(got, c / last), (n, last)


# ---- search --------------------------------------------------------------------------------------------------------------------------------
def _device_cdf(eng, law, n, mode="exact", seed=2):
    """(device tensor, host copy) of the normalised cdf of the law."""
    w = R.staircase_cdf(n, max(n // 4, 1)) if law == "staircase" else None
    if w is not None:
        return eng.asarray(w), w
    cdf = eng.cdf(eng.asarray(R.weights(law, n, seed)), mode, 0.0, normalize=True)[0]
    return cdf, cdf.cpu().numpy()


def _keys(cdf, n_out, seed=1):
    """Exactly n_out keys: the named ones, then keys on and around the bucket edges of nb = n / 4 and n, then draws."""
    n = cdf.size
    named = R.all_keys(cdf, tuple({max(n // 4, 1), n}))
    edges = np.concatenate([R.edge_keys(max(n // 4, 1), every=max(1, (n // 4) // 3000)), R.edge_keys(n, every=max(1, n // 3000))])
    pool = np.concatenate([named, edges])
    if pool.size >= n_out:
        return pool[:n_out] if n_out >= named.size else named[np.linspace(0, named.size - 1, n_out).astype(np.int64)]
    return np.concatenate([pool, np.random.default_rng(seed).random(n_out - pool.size)])


def _check_search(eng, cdf_d, cdf, u, guided):
    expect = {("k_guide_build",): 1, ("k_search_guided",): 1} if guided else {("k_search",): 1}
    idx = ran(eng, lambda: eng.search(cdf_d, eng.asarray(u)), expect).cpu().numpy()
    ref = R.search_device(cdf, u)
    assert np.array_equal(idx, ref), (np.flatnonzero(idx != ref)[:5], u[idx != ref][:5], idx[idx != ref][:5], ref[idx != ref][:5])
    assert np.all(idx[np.isnan(u)] == 0)  # the pinned deviation from numpy (which answers n)
    if cdf[-1] == 1.0:  # then nothing was clamped: numpy's answer wherever the key is a number
        ok = ~np.isnan(u)
        assert np.array_equal(idx[ok], R.search(cdf, u)[ok]) and np.all(idx[u < 1.0] < cdf.size)


@pytest.mark.parametrize("law", SEARCH_LAWS + ("staircase",))
def test_plain_search_is_searchsorted_right(eng, law):
    for n, n_out in ((1, None), (5, None), (100000, None), (131072, 16383), (131071, 131071)):
        cdf_d, cdf = _device_cdf(eng, law, n)
        u = _keys(cdf, n_out if n_out else R.all_keys(cdf, tuple({max(n // 4, 1), n})).size + 2000)
        assert n < R.SEARCH_GUIDE_MIN_N or u.size < n // 8
        _check_search(eng, cdf_d, cdf, u, guided=False)


@pytest.mark.parametrize("law", SEARCH_LAWS + ("staircase",))
def test_guided_search_is_searchsorted_right(eng, law):
    for n, n_out in ((131072, 16384), (131074, 16384 + 7000), (300001, 300001 // 8), (300001, 120000)):
        cdf_d, cdf = _device_cdf(eng, law, n)
        u = _keys(cdf, n_out)
        assert u.size == n_out >= n // 8 and np.isnan(u).any() and (u >= 1).any() and (u < 0).any()
        _check_search(eng, cdf_d, cdf, u, guided=True)


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_no_draw_below_one_leaves_the_rows(eng, mode):
    """For every law and both cdf modes: idx < n for every key in [0, 1), checked on the host before any gather."""
    for law in R.LAWS:
        for n, guided in ((100003, False), (131072, True)):
            cdf_d, cdf = _device_cdf(eng, law, n, mode, seed=0)
            g = np.random.default_rng(n)
            u = np.concatenate([g.random(n // 8 + 5), [0.0, np.nextafter(1.0, 0.0)], 1.0 - g.random(4000) * 2.0 ** -40])
            u = u[(u >= 0.0) & (u < 1.0)]
            expect = {("k_guide_build",): 1, ("k_search_guided",): 1} if guided else {("k_search",): 1}
            idx = ran(eng, lambda: eng.search(cdf_d, eng.asarray(u)), expect).cpu().numpy()
            assert idx.min() >= 0 and idx.max() < n, (law, n, mode, idx.max())
            if not np.isnan(cdf).any():
                assert np.array_equal(idx, R.search_device(cdf, u)), (law, n, mode)


def test_search_clamps_a_key_below_one_on_a_cdf_that_ends_below_it(eng):
    for n, guided in ((1000, False), (131072, True)):
        cdf = R.exact_cdf(R.weights("smooth", n, 1), normalize=True) * (1.0 - 2.0 ** -30)
        u = _keys(cdf, max(n // 8, 3000))
        assert (u > cdf[-1]).any() and R.search(cdf, u[u < 1.0]).max() == n
        _check_search(eng, eng.asarray(cdf), cdf, u, guided)


# ---- the importance step's fused draw + search -----------------------------------------------------------------------------------------
def _log_weight_law(law, n, seed):
    g = np.random.default_rng([seed, n])
    ll = g.normal(size=n)
    lp, lq = 0.01 * g.normal(size=n), 0.01 * g.normal(size=n)
    if law == "zeros_tail":
        ll[n - 3000:] = -np.inf
        return ll, lp, lq, 0.5
    ll = 0.01 * ll
    ll[R.dominant_index(n)] += 150.0  # at beta = 1 every other weight is e^-150 of it, and nonzero
    return ll, lp, lq, 1e-6  # (ESS / N = 1 / N at beta = 1 is above this target: beta* = 1)


@pytest.mark.parametrize("law", ["zeros_tail", "dominant"])
@pytest.mark.parametrize("n", [131071, 131072, 131073])
def test_importance_step_indices_are_searchsorted_of_the_restated_cdf(eng, n, law):
    from aspire_amd import smc_math

    ll, lp, lq, target = _log_weight_law(law, n, 3)
    d = dev(eng, ll, lp, lq)
    for n_out in (n // 8, n // 8 - 1):
        rng = np.random.default_rng(n_out)
        idx = ran(eng, lambda: eng.importance_step(*d, 0.0, target, 1e-6, smc_math.pcg64_state(rng), n_out), {("k_search_pcg",): 1})
        res = eng.importance_result()
        assert res[9] and (law != "dominant" or res[0] == 1.0), res
        w = eng._is_bufs["w"].cpu().numpy()
        cdf = R.exact_cdf(w, normalize=True)
        assert R.bits_equal(eng._is_bufs["cdf"].cpu().numpy(), cdf)
        if law == "zeros_tail":
            assert np.all(w[n - 3000:] == 0.0) and np.all(cdf[n - 3001:] == 1.0)
        else:
            assert np.count_nonzero(w) == n and w[R.dominant_index(n)] > 0.99
        got = idx.cpu().numpy()
        assert got.max() < n and np.array_equal(got, R.search(cdf, R.pcg64_uniforms(rng, 0, n_out))), (n, n_out, law)


# ---- uniforms ------------------------------------------------------------------------------------------------------------------------------
def test_pcg64_uniforms_large_offsets_and_a_second_increment(eng):
    a, b = np.random.default_rng(5), np.random.default_rng(6)
    sa, sb = R.pcg64_state(a), R.pcg64_state(b)
    assert (sa[2], sa[3]) != (sb[2], sb[3])  # another increment: the jump table is rebuilt, and rebuilt again
    for rng, st in ((a, sa), (b, sb), (a, sa)):
        for offset in (0, 2 ** 32 - 3, 2 ** 40 + 1):
            for n in (1, 65535, 65536, 65537):
                got = ran(eng, lambda: eng.uniforms_pcg64(st, offset, n), {("k_pcg64_uniforms",): 1}).cpu().numpy()
                assert R.bits_equal(got, R.pcg64_uniforms(rng, offset, n)), (offset, n)


def test_systematic_uniforms_bit_for_bit(eng):
    g = np.random.default_rng(3)
    for n_out, j0, n_total in ((1, 0, 1), (1, 5, 9), (1025, 0, 1025), (1025, 4099, 10007), (300001, 7, 1 << 21)):
        for u0 in (0.0, 0.25, float(np.nextafter(1.0, 0.0))):
            got = ran(eng, lambda: eng.systematic_uniforms(n_out, j0, n_total, u0), {("k_systematic",): 1}).cpu().numpy()
            assert R.bits_equal(got, R.systematic(n_out, j0, n_total, u0)), (n_out, j0, n_total, u0)
        v = g.random(n_out)
        got = ran(eng, lambda: eng.systematic_uniforms(n_out, j0, n_total, 0.5, eng.asarray(v)), {("k_systematic",): 1}).cpu().numpy()
        assert R.bits_equal(got, R.systematic(n_out, j0, n_total, v=v)), (n_out, j0, n_total)


# ---- gather --------------------------------------------------------------------------------------------------------------------------------
PAYLOAD_ROWS = (3, 5, 7, 9)


def _rows(n, d, f32, seed=7):
    """(x, ll, lp, lq) with NaN (one with a payload), +inf and -inf in rows 3, 5, 7, 9 where they exist."""
    g = np.random.default_rng([seed, n, d])
    x = g.normal(size=(n, d)).astype(np.float32 if f32 else np.float64)
    ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
    if n > 9:
        x[3, d // 2], x[5, 0], x[7, d - 1] = np.nan, np.inf, -np.inf
        x[9] = np.frombuffer(np.array([0x7FC00123] * d, dtype=np.uint32).tobytes(), dtype=np.float32) if f32 else \
            np.frombuffer(np.array([0x7FF8000000000123] * d, dtype=np.uint64).tobytes(), dtype=np.float64)
        ll[3], lp[5], lq[7], ll[9] = np.nan, np.inf, -np.inf, -np.inf
    return x, ll, lp, lq


def _indices(n_in, n_out, seed=1, payload=True):
    """n_out indices in [0, n_in): row 0, row n_in - 1, duplicates, the payload rows (or none of them), the rest drawn."""
    g = np.random.default_rng([seed, n_in, n_out])
    idx = g.integers(0, n_in, n_out)
    if not payload and n_in > 10:
        idx = 10 + idx % (n_in - 10)
    head = [0, n_in - 1, n_in - 1, 0] + ([r for r in PAYLOAD_ROWS if r < n_in and payload and n_in > 9] * 2)
    k = min(len(head), n_out)
    idx[:k] = head[:k]
    assert idx.min() >= 0 and idx.max() < n_in
    return idx.astype(np.int64)


def _check_gather(eng, n_in, n_out, d, f32, kernel, packs, misalign=False, colsum=False):
    import torch

    x, ll, lp, lq = _rows(n_in, d, f32)
    if misalign:  # a row of whole 16-byte pieces behind a pointer that is 8 mod 16
        store = torch.empty(n_in * d + 1, dtype=torch.float64, device=eng.device)
        xd = store[1:].view(n_in, d)
        xd.copy_(torch.as_tensor(x))
        assert xd.data_ptr() % 16 == 8 and xd.is_contiguous()
    else:
        xd = torch.as_tensor(x).to(eng.device)
    d3 = dev(eng, ll, lp, lq)
    expect = {kernel: 1, **({("k_pack_records",): 1} if packs else {})}
    assert packs == (n_in >= R.GATHER_PACK_MIN_N and n_out >= n_in // 4)
    idx = _indices(n_in, n_out)
    xo, a, b, c = ran(eng, lambda: eng.gather(eng.asarray(idx, dtype=torch.int64), xd, *d3), expect)
    rx, ra, rb, rc = R.gather(idx, x, ll, lp, lq)
    for got, ref in ((xo, rx), (a, ra), (b, rb), (c, rc)):
        assert R.bits_equal(got.cpu().numpy(), ref), (n_in, n_out, d, f32, kernel)
    iv = torch.int32 if f32 else torch.int64
    assert torch.equal(xo.cpu().view(iv), torch.as_tensor(rx).view(iv))
    if not colsum:
        return None
    # the column sums that rode along (finite rows only), through the reduction the reference fit uses behind a gather
    idx = _indices(n_in, n_out, seed=2, payload=False)
    eng.profile(True)
    try:
        xo = eng.gather(eng.asarray(idx, dtype=torch.int64), xd, *d3)[0]
        s = eng.colsum_dev(xo, gathered=True).cpu().numpy()
        var = eng.profile_variants()
    finally:
        eng.profile(False)
    assert not any("k_colsum" in k for k in var), var  # (no pass over the rows: the gather's partials were used)
    ref, sabs = R.colsum(R.gather(idx, x, ll, lp, lq)[0])
    wv = M.compare(s, ref, M.tol_colsum(n_out, sabs.astype(np.float64)), f"gathered column sums {n_out}x{d}", quiet=True)
    assert R.bits_equal(xo.cpu().numpy(), x[idx])
    s2 = eng.colsum(xo)  # and the ordinary pass over the same rows agrees under the same tolerance
    M.compare(s2, ref, M.tol_colsum(n_out, sabs.astype(np.float64)), f"column sums {n_out}x{d}", quiet=True)
    return wv


POW2 = "k_gather16_pow2"


@pytest.mark.parametrize("d,sh", [(16, 3), (32, 4), (64, 5)])
def test_gather_pow2_rows_with_column_sums(eng, d, sh):
    worst = 0.0
    for n_in, n_out in ((20011, 30007), (20011, 1), (11, 300), (2049, 2048)) + (((3001, 262145),) if d == 32 else ()):
        worst = max(worst, _check_gather(eng, n_in, n_out, d, False, (POW2, f"Li{sh}ELb1E"), False, colsum=True))
    if d == 32:  # four pieces per lane and trip over 4096 blocks of 256: 262 145 rows of 16 pieces take a second trip
        assert 262145 * 16 > 4 * 4096 * 256
    print(f"k_gather16_pow2<{sh}, true>: column sums, worst error {worst:.3g} of the moments tolerance")


@pytest.mark.parametrize("d,sh", [(32, 3), (64, 4), (128, 5)])
def test_gather_pow2_rows_fp32(eng, d, sh):
    for n_in, n_out in ((20011, 30007), (20011, 1), (11, 300)):
        _check_gather(eng, n_in, n_out, d, True, (POW2, f"Li{sh}ELb0E"), False)


@pytest.mark.parametrize("d,f32", [(2, False), (4, False), (6, False), (12, False), (128, False), (4, True), (12, True)])
def test_gather_sixteen_byte_pieces(eng, d, f32):
    for n_in, n_out in ((20011, 30007), (20011, 1), (11, 300)) + (((4097, 1 << 19),) if d <= 12 else ()):  # (the last: both of k_gather16's loops)
        _check_gather(eng, n_in, n_out, d, f32, ("k_gather16",), False)


@pytest.mark.parametrize("d,f32,misalign", [(3, False, False), (5, False, False), (3, True, False), (5, True, False), (4, False, True)])
def test_gather_elementwise(eng, d, f32, misalign):
    for n_in, n_out in ((20011, 30007), (20011, 1), (11, 300)):
        _check_gather(eng, n_in, n_out, d, f32, ("k_gather_elem", "f" if f32 else "d"), False, misalign=misalign)


def test_gather_packs_records_from_the_thresholds_on(eng):
    for n_in, n_out, packs in ((65536, 16384, True), (65535, 16384, False), (65536, 16383, False), (65537, 70001, True)):
        _check_gather(eng, n_in, n_out, 4, False, ("k_gather16",), packs)
        _check_gather(eng, n_in, n_out, 3, False, ("k_gather_elem", "d"), packs)
        _check_gather(eng, n_in, n_out, 32, False, (POW2, "Li4ELb1E"), packs, colsum=packs)


# ---- the forms an environment variable selects once per process --------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_resample as T, resample_ref as R
from aspire_amd.engine import HipEngine
eng = HipEngine(0, n_max=1 << 19, d_max=64)
mode = {mode!r}
if mode == "search":
    for law in ("smooth", "zeros70", "staircase"):
        for n, n_out in ((131072, 16384), (300001, 40000)):
            cdf_d, cdf = T._device_cdf(eng, law, n)
            T._check_search(eng, cdf_d, cdf, T._keys(cdf, n_out), guided=False)
elif mode == "gather":
    for d, f32 in ((16, False), (32, False), (64, False), (32, True), (6, False)):
        T._check_gather(eng, 20011, 30007, d, f32, ("k_gather16",), False)
    T._check_gather(eng, 65536, 16384, 32, False, ("k_gather16",), True)
else:
    T._check_gather(eng, 20011, 30007, 32, False, (T.POW2, "Li4ELb0E"), False)
    T._check_gather(eng, 65536, 16384, 64, False, (T.POW2, "Li5ELb0E"), True)
print("CHILD_OK", sorted(T.RAN, key=str))
eng.close()
"""


@pytest.mark.parametrize("mode,var,covers", [("search", "ASMC_SEARCH_PLAIN", None), ("gather", "ASMC_GATHER_PLAIN", None),
                                             ("nocolsum", "ASMC_GATHER_NO_COLSUM", [(POW2, "Li4ELb0E"), (POW2, "Li5ELb0E")])])
def test_plain_forms_in_a_child_process(mode, var, covers):
    """ASMC_SEARCH_PLAIN and ASMC_GATHER_PLAIN are read once per process: above both thresholds the search stays k_search, and
    rows of 2^SH pieces go through k_gather16; ASMC_GATHER_NO_COLSUM gives the fp64 rows k_gather16_pow2<SH, false>."""
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mode=mode)
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, var: "1"}, capture_output=True, text=True, timeout=240)
    print(out.stdout[-400:])
    assert out.returncode == 0 and "CHILD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    RAN.update(covers or [])


# ---- validity compaction -------------------------------------------------------------------------------------------------------------------
def _mask_case(n, mask, seed):
    g = np.random.default_rng([seed, n])
    ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
    lq[g.integers(0, n, max(1, n // 10))] = np.nan  # (log q plays no part in validity, and is copied as it is)
    bad = {"none_valid": np.ones(n, bool), "first_invalid": np.arange(n) == 0, "last_invalid": np.arange(n) == n - 1,
           "half": g.random(n) < 0.5}[mask]
    kinds = g.integers(0, 4, n)
    ll[bad & (kinds == 0)] = np.nan
    ll[bad & (kinds == 1)] = np.inf
    ll[bad & (kinds == 2)] = -np.inf
    lp[bad & (kinds == 3)] = np.nan
    return ll, lp, lq, bad


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("mask", ["none_valid", "first_invalid", "last_invalid", "half"])
def test_compact_valid_every_mask_and_size(eng, mask, f32):
    import torch

    for n in (1, 2048, 2049, 10007, 64 * 2048 + 1):
        for d in (1, 5, 32):
            if n > 20000 and d == 32:
                continue
            ll, lp, lq, bad = _mask_case(n, mask, d)
            x = np.random.default_rng(n + d).normal(size=(n, d)).astype(np.float32 if f32 else np.float64)
            xd = torch.as_tensor(x).to(eng.device)
            d3 = dev(eng, ll, lp, lq)
            expect = {("k_valid_count",): 1, ("k_scan_tiles_ll",): 1, ("k_compact_scatter", "f" if f32 else "d"): int(bad.any())}
            got = ran(eng, lambda: eng.compact_valid(xd, *d3), expect)
            ref = R.compact(x, ll, lp, lq)
            assert ref[0].shape[0] == n - int(bad.sum())
            for a, b in zip(got, ref):
                assert R.bits_equal(a.cpu().numpy(), b), (n, d, mask, f32)


def test_compact_valid_leaves_a_valid_population_alone(eng):
    for n in (1, 2049, 64 * 2048 + 1):
        x, ll, lp, lq = _rows(n, 5, False)
        ll, lp = np.where(np.isfinite(ll), ll, 0.0), np.where(np.isfinite(lp), lp, 0.0)
        import torch

        args = (torch.as_tensor(x).to(eng.device),) + dev(eng, ll, lp, lq)
        got = ran(eng, lambda: eng.compact_valid(*args), {("k_valid_count",): 1, ("k_scan_tiles_ll",): 1})
        assert all(a is b for a, b in zip(got, args))


# ---- range selection ---------------------------------------------------------------------------------------------------------------------
RANGE = {("k_range_count",): 1, ("k_scan_tiles_ll",): 1, ("k_range_scatter", "Lb0"): 1}


@pytest.mark.parametrize("n", [1, 2048, 2049, 64 * 2048 + 1])
def test_select_range_edges_and_empty_results(eng, n):
    import torch

    u = np.random.default_rng(n).random(n)
    u[:: 7] = 0.25  # keys equal to lo
    u[3:: 7] = 0.5  # ... and to hi
    ud = eng.asarray(u)
    for lo, hi in ((0.0, 1.0), (0.25, 0.5), (0.5, 0.5), (0.5, 0.25), (2.0, 3.0), (0.25, float(np.nextafter(0.25, 1.0)))):
        got = ran(eng, lambda: eng.select_range(ud, eng.asarray(np.array([lo, hi]))), RANGE).cpu().numpy()
        assert R.bits_equal(got, R.select_range(u, lo, hi)), (n, lo, hi)
        edges = eng.asarray(np.array([1.0, 0.125, lo, hi]))  # {failure flag, total, lo, hi}
        out, info = ran(eng, lambda: eng.select_range_dev(ud, edges), {**RANGE, ("k_range_info",): 1})
        kept, flag = info.cpu().numpy().tolist()
        assert flag == 1 and kept == got.size and R.bits_equal(out[:kept].cpu().numpy(), got)


def _shard_chain(eng, w, cuts):
    """The sharded exact cdf for emulated ranks up to the final chain state: per rank (weights, cdf buffer, all records, first
    tile, work buffer, state)."""
    import torch

    shards = [eng.asarray(w[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    recs, cdfs = [], []
    for r, ws in enumerate(shards):
        cdf, rec = eng.cdf_shard_records(ws, float(np.sum(w[:cuts[r]])), r == 0)
        recs.append(rec), cdfs.append(cdf)
    recs_all = torch.cat(recs, dim=0).contiguous()
    t0 = np.cumsum([0] + [rc.shape[0] for rc in recs])
    world = len(shards)
    r1 = [eng.cdf_shard_chain(shards[r], cdfs[r], recs_all, int(t0[r]), None, None, world, r) for r in range(world)]
    states = torch.cat([st for _, st in r1]).contiguous()
    out = []
    for r in range(world):
        work, st = eng.cdf_shard_chain(shards[r], cdfs[r], recs_all, int(t0[r]), r1[r][0], states, world, r)
        out.append((shards[r], cdfs[r], recs_all, int(t0[r]), work, st))
    return out


@pytest.mark.parametrize("n,cuts,n_u", [(10000, [0, 4097, 10000], 10000), (10000, [0, 4097, 10000], 256 * 2048 + 4099), (6000, [0, 1, 2049, 6000], 2049),
                                        (300001, [0, 100000, 200001, 300001], 10007)])
def test_shard_finish_select_equals_finish_then_select(eng, n, cuts, n_u):
    """k_range_count_shard + k_range_scatter<true> against the step-by-step form, bit for bit; more than 256 tiles of draws make
    the scatter's own scan over the counts stride."""
    w = R.weights("smooth", n, 9)
    u = eng.asarray(np.random.default_rng(n_u).random(n_u))
    steps = _shard_chain(eng, w, cuts)
    fused = _shard_chain(eng, w, cuts)
    ref = np.cumsum(w)
    ref = ref / ref[-1]
    for r, (a, b) in enumerate(zip(steps, fused)):
        edges = eng.cdf_shard_finish(*a)
        out, info = ran(eng, lambda: eng.select_range_dev(u, edges), {**RANGE, ("k_range_info",): 1})
        e2, out2, info2 = ran(eng, lambda: eng.cdf_shard_finish_select(*b, u), {("k_range_count_shard",): 1, ("k_range_scatter", "Lb1"): 1})
        assert R.bits_equal(edges.cpu().numpy(), e2.cpu().numpy()) and R.bits_equal(a[1].cpu().numpy(), b[1].cpu().numpy())
        kept, flag = info.cpu().numpy().tolist()
        assert info2.cpu().numpy().tolist() == [kept, flag] and flag in (0, 1)
        print(f"sharded finish n={n} cuts={cuts} rank {r}: flag {flag}, kept {kept}")
        assert flag == 0 or cuts[1] < 8192  # (smooth weights, boundaries past the first tiles: the chain closes, numpy judges below)
        assert R.bits_equal(out[:kept].cpu().numpy(), out2[:kept].cpu().numpy())
        if flag == 0:  # (a rank boundary this early may leave the chain open: the flag then says so, and both forms agree on it)
            lo, hi = (ref[cuts[r] - 1] if cuts[r] else 0.0), ref[cuts[r + 1] - 1]
            assert R.bits_equal(out2[:kept].cpu().numpy(), R.select_range(u.cpu().numpy(), lo, hi)), r
            assert R.bits_equal(b[1].cpu().numpy(), ref[cuts[r]:cuts[r + 1]])


# ---- every kernel of the families ran ---------------------------------------------------------------------------------------------------
def test_every_kernel_symbol_ran():
    """Closes the module: every __global__ kernel of csrc/asmc_cdf.hip and csrc/asmc_resample.hip in the families above, in every instantiation the
    library launches, appears in an asserted launch.  It needs the whole module to have run: under a -k selection it fails."""
    src = "".join(open(os.path.join(ROOT, "aspire_amd", "csrc", f)).read() for f in ("asmc_cdf.hip", "asmc_resample.hip"))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\([A-Z_0-9a-z]+\)\s+)?void\s+(k_[a-z0-9_]+)\s*\(", src))
    kernels = {k for k in kernels if any(f in k for f in FAMILIES)}
    assert len(kernels) == 22, sorted(kernels)
    templated = {"k_scan_tiles": ["Lb0", "Lb1"], "k_gather16_pow2": [f"Li{sh}ELb{cs}E" for sh in (3, 4, 5) for cs in (0, 1)],
                 "k_gather_elem": ["d", "f"], "k_compact_scatter": ["d", "f"], "k_range_scatter": ["Lb0", "Lb1"]}
    assert set(templated) <= kernels
    required = {(k, t) for k in kernels for t in templated.get(k, [None])}
    assert not required - RAN, sorted(required - RAN, key=str)
