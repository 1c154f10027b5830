"""Pins tests/resample_ref.py, the restatement tests/test_gpu_resample.py judges the resampling kernels by (no GPU):

  - it reproduces tests/golden/ref_resample.npz (the reference's own indices) and the C oracle's resample_indices, compact_valid and
    systematic_uniforms;
  - numpy's fp64 cumsum lies inside the fast-cdf tolerance for every law up to n = 44, where its own chain of k - 1 sequential
    additions is no longer than the A = 43 of the kernels' tree (beyond that it may drift out: `equal` at n = 2047 rounds the
    same way at every step and ends 8.7 tolerances away - the fast cdf is the more accurate of the two);
  - an fp64 model of the fast kernels' order of additions (`model_fast_cdf`: serial sums of 8, xor butterfly, Hillis-Steele scans,
    shifted exclusive prefixes, running maxima, clamps) meets the tolerance and the contract (non-decreasing, last == total) on
    every law, and the same model with the scan the kernels had before (exclusive prefix by subtraction, no maxima, last element
    from its own tree) breaks each of the three on some law: what the GPU module is expected to show on the parent's kernels;
  - plausible mistakes land outside: side="left", a guide built with `<`, a bucket without the settling loops, the subtracting
    scan on `dominant`, a tile prefix without its carry, a gather with row stride d - 1, a compaction that keeps +inf rows;
  - the guided window contains the unguided answer for every named key at every (n, nb) the GPU module uses.
"""
import os

import numpy as np
import pytest

import resample_ref as R

LD = R.LD
GUIDED = [(131072, 131072 // 4), (131074, 131074 // 4), (300001, 300001 // 4), (131072, 131072), (131071, 131071), (131073, 131073)]
SEARCH_LAWS = ("smooth", "zeros70", "heavy", "zeros_tail", "first_only", "last_only")


# ---- an fp64 model of the fast kernels' order of additions -----------------------------------------------------------------------------
def _hillis_steele(a):
    """Inclusive scan over the last axis (64 lanes) as __shfl_up does it."""
    inc = a.copy()
    o = 1
    while o < inc.shape[-1]:
        nxt = inc.copy()
        nxt[..., o:] = inc[..., o:] + inc[..., :-o]
        inc, o = nxt, o * 2
    return inc


def _running_max(a):
    return np.maximum.accumulate(a, axis=-1)


def model_fast_cdf(w, carry=0.0, fixed=True, tile_carry=True):
    """(cdf, total) as k_tile_sum / k_scan_tiles / k_tile_scan form them.  fixed=False: the scan those kernels held before
    (`inc - v` / `inc - acc` for the exclusive prefixes, no maxima or clamps, the last element from its own tree).
    tile_carry=False plants the mistake of a tile prefix without the chunk's carry."""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    T = (n + R.SCAN_TILE - 1) // R.SCAN_TILE
    v = np.cumsum(np.concatenate([w, np.zeros(T * R.SCAN_TILE - n)]).reshape(T, 4, 64, 8), axis=3)  # serial sums of a thread
    acc = v[..., 7]
    # k_tile_sum: xor butterfly over the wave, then ((s0 + s1) + s2) + s3
    b = acc.copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        b = b + b[..., lane ^ o]
    sums = ((b[:, 0, 0] + b[:, 1, 0]) + b[:, 2, 0]) + b[:, 3, 0]
    # k_scan_tiles: chunks of 1024 tiles, 16 waves of 64
    pre = np.empty(T)
    s_carry = np.float64(carry)
    for start in range(0, T, 1024):
        t = np.zeros(1024)
        m = min(1024, T - start)
        t[:m] = sums[start:start + m]
        inc = _hillis_steele(t.reshape(16, 64))
        wp = np.empty(16)
        run = s_carry if tile_carry else np.float64(0.0)
        for k in range(16):
            wp[k] = run
            run = run + inc[k, 63]
        if fixed:
            incl = np.maximum(_running_max((wp[:, None] + inc).reshape(-1)), s_carry)
            ex = np.concatenate([[s_carry], incl[:-1]])
            pre[start:start + m] = ex[:m]
            s_carry = incl[-1]
        else:
            pre[start:start + m] = (wp[:, None] + (inc - t.reshape(16, 64))).reshape(-1)[:m]
            s_carry = wp[15] + inc[15, 63]
    total = s_carry
    # k_tile_scan
    inc = _hillis_steele(acc)
    off = np.empty((T, 4))
    run = pre.copy()
    for k in range(4):
        off[:, k] = run
        run = run + inc[:, k, 63]
    if fixed:
        ex = np.concatenate([np.zeros((T, 4, 1)), inc[..., :-1]], axis=2)
        x = ((off[:, :, None] + ex)[..., None] + v).reshape(T, -1)
        last = x.reshape(T, 256, 8)[..., 7]
        floor = np.concatenate([pre[:, None], _running_max(last)[:, :-1]], axis=1)
        floor = np.maximum(floor, pre[:, None])
        hi = np.concatenate([pre[1:], [total]])
        x = np.minimum(np.maximum(x.reshape(T, 256, 8), floor[..., None]), hi[:, None, None]).reshape(-1)[:n]
        x[n - 1] = total
    else:
        x = ((off[:, :, None] + (inc - acc))[..., None] + v).reshape(-1)[:n]
    return x, total


def test_model_of_the_fixed_kernels_meets_tolerance_and_contract_on_every_law():
    worst = 0.0
    for law in R.LAWS:
        for n in (1, 7, 2047, 2048, 2049, 100003):
            for carry in (0.0, 0.37):
                w = R.weights(law, n, 3)
                x, total = model_fast_cdf(w, carry)
                ref, tol = R.fast_tol(w, carry)
                worst = max(worst, R.units(x, ref, tol))
                assert np.all(np.diff(x) >= 0) and x[-1] == total, (law, n, carry)
                if n > 1 and law == "dominant" and carry == 0.0:
                    k = R.dominant_index(n)
                    assert x[k - 1] > 0 and abs(x[k - 1] - float(ref[k - 1])) <= float(tol[k - 1]) and float(tol[k - 1]) < 1e-13 * float(ref[k - 1])
    assert worst < 1, worst


def test_model_of_the_former_kernels_breaks_each_part_of_the_contract():
    """The three violations the issue predicts for `inc - acc`: a last element that is not the total, a decrease where weights are
    exactly zero, and a lost prefix in front of a dominant weight (relative error 1: far outside the tolerance, which is relative
    to the element's own value)."""
    last_differs = decreases = 0
    for law in ("smooth", "zeros70", "heavy"):
        for seed in range(3):
            w = R.weights(law, 100003, seed)
            x, total = model_fast_cdf(w, fixed=False)
            last_differs += x[-1] != total
            decreases += int(np.sum(np.diff(x) < 0))
    assert last_differs > 0 and decreases > 0, (last_differs, decreases)
    w = R.weights("dominant", 2049, 0)
    k = R.dominant_index(2049)
    x, _ = model_fast_cdf(w, fixed=False)
    ref, tol = R.fast_tol(w)
    lost = np.abs(x[:k] - ref[:k]) > tol[:k]
    assert lost.any() and R.units(x, ref, tol) > 1e10
    # ... while the absolute error stays at the rounding level of the total, which is why no looser check saw it
    assert float(np.max(np.abs(x - ref))) <= 64 * R.U * float(ref[-1])


def test_numpy_cumsum_lies_inside_the_fast_tolerance():
    for law in R.LAWS:
        for n in (1, 7, 44):  # k - 1 <= 43 = A sequential additions: inside by the same argument, whatever the weights
            for carry, norm in ((0.0, False), (0.37, False), (0.0, True)):
                w = R.weights(law, n, 5)
                ref, tol = R.fast_tol(w, carry, norm)
                got = R.exact_cdf(w, carry, norm)
                if norm and law == "all_zero":
                    assert np.all(np.isnan(got)) and np.all(np.isnan(ref.astype(np.float64)))
                    continue
                assert R.units(got, ref, tol) < 1, (law, n, carry, norm, R.units(got, ref, tol))


def test_fast_additions_counts_the_chunks():
    assert R.fast_additions(1) == R.fast_additions(1024 * 2048) == 43
    assert R.fast_additions(1024 * 2048 + 1) == 59


def test_a_tile_prefix_without_its_carry_lands_outside():
    w = R.weights("smooth", 4097, 1)
    ref, tol = R.fast_tol(w, 0.37)
    assert R.units(model_fast_cdf(w, 0.37)[0], ref, tol) < 1
    assert R.units(model_fast_cdf(w, 0.37, tile_carry=False)[0], ref, tol) > 1e10


# ---- golden indices and the C oracle -------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_indices(golden):
    from conftest import synth

    g = golden["ref_resample"]
    for n, d, seed, b0, b, n_out in g["cases"]:
        n, d, seed, n_out = int(n), int(d), int(seed), int(n_out)
        x, ll, lp, lq = synth(n, d, seed)
        rng = np.random.default_rng(1000 + seed)
        u = R.pcg64_uniforms(rng, 0, n_out)
        idx = R.resample_indices(ll, lp, lq, b0, b, u)
        assert np.array_equal(idx, g[f"n{n}_b{b0}_t{b}_o{n_out}_idx"]), (n, b0, b, n_out)
        rng.bit_generator.advance(n_out)
        assert np.array_equal(rng.random(3), g[f"n{n}_b{b0}_t{b}_o{n_out}_next_u"])


def test_restatement_reproduces_the_c_oracle(oracle):
    from conftest import synth

    g = np.random.default_rng(2)
    for n, n_out in ((10, 20), (2049, 4099), (65537, 1000)):
        x, ll, lp, lq = synth(n, 3, 40 + n)
        u = g.random(n_out)
        assert np.array_equal(R.resample_indices(ll, lp, lq, 0.0, 0.07, u), oracle.resample_indices(ll, lp, lq, 0.0, 0.07, u))
        ll[g.integers(0, n, n // 7)] = -np.inf
        lp[g.integers(0, n, n // 9)] = np.inf
        ll[1], lp[1] = 0.5, np.inf  # (a row only the planted mistake keeps)
        ll[g.integers(0, n, 3)] = np.nan
        lq[g.integers(0, n, 3)] = np.nan  # (log q plays no part)
        for a, b in zip(R.compact(x, ll, lp, lq), oracle.compact_valid(x, ll, lp, lq)):
            assert R.bits_equal(a, b)
        assert any(a.shape != b.shape for a, b in zip(R.compact(x, ll, lp, lq, keep_pos_inf=True), oracle.compact_valid(x, ll, lp, lq)))
    for n_out, u0 in ((1, 0.25), (1025, 0.999), (7, 0.0)):
        assert np.array_equal(R.systematic(n_out, 0, n_out, u0), oracle.systematic_uniforms(n_out, u0))
        v = g.random(n_out)
        assert np.array_equal(R.systematic(n_out, 0, n_out, v=v), oracle.stratified_uniforms(v))
    # a slice of a larger set of slots is the same numbers
    assert np.array_equal(R.systematic(100, 37, 1025, 0.3), R.systematic(1025, 0, 1025, 0.3)[37:137])


def test_pcg64_offsets_continue_the_stream():
    rng = np.random.default_rng(11)
    full = np.random.default_rng(11).random(70000)
    assert np.array_equal(R.pcg64_uniforms(rng, 65535, 100), full[65535:65635])
    assert np.array_equal(rng.random(4), full[:4])  # the generator was not touched
    a = R.pcg64_uniforms(np.random.default_rng(11), 2 ** 40 + 1, 5)
    bg = np.random.PCG64(11)
    bg.advance(2 ** 40)
    assert np.array_equal(np.random.Generator(bg).random(6)[1:], a)
    st = R.pcg64_state(np.random.default_rng(11))
    assert st.dtype == np.uint64 and st.shape == (4,) and int(st[3]) & 1 == 1  # (an LCG increment is odd)


# ---- search ----------------------------------------------------------------------------------------------------------------------------------
def _cdf(law, n, seed=2):
    return R.exact_cdf(R.weights(law, n, seed), normalize=True)


def test_search_counts_entries_not_above_the_key_and_left_lands_outside():
    for law in SEARCH_LAWS:
        for n in (1, 5, 300):
            cdf = _cdf(law, n)
            u = R.all_keys(cdf, (max(n // 4, 1), n))
            brute = np.array([np.sum(cdf <= k) if not np.isnan(k) else n for k in u])
            assert np.array_equal(R.search(cdf, u), brute), (law, n)
            dev = R.search_device(cdf, u)
            assert np.all(dev[np.isnan(u)] == 0) and np.all(dev[u < 1.0] < n) and np.array_equal(dev[u >= 1.0], brute[u >= 1.0])
            assert np.array_equal(dev[~np.isnan(u)], brute[~np.isnan(u)])  # on a cdf that ends at 1 the clamp never acts
    cdf = _cdf("zeros70", 300)
    u = R.keys(cdf)["hits"]
    assert not np.array_equal(np.searchsorted(cdf, u, side="left"), R.search(cdf, u))
    # the clamp acts on a cdf whose last element stayed below 1
    short = cdf * (1.0 - 2.0 ** -52)
    assert R.search(short, [np.nextafter(1.0, 0.0)])[0] == 300 and R.search_device(short, [np.nextafter(1.0, 0.0)])[0] == 299


@pytest.mark.parametrize("n,nb", GUIDED)
def test_guided_window_contains_the_answer_for_every_named_key(n, nb):
    for law in SEARCH_LAWS:
        cdf = _cdf(law, n)
        G = R.guide(cdf, nb)
        assert G[0] == np.sum(cdf <= 0.0) and G[nb] == n and np.all(np.diff(G) >= 0)
        u = np.concatenate([R.all_keys(cdf, (nb,)), np.random.default_rng(n).random(20000)])
        inside = (u >= 0.0) & (u < 1.0)
        b = R.bucket(u[inside], nb)
        fnb = np.float64(nb)
        assert np.all(b / fnb <= u[inside]) and np.all(u[inside] < (b + 1) / fnb)  # the bucket rule, in the kernels' expressions
        lo, hi = R.guided_window(cdf, u, nb, G)
        ans = R.search(cdf, u)
        ok = ~np.isnan(u)
        assert np.all(lo[ok] <= ans[ok]) and np.all(ans[ok] <= hi[ok]), (law, n, nb)
        assert np.array_equal(R.guided_search(cdf, u, nb, G), R.search_device(cdf, u))


def test_a_guide_built_with_less_than_is_not_the_table():
    """G'[b] = #{cdf < b / nb} differs from the table wherever a cdf value IS some b / nb (`equal` at a power of two: all of them).
    Its windows still contain the answer (they only open further down), so indices cannot show this mistake; the table's
    definition does.  (The table's contents cannot be read back from the device: only indices are compared there.)"""
    cdf = R.exact_cdf(R.weights("equal", 64), normalize=True)
    G, Gl = R.guide(cdf, 16), R.guide(cdf, 16, side="left")
    brute = np.array([np.sum(cdf <= b / 16.0) for b in range(17)])
    assert np.array_equal(G, brute) and not np.array_equal(Gl, brute)
    u = R.all_keys(cdf, (16,))
    assert np.array_equal(R.guided_search(cdf, u, 16, Gl), R.search_device(cdf, u))


@pytest.mark.parametrize("n,nb", [(300001, 300001 // 4), (75000, 75000)])
def test_a_bucket_without_the_settling_loops_fails_on_the_bucket_edges(n, nb):
    """On the staircase cdf (every value a bucket edge) with keys on and one ulp either side of every edge: the truncated product
    alone breaks the bucket rule, and where it lands one bucket too high the window opens above the answer."""
    cdf = R.staircase_cdf(n, nb)
    u = R.edge_keys(nb)
    raw, b = R.bucket(u, nb, settle=False), R.bucket(u, nb)
    fnb = np.float64(nb)
    assert np.all(b / fnb <= u) and np.all(u < (b + 1) / fnb)
    broken = ~((raw / fnb <= u) & (u < (raw + 1) / fnb))
    assert broken.any() and not np.array_equal(raw, b)
    assert not np.array_equal(R.guided_search(cdf, u, nb, settle=False), R.search(cdf, u))
    assert np.array_equal(R.guided_search(cdf, u, nb), R.search(cdf, u))


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def test_gather_stride_and_bit_copies(oracle):
    g = np.random.default_rng(4)
    n, d = 300, 6
    x = g.normal(size=(n, d))
    x[3, 2], x[5, 0], x[7, 1] = np.nan, np.inf, -np.inf
    x[9] = np.frombuffer(np.array([0x7FF8000000000123] * d, dtype=np.uint64).tobytes(), dtype=np.float64)  # a NaN with a payload
    ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
    idx = np.concatenate([[0, n - 1, 9, 9, 3, 5, 7], g.integers(0, n, 500)])
    got = R.gather(idx, x, ll, lp, lq)
    for a, b in zip(got, oracle.gather_rows(idx, x, ll, lp, lq)):
        assert R.bits_equal(a, b)
    assert not R.bits_equal(R.gather(idx, x, ll, lp, lq, stride=d - 1)[0], got[0])
    s, sabs = R.colsum(np.nan_to_num(got[0], nan=0.0, posinf=0.0, neginf=0.0))
    assert s.dtype == LD and np.all(sabs >= np.abs(s))


def test_select_range_edges():
    u = np.array([0.0, 0.25, 0.5, np.nextafter(0.5, 0), 0.75, 1.0, np.nan])
    assert np.array_equal(R.select_range(u, 0.25, 0.5), [0.25, np.nextafter(0.5, 0)])
    assert R.select_range(u, 0.5, 0.5).size == 0 and R.select_range(u, 0.0, 2.0).size == 6


def test_named_laws_are_what_their_names_say():
    n = 100003
    assert abs(np.mean(R.weights("zeros70", n) == 0) - 0.7) < 0.01
    w = R.weights("dominant", n)
    assert R.dominant_index(n) % 8 == 3 and R.dominant_index(n) // 8 % 64 == 37 and w[R.dominant_index(n)] == 1e30 and np.sum(w == 1e-30) == n - 1
    assert np.all(R.weights("zeros_tail", n)[-3000:] == 0) and R.weights("zeros_tail", n)[-3001] > 0
    assert np.flatnonzero(R.weights("first_only", n)).tolist() == [0] and np.flatnonzero(R.weights("last_only", n)).tolist() == [n - 1]
    assert not R.weights("all_zero", 7).any() and R.weights("zeros_tail", 1)[0] > 0
