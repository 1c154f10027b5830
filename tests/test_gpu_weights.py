"""The weight, ESS and temperature-search kernels of csrc/asmc_weights.hip, asmc_search.hip and asmc_is_weights.hip on every dispatch path and at the edges, against the
long-double restatement of tests/weights_ref.py (tolerance formulas: its docstring and DESIGN.md section 3.16; none comes from the
device's output).

Shape -> path (CU = the device's compute units, read from the device; every case asserts, from profile_variants, the symbol that ran):

  k_weights_max<KT>, k_weights_sums<KT>   KT = the power of two >= K; grid = min(ceil(n / per), 4 CU), per = 2048 (KT < 16), 1024
                                          (KT >= 16); one more trip per lane above 4 CU per: KT >= 16 at n = 4 CU 1024 + 1 on the
                                          suite's engine, KT < 16 at 4 CU 2048 + 5 on an engine of its own
  k_finalize_columns                      behind every reduction; 2 KT columns, lane l adds the block records l, l + 64, ... (KT = 32 at
                                          the full grid: 4 CU records per column, more than 64)
  k_weights_m2, k_weights_m2_lse          grid as KT = 1
  k_weights_map<0 | 1>                    grid = min(ceil(n / 1024), 2048): a second trip above 2^21
  k_count_nonfinite                       grid = min(ceil(n / 2048), 2048): a second trip above 2^22; two counter slots in turn
  k_bis_sums (asmc_find_beta)             grid = min(ceil(n / 512), CU), two particles per trip
  k_is_weights<true>                      n <= 4096 CU (one chunk per block, particles resident in LDS)
  k_is_weights<false>                     n > 4096 CU (streaming)
  k_bis_sums + k_bis_decide, k_weights_m2_lse_shard, k_weights_map_shard   the sharded forms, emulated ranks on one device

Every case prints its tolerance and the device's worst error in units of it (pytest -s).  The non-finite pattern of every
output must be the restatement's exactly, and every finite element is compared.  beta*, the flags and the shifts are compared bit
for bit on decidable cases (weights_ref.decide).

Measured on an MI355X (DESIGN.md section 3.16 has the full list): device exp against long double 0.86 ulp at worst; worst error in
units of the tolerance: k_weights_max/sums 0.20 (0.11 on the fifth trip at KT = 32), second trip of KT < 16 0.009, m2 / m2_lse /
k_weights_map<1> 0.06 .. 0.35 on the ordinary populations, the weights 0.88 at most (where |lw + shift| is of order 1e4: its two roundings are most of the bound), k_bis_sums 0.10 over
63 named and 100 random cases (none undecidable), k_is_weights<true> with tile sums and cumulative sums 0.22, <false> 0.16, sharded
forms 0.24, with a dead rank 0.19.  Against the parent's kernels six sharded cases fail (a rank whose rows are all -inf gave NaN sums on
every rank).  Total time of the module: 12 s for 75 tests (the child process 3 s).
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import weights_ref as W

pytestmark = pytest.mark.gpu
LD = W.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_weights_", "k_finalize_columns", "k_count_nonfinite", "k_bis_", "k_is_weights")
RAN = set()  # (kernel name, template arguments) an asserted launch has covered (test_every_kernel_symbol_ran closes the module)


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(scope="module")
def cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def big(cu):
    """An engine above every second-trip threshold of the KT < 16 kernels (the suite's engine ends at 2^21)."""
    from aspire_amd.engine import HipEngine

    e = HipEngine(0, n_max=max(4 * cu * 2048, 1 << 22) + 4096, d_max=1)
    yield e
    e.close()


def sym(name, targs=None):
    return f"_Z{len(name)}{name}" + ("" if targs is None else f"I{targs}E")


def ran(eng, fn, expect):
    """fn() with the assertion that, of this module's kernel families, exactly the symbols `expect` ran ({(name, template
    arguments or None): launches})."""
    eng.profile(True)
    try:
        out = fn()
        var = {s: c for s, c in eng.profile_variants().items() if any(f in s for f in FAMILIES)}
    finally:
        eng.profile(False)
    want = {sym(*k): c for k, c in expect.items()}
    for s in var:  # (the length in front of a mangled name keeps k_weights_m2 and k_weights_m2_lse apart)
        assert any(s.startswith(p) for p in want), (s, want)
    for p, cnt in want.items():
        got = sum(c for s, c in var.items() if s.startswith(p))
        assert cnt is None and got > 0 or got == cnt, (p, cnt, var)
    RAN.update((k[0], k[1] if len(k) > 1 else None) for k in expect)
    return out


def dev(eng, *arrs):
    return tuple(eng.asarray(np.ascontiguousarray(a, dtype=np.float64)) for a in arrs)


def report(label, worst, extra=""):
    print(f"{label}: worst error {worst:.3g} of the tolerance {extra}")
    assert worst < 1, (label, worst)


def tiled(kind, n, base=4099, seed=3):
    """A population of n rows built from `base` distinct ones (row i = base row i mod base): the long-double sums cost `base`
    exponentials.  Returns (ll, lp, lq, index of every row's base row)."""
    bl, bp, bq = W.population(kind, base, seed)
    idx = np.arange(n) % base
    return bl[idx], bp[idx], bq[idx], idx


# ---- the device exp ---------------------------------------------------------------------------------------------------------------------
def test_device_exp_error_is_within_the_figure_the_tolerances_assume(eng):
    """exp(t) of k_weights_map<1> (shift = 0, lse = m) against long double over the arguments t = lw - m of every population: the
    worst error in ulps must stay within twice the figure weights_ref.EXP_ULPS_MEASURED records (= the E of every tolerance)."""
    worst = 0.0
    for kind in W.POPULATIONS:
        ll, lp, lq = W.population(kind, 30011, 21)
        for b0, b in ((0.0, 0.03), (0.0, 1.0), (0.4, 0.41)):
            lw = W.log_weights(ll, lp, lq, b0, b)
            m, _ = W.max_and_nan(lw)
            if not math.isfinite(m):
                continue
            got = ran(eng, lambda: eng.normalized_weights(*dev(eng, ll, lp, lq), b0, b, 0.0, m), {("k_weights_map", "Li1"): 1}).cpu().numpy()
            with np.errstate(all="ignore"):
                t = lw - m
                ref = np.exp(t.astype(LD))
            ok = ref >= LD(2.0 ** -1021)  # normal results (a subnormal's ulp is not a relative error)
            worst = max(worst, float(np.max(np.abs(got[ok] - ref[ok]) / W.ulp64(ref[ok].astype(np.float64)))))
            assert np.all(np.abs(got[~ok] - ref[~ok]) <= W.SUBNORMAL_FLOOR + ref[~ok] * LD(W.EXP_REL))
    print(f"device exp: worst error {worst:.4f} ulp over the suite's arguments (recorded: {W.EXP_ULPS_MEASURED})")
    assert worst * 2 * W.U <= W.EXP_REL


# ---- log-weights and maxima: bit for bit ------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 257, 2047, 2049)


def _nonfinite_rows(n):
    """(ll, lp, lq) with every class of the contract table among ordinary rows."""
    g = np.random.default_rng(n)
    ll, lp, lq = g.normal(size=n), g.normal(size=n), g.normal(size=n)
    for k, (a, q) in enumerate(((-np.inf, 0.0), (np.inf, 0.0), (np.inf, np.inf), (np.nan, 0.0), (0.0, -np.inf), (-np.inf, -np.inf))):
        if 7 * k + 3 < n:
            ll[7 * k + 3], lq[7 * k + 3] = a, q
    return ll, lp, lq


@pytest.mark.parametrize("n", SIZES + (30011,))
def test_log_weights_bit_for_bit(eng, n):
    for ll, lp, lq in (W.population("heavy", n, 1), W.population("offset1e6", n, 1), _nonfinite_rows(n)):
        d = dev(eng, ll, lp, lq)
        for b0, b, shift in ((0.0, 0.37, 0.0), (0.4, 1.0, -3.25), (float(np.nextafter(1.0, 0.0)), 1.0, 1e3), (0.3, 0.3, 0.5)):
            got = ran(eng, lambda: eng.log_weights(*d, b0, b, shift), {("k_weights_map", "Li0"): 1}).cpu().numpy()
            ref = W.log_weights(ll, lp, lq, b0, b, shift)
            assert W.same_nonfinite(got, ref)
            fin = np.isfinite(ref)
            assert np.array_equal(got[fin], ref[fin]), np.flatnonzero(got != ref)[:5]


def _betas(K, b0):
    return b0 + (1.0 - b0) * (np.arange(1, K + 1) / K) ** 2


def _check_stats(eng, cu, ll, lp, lq, b0, K, label, counts=None, base=None):
    """weights_max, weights_stats (m from the keys) and weights_sums (host m and a shift) of K candidates against the
    restatement; returns the worst error in units of the tolerance."""
    n, kt = len(ll), W.bucket_of(K)
    d = dev(eng, ll, lp, lq)
    betas = _betas(K, b0)
    L = W.chain_len(n, cu, kt)
    m_dev, nan_dev = ran(eng, lambda: eng.weights_max(*d, b0, betas), {("k_weights_max", f"Li{kt}"): 1})
    full = ran(eng, lambda: eng.weights_stats(*d, b0, betas), {("k_weights_max", f"Li{kt}"): 1, ("k_weights_sums", f"Li{kt}"): 1, ("k_finalize_columns",): 1})
    shifts = np.linspace(-2.0, 3.0, K)
    bl, bp, bq = (ll, lp, lq) if base is None else base
    worst, ms, nn = 0.0, [], 0
    for k, b in enumerate(betas):
        lw = W.log_weights(bl, bp, bq, b0, b)
        m, n_nan = W.max_and_nan(lw)
        nn += n_nan if counts is None else int(counts[np.isnan(lw)].sum())
        ms.append(m)
        assert m_dev[k] == m and full[k, 0] == m, (label, k, m_dev[k], full[k, 0], m)
        S1, S2, t1, t2 = W.sums(lw, m, 0.0, L, counts)
        for got, ref, tol in ((full[k, 1], S1, t1), (full[k, 2], S2, t2)):
            assert W.same_nonfinite(np.float64(got), np.float64(ref)), (label, k, got, ref)
            if np.isfinite(np.float64(ref)):
                worst = max(worst, W.units(got, ref, tol))
    # (the census counts a NaN log-weight once per candidate, padding candidates included: kt / K copies of the last one)
    pad_nan = (kt - K) * (W.max_and_nan(W.log_weights(bl, bp, bq, b0, betas[-1]))[1] if counts is None else
                          int(counts[np.isnan(W.log_weights(bl, bp, bq, b0, betas[-1]))].sum()))
    assert nan_dev == nn + pad_nan and np.all(full[:, 3] == nn + pad_nan), (label, nan_dev, nn, pad_nan)
    if all(math.isfinite(m) for m in ms):
        mh = np.array(ms) + 0.125  # a host-supplied m that is not the maximum, and a shift
        got = ran(eng, lambda: eng.weights_sums(*d, b0, betas, mh, shifts), {("k_weights_sums", f"Li{kt}"): 1, ("k_finalize_columns",): 1})
        for k, b in enumerate(betas):
            S1, S2, t1, t2 = W.sums(W.log_weights(bl, bp, bq, b0, b), mh[k], shifts[k], L, counts)
            worst = max(worst, W.units(got[k, 0], S1, t1), W.units(got[k, 1], S2, t2))
    return worst


@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 17, 32])
def test_max_and_sums_every_bucket_and_size(eng, cu, K):
    kinds = ("synth", "heavy", "peaked3e4", "dominant", "neginf20", "neginf_lanes", "offset1e6", "sorted_down", "uniform", "neginf_chunk")
    per = 1024 if W.bucket_of(K) >= 16 else 2048
    worst = 0.0
    for i, n in enumerate(SIZES + (per - 1, per + 1, 3 * per + 1)):
        ll, lp, lq = W.population(kinds[(i + K) % len(kinds)], n, 30 + K)
        worst = max(worst, _check_stats(eng, cu, ll, lp, lq, (0.0, 0.3)[i % 2], K, f"K={K} n={n}"))
    # rows of every non-finite class: the census, the maxima and the NaN / inf pattern of the sums
    _check_stats(eng, cu, *_nonfinite_rows(257), 0.0, K, f"K={K} non-finite rows")
    _check_stats(eng, cu, *W.population("neginf_all", 300, 1), 0.0, K, f"K={K} every row -inf")
    report(f"k_weights_max/sums<{W.bucket_of(K)}> K={K}", worst, f"(L = {W.chain_len(3 * per + 1, cu, W.bucket_of(K))})")


@pytest.mark.parametrize("K", [17, 32])
def test_sums_second_trip_at_sixteen_and_more_candidates(eng, cu, K):
    """n just above 4 CU x 1024: the lanes of the first blocks take one more trip; K = 32 at the full grid also gives
    k_finalize_columns 4 CU records per column, more than the 64 its lanes take at once."""
    n = 4 * cu * 1024 + 1
    ll, lp, lq, idx = tiled("heavy", n)
    counts = np.bincount(idx, minlength=4099)
    worst = _check_stats(eng, cu, ll, lp, lq, 0.0, K, f"K={K} n={n}", counts=counts, base=W.population("heavy", 4099, 3))
    assert W.reduce_grid(n, cu, 32) == 4 * cu and (n + 4 * cu * 256 - 1) // (4 * cu * 256) == 5
    report(f"second trip K={K} n={n}", worst)


def _planted(n, first):
    """synth rows (tiled) with a -inf row at `first` and a dominant last row, both in the range only a further trip reaches: a
    skipped tail shows in the maximum, the sums and the map's output (the callers plant their NaN row there themselves)."""
    ll, lp, lq, idx = tiled("synth", n)
    ll, lp, lq = ll.copy(), lp.copy(), lq.copy()
    ll[first], ll[n - 1] = -np.inf, ll[n - 1] + 40.0
    return ll, lp, lq


def test_second_trip_below_sixteen_candidates(big, cu):
    """KT < 16 on an engine of its own: n = 4 CU x 2048 + 5 (reductions), 2^21 + 5 (maps), 2^22 + 3 (census)."""
    worst = {}
    n = 4 * cu * 2048 + 5
    first = 4 * cu * 2048
    ll, lp, lq = _planted(n, first)
    d = dev(big, ll, lp, lq)
    b0, b = 0.0, 0.3
    lw = W.log_weights(ll, lp, lq, b0, b)
    m, _ = W.max_and_nan(lw)
    assert np.argmax(lw) == n - 1
    L = W.chain_len(n, cu)
    full = ran(big, lambda: big.weights_stats(*d, b0, [b, 1.0, 0.01]), {("k_weights_max", "Li4"): 1, ("k_weights_sums", "Li4"): 1, ("k_finalize_columns",): 1})
    assert full[0, 0] == m and full[0, 3] == 0
    lwu, inv, counts = np.unique(lw, return_inverse=True, return_counts=True)
    S1, S2, t1, t2 = W.sums(lwu, m, 0.0, L, counts)
    worst["sums"] = max(W.units(full[0, 1], S1, t1), W.units(full[0, 2], S2, t2))
    mean_u = float(S1 / LD(n))
    shift = float((m + math.log(float(S1))) - math.log(n))
    mp = m + shift
    m2, S1p, tm2, t1p = W.m2_lse(lwu, m, mean_u, shift, mp, L, counts)
    got = ran(big, lambda: big.weights_m2(*d, b0, b, m, mean_u), {("k_weights_m2",): 1, ("k_finalize_columns",): 1})
    worst["m2"] = W.units(got, m2, tm2)
    got = ran(big, lambda: big.weights_m2_lse(*d, b0, b, m, mean_u, shift, mp), {("k_weights_m2_lse",): 1, ("k_finalize_columns",): 1})
    worst["m2_lse"] = max(W.units(got[0], m2, tm2), W.units(got[1], S1p, t1p))
    # NaN in the tail: the census of the max kernel
    ll2 = ll.copy()
    ll2[n - 2] = np.nan
    _, nn = ran(big, lambda: big.weights_max(big.asarray(ll2), d[1], d[2], b0, [b]), {("k_weights_max", "Li1"): 1})
    assert nn == 1
    # maps: a second trip above 2048 blocks x 1024
    n = (1 << 21) + 5
    ll, lp, lq = _planted(n, 1 << 21)
    ll[n - 3] = np.nan
    d = dev(big, ll, lp, lq)
    got = ran(big, lambda: big.log_weights(*d, b0, b, 0.5), {("k_weights_map", "Li0"): 1}).cpu().numpy()
    ref = W.log_weights(ll, lp, lq, b0, b, 0.5)
    assert W.same_nonfinite(got, ref) and np.array_equal(got[np.isfinite(ref)], ref[np.isfinite(ref)])
    lse = 1.75
    got = ran(big, lambda: big.normalized_weights(*d, b0, b, 0.5, lse), {("k_weights_map", "Li1"): 1}).cpu().numpy()
    with np.errstate(all="ignore"):
        a = ref - lse
        refu, inv = np.unique(a, return_inverse=True)
        want = np.exp(refu.astype(LD))[inv]
    assert W.same_nonfinite(got, want.astype(np.float64))
    fin = np.isfinite(a)
    worst["map<1>"] = W.units(got[fin], want[fin], want[fin] * LD(W.EXP_REL) + W.SUBNORMAL_FLOOR)
    assert got[1 << 21] == 0.0 and math.isnan(got[n - 3])
    # census: a second trip above 2048 blocks x 2048, three calls in a row (both slots and the hand-over)
    import torch

    n = (1 << 22) + 3
    v = torch.zeros(n, dtype=torch.float64, device=big.device)
    v[n - 1], v[n - 2], v[5] = float("nan"), float("inf"), float("-inf")
    assert ran(big, lambda: big.count_nonfinite(v), {("k_count_nonfinite",): 1}) == (1, 2)
    assert ran(big, lambda: big.count_nonfinite(v[: 1 << 22].contiguous()), {("k_count_nonfinite",): 1}) == (0, 1)  # the tail's are gone
    clean = torch.ones(n, dtype=torch.float64, device=big.device)
    assert ran(big, lambda: big.count_nonfinite(clean), {("k_count_nonfinite",): 1}) == (0, 0)  # a second trip that finds nothing
    v[n - 3] = float("nan")
    assert ran(big, lambda: big.count_nonfinite(v), {("k_count_nonfinite",): 1}) == (2, 2)
    assert ran(big, lambda: big.count_nonfinite(clean), {("k_count_nonfinite",): 1}) == (0, 0)
    for k, wv in worst.items():
        print(f"second trip {k}: worst error {wv:.3g} of the tolerance")
    assert max(worst.values()) < 1, worst


def test_count_nonfinite_both_slots_and_a_clean_call(eng):
    g = np.random.default_rng(4)
    v = g.normal(size=70001)
    a = v.copy()
    a[[0, 63, 64, 70000]] = np.nan
    a[[1, 4096]] = np.inf
    b = v.copy()
    b[[255, 256, 257]] = -np.inf
    seq = [(a, (4, 2)), (v, (0, 0)), (b, (0, 3)), (v, (0, 0)), (v, (0, 0)), (a, (4, 2)), (a[:1], (1, 0)), (b[:300], (0, 3))]
    for arr, want in seq:
        assert ran(eng, lambda: eng.count_nonfinite(eng.asarray(arr)), {("k_count_nonfinite",): 1}) == want


# ---- direct evidence moments and weights on every population --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", W.POPULATIONS)
def test_m2_lse_and_normalized_weights(eng, cu, kind):
    worst = 0.0
    for n in (1, 65, 2049, 30011):
        ll, lp, lq = W.population(kind, n, 7)
        d = dev(eng, ll, lp, lq)
        for b0, b in ((0.0, 0.07), (0.3, 1.0)):
            lw = W.log_weights(ll, lp, lq, b0, b)
            m, _ = W.max_and_nan(lw)
            if not math.isfinite(m):
                continue
            L = W.chain_len(n, cu)
            S1 = W.sums(lw, m, 0.0, L)[0]
            mean_u = float(S1 / LD(n))
            shift = float((m + math.log(float(S1))) - math.log(n))
            mp = m + shift
            m2, S1p, tm2, t1p = W.m2_lse(lw, m, mean_u, shift, mp, L)
            got = ran(eng, lambda: eng.weights_m2(*d, b0, b, m, mean_u), {("k_weights_m2",): 1, ("k_finalize_columns",): 1})
            worst = max(worst, W.units(got, m2, tm2))
            got = ran(eng, lambda: eng.weights_m2_lse(*d, b0, b, m, mean_u, shift, mp), {("k_weights_m2_lse",): 1, ("k_finalize_columns",): 1})
            worst = max(worst, W.units(got[0], m2, tm2), W.units(got[1], S1p, t1p))
            lse = mp + math.log(got[1])
            w = ran(eng, lambda: eng.normalized_weights(*d, b0, b, shift, lse), {("k_weights_map", "Li1"): 1}).cpu().numpy()
            ref, tw = W.normalized_weights(ll, lp, lq, b0, b, L)
            assert W.same_nonfinite(w, ref.astype(np.float64)) and np.all(w[lw == -np.inf] == 0.0)
            worst = max(worst, W.units(w, ref, tw))
    report(f"m2 / m2_lse / map<1> {kind}", worst)


# ---- the search ---------------------------------------------------------------------------------------------------------------------------
def _ess_over_n_tol(m, S1, S2, t1, t2, n):
    """(ESS/N, its tolerance) for the device's ess_over_n: the sums' shares and, on the exponent 2 l1 - l2, the roundings of
    c = (m + log S1) - log N, mp = m + c, l1 = mp + log S1, l2 = 2 mp + log S2 and of the difference: eight operations (two
    logs of about an ulp, six additions), each at most u times the largest operand it sees, which 2 |l1| + |l2| + |m| + |c| + 2
    bounds - hence the factor 8."""
    with np.errstate(all="ignore"):
        ess = W.ess_ld(S1, S2) / LD(n)
        c = float(LD(m) + np.log(S1) - math.log(n))
        l1, l2 = abs(m + c) + abs(float(np.log(S1))), 2 * abs(m + c) + abs(float(np.log(S2)))
        return ess, W.ess_tol(S1, S2, t1, t2) / LD(n) + ess * LD(8 * W.U * (2 * l1 + l2 + abs(m) + abs(c) + 2))


def check_search(out, ll, lp, lq, case, cu, block_m=None, label="find_beta"):
    """A search result (engine.find_beta's tuple) against the restatement; returns the worst error in units of the tolerance, or
    None when the case is undecidable."""
    kind, n, seed, b0, target, tol = case
    b_dev, eff1, conv, rounds, n_nan, trip, trip_one = out
    lw1 = W.log_weights(ll, lp, lq, b0, 1.0)
    m_one, nn = W.max_and_nan(lw1)
    assert n_nan == nn and conv, (case, out)
    assert trip_one[0] == m_one or (math.isnan(trip_one[0]) and math.isnan(m_one)), (case, trip_one, m_one)
    L = W.bis_chain_len(n, cu)
    b_star, ok, margin = W.decided(case, 64)
    if not ok:
        return None
    assert b_dev == b_star, (case, b_dev, b_star, margin)
    # rounds: one when the first round settles it (beta* = 1, or 1 - beta0 within the tolerance).  Otherwise the plain search
    # resolves four of the loop's levels per round and may spend one more on the lower end's own sums or on a level the float
    # test adds or takes away (asmc_bisect.h); with prediction windows never more than one round above that
    levels = W.plain_levels(b0, tol)
    if b_star == 1.0 or levels == 0:
        assert rounds == 1, (case, rounds)
    elif os.environ.get("ASMC_BISECT_PLAIN"):
        assert math.ceil((levels - 1) / 4) <= rounds <= math.ceil(levels / 4) + 1, (case, rounds, levels)
    else:
        assert 1 <= rounds <= math.ceil(levels / 4) + 2, (case, rounds, levels)
    worst = 0.0
    bm = block_m
    S1, S2, t1, t2 = W.progression_sums(ll, lp, lq, b0, 1.0, m_one, L, bm, m_one)  # (first round: the level-4 grid)
    if label == "k_is_weights" and m_one == -math.inf:
        # pinned deviation: its blocks reduce against 0 when they hold no finite log-weight, so a population
        # without any reports the sums 0, 0 where the reference's log-sum-exp gives NaN; ESS is NaN and beta* = beta0 either way
        assert trip_one[1] == 0.0 and trip_one[2] == 0.0, (case, trip_one)
        S1 = S2 = LD(0)
    for got, ref, t in ((trip_one[1], S1, t1), (trip_one[2], S2, t2)):
        assert W.same_nonfinite(np.float64(got), np.float64(ref)), (case, got, ref)
        if np.isfinite(np.float64(ref)):
            worst = max(worst, W.units(got, ref, t))
    if np.isfinite(np.float64(S1)) and S1 > 0:  # (otherwise log(0) or NaN sums: NaN)
        ess, te = _ess_over_n_tol(m_one, S1, S2, t1, t2, n)
        worst = max(worst, W.units(eff1, ess, te))
    else:
        assert math.isnan(eff1), (case, eff1)
    # TRIP_OK: the triple at beta* exists exactly when the search moved off beta0 (or ended at 1)
    assert (trip is not None) == (b_star > b0), (case, trip)
    if trip is not None:
        m = m_one if b_star == 1.0 else W.node_shift(m_one, b_star, b0)
        assert trip[0] == m, (case, trip[0], m)
        S1, S2, t1, t2 = W.progression_sums(ll, lp, lq, b0, b_star, m, L, bm, m_one, None if b_star == 1.0 else tol)
        worst = max(worst, W.units(trip[1], S1, t1), W.units(trip[2], S2, t2))
    return worst


def _run_search_cases(eng, cu, cases, label):
    worst, left_out = 0.0, []
    for case in cases:
        kind, n, seed, b0, target, tol = case
        ll, lp, lq = W.population(kind, n, seed)
        d = dev(eng, ll, lp, lq)
        out = ran(eng, lambda: eng.find_beta(*d, b0, target, tol), {("k_weights_max", "Li1"): 1, ("k_bis_sums",): None})
        r = check_search(out, ll, lp, lq, case, cu)
        if r is None:
            left_out.append(case)
        else:
            if r > 0.5:
                print(f"  {case}: {r:.3g} of the tolerance, result {out}")
            worst = max(worst, r)
    report(f"{label}: {len(cases)} cases, {len(left_out)} undecidable", worst)
    return left_out


NAMED = W.named_search_cases()


@pytest.mark.parametrize("part", range(4))
def test_find_beta_named_cases(eng, cu, part):
    cases = [c for c in NAMED if c[1] < 100000][part::4]
    assert not _run_search_cases(eng, cu, cases, f"k_bis_sums named cases {part}")  # none of them may be left out


@pytest.mark.parametrize("case", [c for c in NAMED if c[1] > 100000], ids=lambda c: f"{c[0]}-{c[1]}")
def test_find_beta_one_and_two_passes(eng, cu, case):
    assert not _run_search_cases(eng, cu, [case], f"k_bis_sums {case[0]} n={case[1]}")


def test_find_beta_random_sweep(eng, cu):
    cases = W.random_search_cases()
    left_out = _run_search_cases(eng, cu, cases, "k_bis_sums random sweep")
    assert len(left_out) * 50 <= len(cases), left_out


def test_find_beta_nonfinite_contract(eng, cu):
    """The contract table: what the restated reference gives for every non-finite class."""
    for cls in W.NONFINITE_CLASSES:
        row = W.nonfinite_contract(cls)
        ll, lp, lq = W.nonfinite_case(cls)
        d = dev(eng, ll, lp, lq)
        b, eff1, conv, rounds, n_nan, trip, trip_one = ran(eng, lambda: eng.find_beta(*d, 0.0, 0.5, 1e-6),
                                                           {("k_weights_max", "Li1"): 1, ("k_bis_sums",): None})
        st = ran(eng, lambda: eng.weights_stats(*d, 0.0, [0.5]), {("k_weights_max", "Li1"): 1, ("k_weights_sums", "Li1"): 1, ("k_finalize_columns",): 1})[0]
        assert st[0] == row["m"] and st[3] == row["n_nan"]
        assert W.same_nonfinite(st[1:3], np.array([row["S1"], row["S2"]])), (cls, st, row)
        lw1 = W.log_weights(ll, lp, lq, 0.0, 1.0)
        m_one, nn = W.max_and_nan(lw1)
        assert n_nan == nn == row["n_nan"] and conv, (cls, n_nan, nn)
        assert trip_one[0] == m_one, (cls, trip_one)
        if row["raises"]:
            continue  # the reference raises on the NaN log-weight; the device reports the census, callers stop there
        assert b == row["beta_star"], (cls, b, row)
        assert (trip is not None) == row["found"], (cls, trip, row)
        if not math.isfinite(row["S1"]):
            assert math.isnan(trip_one[1]) and math.isnan(trip_one[2]) and math.isnan(eff1), (cls, trip_one, eff1)


PLAIN_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_weights as T, weights_ref as W
from aspire_amd.engine import HipEngine
eng = HipEngine(0, n_max=1 << 18, d_max=1)
cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
cases = [c for c in W.named_search_cases() if c[1] < 100000][::3] + [c for c in W.named_search_cases() if c[1] == 131073][:1]
left = T._run_search_cases(eng, cu, cases, "plain mode")
assert not left, left
print("PLAIN_OK", len(cases))
"""


def test_find_beta_plain_mode_in_a_child_process():
    """ASMC_BISECT_PLAIN (read once per process): the 16-ary search without prediction windows returns the same beta* and sums."""
    code = PLAIN_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ASMC_BISECT_PLAIN="1"), capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "PLAIN_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- the persistent importance step -----------------------------------------------------------------------------------------------------
def _is_step(eng, d, b0, target, tol, reg):
    from aspire_amd import smc_math

    st4 = smc_math.pcg64_state(np.random.default_rng(1))
    n = d[0].numel()

    def go():
        eng.importance_step(*d, b0, target, tol, st4, min(n, 64))
        return eng.importance_result()
    eng.profile(True)
    try:
        res = go()
        var = {s: c for s, c in eng.profile_variants().items() if "k_is_weights" in s}
    finally:
        eng.profile(False)
    want = sym("k_is_weights", "Lb1" if reg else "Lb0")
    assert list(var) and all(s.startswith(want) for s in var) and sum(var.values()) == 1, (var, want)
    RAN.add(("k_is_weights", "Lb1" if reg else "Lb0"))
    return res, eng._is_bufs["w"].cpu().numpy(), eng._is_bufs["cdf"].cpu().numpy(), eng.importance_tile_sums(n).cpu().numpy()


def _check_tiles(tiles, n, ref, tw):
    """k_is_weights' sums per scan tile (2048 particles: half a chunk; the last one partly empty) against the long-double sums of
    the restated weights: the weights' own tolerances plus the chain of 17 additions (4 per thread, 6 butterfly steps, 7 over
    the eight waves).  Returns the worst error in units of it."""
    assert len(tiles) == (n + W.SCAN_TILE - 1) // W.SCAN_TILE
    worst = 0.0
    for t, got in enumerate(tiles):
        seg = slice(t * W.SCAN_TILE, min(n, (t + 1) * W.SCAN_TILE))
        s_ref = ref[seg].sum()
        worst = max(worst, W.units(got, s_ref, tw[seg].sum() + LD(17 * W.U) * s_ref))
    return worst


def _check_cdf(w, cdf, ref, tw):
    """The cumulative sums the step's exact scan makes of the weights (the tile sums are only hints to it: `_check_tiles` judges
    those): numpy's sequential cumsum of the device's weights divided by its last element, bit for bit, and within the derived
    tolerance of the long-double prefix sums
    P_k of the restated weights: the weights' own tolerances up to k, k additions of at most u P_k each, and for the division
    by the total the same two shares over all n rows, plus its rounding.  Returns the worst error in units of it."""
    c = np.cumsum(w)
    assert np.array_equal(cdf, c / c[-1]), np.flatnonzero(cdf != c / c[-1])[:5]
    n = len(w)
    P, T = np.cumsum(ref), np.cumsum(tw)
    tol = T + LD(W.U) * np.arange(1, n + 1) * P + P * (T[-1] / P[-1] + LD((n + 1) * W.U))
    return W.units(cdf, P / P[-1], tol)


def _check_is_step(eng, cu, case, reg):
    kind, n, seed, b0, target, tol = case
    ll, lp, lq = W.population(kind, n, seed)
    d = dev(eng, ll, lp, lq)
    res, w, cdf, tiles = _is_step(eng, d, b0, target, tol, reg)
    b, eff1, conv, rounds, n_nan, trip, trip_one, m2, s1p, found = res
    # the first round reduces every block against its own maximum: blocks are `chunk` particles
    chunk = W.ISW_CHUNK if reg else (((n + cu - 1) // cu + W.ISW_CHUNK - 1) // W.ISW_CHUNK) * W.ISW_CHUNK
    lw1 = W.log_weights(ll, lp, lq, b0, 1.0)
    mb = np.array([W.max_and_nan(lw1[k:k + chunk])[0] for k in range(0, n, chunk)])
    worst = check_search(res[:7], ll, lp, lq, case, cu, block_m=np.repeat(mb, chunk)[:n], label="k_is_weights")
    assert worst is not None, case
    want_found = trip is not None and n_nan == 0 and b > b0
    assert found == want_found, (case, res)
    if not found:
        assert np.all(w == 1.0 / n) and m2 == 0.0 and s1p == 0.0, case  # exact uniform weights
        uni, tuni = np.full(n, LD(1) / LD(n)), np.full(n, LD(W.U) / LD(n))  # (1 / N rounded once)
        return max(worst, _check_cdf(w, cdf, uni, tuni), _check_tiles(tiles, n, uni, tuni))
    L = W.chain_len(n, cu)
    m, S1 = trip[0], trip[1]
    lw = W.log_weights(ll, lp, lq, b0, b)
    mean_u = S1 / n
    shift = float((np.float64(m) + np.log(np.float64(S1))) - np.float64(math.log(n)))
    mp = m + shift
    Lb = W.bis_chain_len(n, cu) + (chunk // 512)
    rm2, rs1p, tm2, ts1p = W.m2_lse(lw, m, mean_u, shift, mp, Lb, free_shift=True)
    worst = max(worst, W.units(m2, rm2, tm2), W.units(s1p, rs1p, ts1p))
    ref, tw = W.normalized_weights(ll, lp, lq, b0, b, Lb)
    assert W.same_nonfinite(w, ref.astype(np.float64)) and np.all(w[lw == -np.inf] == 0.0)
    worst = max(worst, W.units(w, ref, tw))
    # and elementwise against k_weights_map<1> at the step's own scalars, under the tolerance that covers both
    w2 = eng.normalized_weights(*d, b0, b, shift, mp + math.log(s1p)).cpu().numpy()
    worst = max(worst, W.units(w, w2, 2 * tw))
    return max(worst, _check_cdf(w, cdf, ref, tw), _check_tiles(tiles, n, ref, tw))


def _is_cases(n_list, kinds):
    return [(kinds[i % len(kinds)], n, 40 + i, (0.0, 0.2)[i % 2], 0.5, 1e-6) for i, n in enumerate(n_list)]


def test_importance_step_resident(eng, cu):
    kinds = ("synth", "heavy", "sorted_up", "neginf_chunk", "dominant", "peaked3e3", "neginf_lanes", "sorted_down")
    worst = 0.0
    for case in _is_cases((1, 4095, 4096, 4097, 8193, 8193, 12289, 12289), kinds):
        assert W.decided(case)[1], case
        worst = max(worst, _check_is_step(eng, cu, case, True))
    report("k_is_weights<true>", worst)


def test_importance_step_found_zero_gives_exact_uniform_weights(eng, cu):
    n = 8193
    for case in (("plateau_below", n, 1, 0.0, 0.5, 1e-6), ("synth", n, 1, 0.4, 0.999, 2.0), ("neginf_all", n, 1, 0.0, 0.5, 1e-6)):
        _check_is_step(eng, cu, case, True)
    ll, lp, lq = W.population("synth", n, 2)
    lp[n - 1] = np.nan
    res, w, cdf, tiles = _is_step(eng, dev(eng, ll, lp, lq), 0.0, 0.5, 1e-6, True)
    assert res[4] == 1 and not res[9] and np.all(w == 1.0 / n)
    uni, tuni = np.full(n, LD(1) / LD(n)), np.full(n, LD(W.U) / LD(n))
    assert _check_cdf(w, cdf, uni, tuni) < 1 and _check_tiles(tiles, n, uni, tuni) < 1


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_importance_step_resident_streaming_switch(big, cu, delta):
    """One chunk per compute unit exactly and one particle either side: k_is_weights<true> up to 4096 CU, <false> above - where
    the blocks take 8192 particles and the last one holds a single particle (the smallest streaming n with a partly empty
    last block)."""
    n = 4096 * cu + delta
    case = (("sorted_up", "heavy", "neginf_chunk")[delta + 1], n, 50, 0.0, 0.5, 1e-3)
    assert W.decided(case)[1], case
    report(f"k_is_weights<{delta <= 0}> n={n}", _check_is_step(big, cu, case, delta <= 0))


# ---- the sharded forms, emulated ranks on one device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranks(eng):
    from aspire_amd.engine import HipEngine

    extra = [HipEngine(0, n_max=1 << 15, d_max=1) for _ in range(7)]
    yield [eng] + extra
    for e in extra:
        e.close()


def _cuts(n, world, layout):
    if world == 1:
        return [0, n]
    if layout == "one":  # a rank of length 1 in front, the rest unequal
        inner = [1] + [1 + (n - 1) * (r * r + r) // (world * world + world - 2) for r in range(1, world - 1)]
        return [0] + inner + [n]
    return [0] + [n * (r * r + 3 * r) // (world * world + 3 * world) for r in range(1, world)] + [n]


def _shard_population(kind, n, cuts):
    ll, lp, lq = W.population("synth" if kind in ("dead_rank", "margin400") else kind, n, 60)  # (neginf_all, one rank: no finite row at all)
    if kind == "dead_rank" and len(cuts) > 2:  # every row of rank 1 has zero likelihood
        ll[cuts[1]:cuts[2]] = -np.inf
    if kind == "margin400":  # the last rank owns the global maximum by a margin of 400
        ll[cuts[-2] + (cuts[-1] - cuts[-2]) // 2] += 400.0
    return ll, lp, lq


def _shard_search(ranks, world, parts, n, b0, target, tol, folded):
    import torch

    engines = ranks[:world]
    recs = [e.empty(40) for e in engines]
    rounds = max(1, math.ceil(math.log2((1.0 - b0) / tol) / 4 - 1e-9)) + 2
    allrec = None
    for rnd in range(rounds):
        for e, p, rec in zip(engines, parts, recs):
            if folded:
                ran(e, lambda: e.find_beta_shard_round(*p, b0, target, tol, world, n, rnd, allrec, rec),
                    {("k_bis_sums",): 1, **({("k_weights_max", "Li1"): 1} if rnd == 0 else {})})
            else:
                ran(e, lambda: e.find_beta_shard_reduce(*p, b0, rnd, rec), {("k_bis_sums",): 1, **({("k_weights_max", "Li1"): 1} if rnd == 0 else {})})
        allrec = torch.cat(recs).contiguous()
        if not folded:
            for e in engines:
                ran(e, lambda: e.find_beta_shard_decide(allrec, world, n, b0, target, tol, rnd), {("k_bis_decide",): 1})
    outs = [e.empty(2) for e in engines]
    for e, p, o in zip(engines, parts, outs):
        if folded:
            ran(e, lambda: e.weights_m2_lse_shard(*p, o, allrec, world, n, b0, target, tol, rounds), {("k_weights_m2_lse_shard",): 1})
        else:
            ran(e, lambda: e.weights_m2_lse_shard(*p, o), {("k_weights_m2_lse_shard",): 1})
    pairs = torch.cat(outs).contiguous()
    res = []
    for r, (e, p) in enumerate(zip(engines, parts)):
        state = e.empty(40 + 4 * world)
        state[40:40 + 2 * world] = pairs
        state[40 + 2 * world:] = 0.0
        w, carry, tiles = ran(e, lambda: e.normalized_weights_shard(*p, pairs, world, r, r / world, state), {("k_weights_map_shard",): 1})
        res.append((e.shard_step_result(state, world)[0], w.cpu().numpy(), float(carry.cpu()[0]), tiles.cpu().numpy()))
    return res, pairs.cpu().numpy().reshape(world, 2)


@pytest.mark.parametrize("folded", [False, True], ids=["decide", "folded"])
@pytest.mark.parametrize("world,layout,kind", [(1, "uneq", "synth"), (2, "uneq", "heavy"), (3, "one", "neginf20"), (8, "uneq", "sorted_up"),
                                               (3, "uneq", "dead_rank"), (8, "one", "dead_rank"), (2, "uneq", "margin400"),
                                               (8, "uneq", "margin400"), (3, "uneq", "plateau_below"), (1, "uneq", "neginf_all")])
def test_sharded_search_moments_and_weights(ranks, cu, world, layout, kind, folded):
    n, b0, target, tol = 9001, 0.013, 0.5, 1e-6
    cuts = _cuts(n, world, layout)
    assert all(b > a for a, b in zip(cuts[:-1], cuts[1:])) and (layout != "one" or cuts[1] == 1)
    ll, lp, lq = _shard_population(kind, n, cuts)
    case = (f"shard:{kind}:{world}:{layout}", n, 60, b0, target, tol)
    assert W.decide_cached(case, ll, lp, lq, b0, target, tol)[1], case
    parts = [dev(ranks[r], ll[cuts[r]:cuts[r + 1]], lp[cuts[r]:cuts[r + 1]], lq[cuts[r]:cuts[r + 1]]) for r in range(world)]
    res, pairs = _shard_search(ranks, world, parts, n, b0, target, tol, folded)
    lw1 = W.log_weights(ll, lp, lq, b0, 1.0)
    rank_m = np.concatenate([np.full(cuts[r + 1] - cuts[r], W.max_and_nan(lw1[cuts[r]:cuts[r + 1]])[0]) for r in range(world)])
    for r in range(1, world):
        assert res[r][0] == res[0][0], (r, res[r][0], res[0][0])  # the same bits on every rank
    out = res[0][0]
    worst = check_search(out, ll, lp, lq, case, cu, block_m=rank_m, label="sharded")
    b, trip, n_nan = out[0], out[5], out[4]
    found = trip is not None and n_nan == 0 and b > b0
    w = np.concatenate([x[1] for x in res])
    if not found:
        assert np.all(w == 1.0 / n) and all(x[2] == r / world for r, x in enumerate(res)), case
        report(f"sharded {kind} world={world} (found = 0)", worst)
        return
    m, S1 = trip[0], trip[1]
    lw = W.log_weights(ll, lp, lq, b0, b)
    shift = float((np.float64(m) + np.log(np.float64(S1))) - np.float64(math.log(n)))
    mp = m + shift
    for r in range(world):
        sl = slice(cuts[r], cuts[r + 1])
        L = W.chain_len(cuts[r + 1] - cuts[r], cu)
        rm2, rs1p, tm2, ts1p = W.m2_lse(lw[sl], m, S1 / n, shift, mp, L, free_shift=True)
        worst = max(worst, W.units(pairs[r, 0], rm2, tm2), W.units(pairs[r, 1], rs1p, ts1p))
    ref, tw = W.normalized_weights(ll, lp, lq, b0, b, W.chain_len(n, cu) + world)
    assert W.same_nonfinite(w, ref.astype(np.float64))
    worst = max(worst, W.units(w, ref, tw))
    # the carry: the lower ranks' share of S1', the ranks' sums added in rank order (exact restatement of those few operations)
    s1p, below = pairs[0, 1], [0.0]
    for r in range(1, world):
        below.append(s1p)
        s1p = s1p + pairs[r, 1]
    for r in range(world):
        assert res[r][2] == below[r] / s1p, (r, res[r][2], below[r] / s1p)
        wr, twr = ref[cuts[r]:cuts[r + 1]], tw[cuts[r]:cuts[r + 1]]
        # a tile's sum: 8 adds per thread, 6 butterfly steps, 3 over the four waves = a chain of 17
        for t, got in enumerate(res[r][3][: (len(wr) + W.SCAN_TILE - 1) // W.SCAN_TILE]):
            seg = slice(t * W.SCAN_TILE, (t + 1) * W.SCAN_TILE)
            worst = max(worst, W.units(got, wr[seg].sum(), twr[seg].sum() + LD(17 * W.U) * wr[seg].sum()))
    report(f"sharded {kind} world={world} {layout} {'folded' if folded else 'decide'}", worst)


# ---- every kernel of the file ran -----------------------------------------------------------------------------------------------------------
def test_every_kernel_symbol_ran():
    """Closes the module: every __global__ kernel defined in csrc/asmc_weights.hip, asmc_search.hip and asmc_is_weights.hip, in every
    instantiation the library launches, appears in an asserted launch above.  It needs the whole module to have run: under a -k
    selection it fails."""
    src = "".join(open(os.path.join(ROOT, "aspire_amd", "csrc", f)).read() for f in ("asmc_weights.hip", "asmc_search.hip", "asmc_is_weights.hip"))
    kernels = set(re.findall(r"__global__\s+__launch_bounds__\([A-Z_0-9a-z]+\)\s+void\s+(k_[a-z0-9_]+)\s*\(", src))
    assert len(kernels) == 12, sorted(kernels)
    templated = {"k_weights_max": [f"Li{k}" for k in (1, 2, 4, 8, 16, 32)], "k_weights_sums": [f"Li{k}" for k in (1, 2, 4, 8, 16, 32)],
                 "k_weights_map": ["Li0", "Li1"], "k_is_weights": ["Lb1", "Lb0"]}
    assert set(templated) <= kernels
    required = {(k, t) for k in kernels for t in templated.get(k, [None])}
    assert not required - RAN, sorted(required - RAN, key=str)
