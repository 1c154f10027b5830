"""The restatement of tests/weights_ref.py and its tolerance formulas, without a GPU: it reproduces the reference's goldens and agrees
with the C oracle; numpy's own fp64 evaluation of every quantity - in the kernels' summation order and in a shuffled one, the
sixteen-term progression and the block-maximum rescale included - stays inside the formulas (a correct fp64 kernel can meet them);
seven plausible mistakes land far outside (the distance of each is asserted and printed); and the decidability cap of the search
cases holds for the restatement alone."""
import math

import numpy as np
import pytest

import weights_ref as W
from conftest import synth

LD = W.LD
NUM_CU = 256  # the dispatch geometry the CPU checks assume (the GPU module reads the device's)


def _golden_batch(n, d, seed):
    return synth(n, d, 0, 2.0) if seed == 0 else synth(n, d, seed)


# ---- goldens and the C oracle ----------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_weight_goldens(golden):
    g = golden["ref_weights"]
    for n, d, seed, b0, b in g["cases"]:
        n, d, seed = int(n), int(d), int(seed)
        _, ll, lp, lq = synth(n, d, seed)
        key = f"n{n}_b{b0}_t{b}"
        lw = W.log_weights(ll, lp, lq, b0, b)
        m, n_nan = W.max_and_nan(lw)
        L = W.chain_len(n, NUM_CU)
        S1, S2, t1, t2 = W.sums(lw, m, 0.0, L)
        ratio = W.evidence_ratio(m, S1, n)
        # the reference's own fp64 value: a pairwise sum of n terms (log2 n + 2 roundings), a log, two additions
        ref_tol = (math.log2(n) + 2) * W.U + 4 * W.U * (abs(m) + abs(float(ratio)) + math.log(n))
        assert n_nan == 0
        assert abs(float(g[key + "_lse_unnorm"]) - float(ratio + np.log(LD(n)))) <= ref_tol + float(t1 / S1)
        assert abs(float(g[key + "_ratio"]) - float(ratio)) <= ref_tol + float(t1 / S1)
        lwn = lw + float(ratio)
        want = g[key + "_lw"] if n <= 2000 else g[key + "_lw_stride"]
        got = lwn if n <= 2000 else lwn[::257]
        assert np.all(np.abs(got - want) <= 2 * W.ulp64(want) + ref_tol)
        # ESS = exp(2 lse(x) - lse(2 x)): the exponent carries the roundings of its two log-sum-exps
        ess = float(W.ess_ld(S1, S2))
        l1, l2 = abs(float(ratio)) + abs(m) + math.log(n), 2 * (abs(float(ratio)) + abs(m)) + math.log(n)
        assert abs(float(g[key + "_ess"]) - ess) <= ess * (8 * W.U * (2 * l1 + l2 + 2) + 2 * (math.log2(n) + 2) * W.U) + float(W.ess_tol(S1, S2, t1, t2))
        m2, _, tm2, _ = W.m2_lse(lw, m, float(S1 / LD(n)), 0.0, m, L)
        var = float(W.evidence_variance(m2, S1, n))
        assert abs(float(g[key + "_var"]) - var) <= var * (float(tm2 / m2) + 2 * float(t1 / S1) + (math.log2(n) + 8) * 4 * W.U)


def test_restated_search_reproduces_the_beta_goldens(golden):
    from aspire_amd import smc_math

    g = golden["ref_beta"]
    for n, d, seed, b0, tol, ti, b_ref in g["cases"]:
        n, d, seed, ti = int(n), int(d), int(seed), int(ti)
        _, ll, lp, lq = _golden_batch(n, d, seed)
        target = smc_math.current_target_efficiency([0.5, (0.3, 0.9)][ti], 1.0, b0)
        b, margin, nodes = W.search(ll, lp, lq, b0, target, tol)
        assert b == b_ref, (n, b0, tol, ti, b, b_ref)
        assert nodes >= 2


@pytest.mark.parametrize("kind", W.SEARCH_POPULATIONS)
def test_oracle_agrees_with_the_restatement(oracle, kind):
    ll, lp, lq = W.population(kind, 1025, 1)
    for b0, b in ((0.0, 0.25), (0.4, 1.0), (0.93, 0.930001)):
        lw = W.log_weights(ll, lp, lq, b0, b)
        got = oracle.unnormalized_log_weights(ll, lp, lq, b0, b)
        assert W.same_nonfinite(got, lw) and np.array_equal(got[np.isfinite(lw)], lw[np.isfinite(lw)])
        m, n_nan = W.max_and_nan(lw)
        if m == -math.inf or n_nan:
            continue
        S1, S2, t1, t2 = W.sums(lw, m, 0.0, 64)
        ess = float(W.ess_ld(S1, S2))
        l1 = abs(m) + math.log(1025) + abs(float(W.evidence_ratio(m, S1, 1025)))
        assert abs(oracle.ess_at_beta(ll, lp, lq, b0, b) - ess) <= ess * (32 * W.U * (3 * l1 + 2) + 1025 * W.U) + float(W.ess_tol(S1, S2, t1, t2))
    case = (kind, 1025, 1, 0.0, 0.5, 1e-6)
    b_star, ok, _ = W.decided(case)
    assert ok, case
    r = oracle.determine_beta(ll, lp, lq, 0.0, beta_tolerance=1e-6, target_efficiency=0.5)
    assert r.beta_star == b_star or (r.stalled and b_star <= 1e-6)


# ---- numpy fp64 meets every tolerance ---------------------------------------------------------------------------------------------------
def _kernel_order_sum(e, n, grid):
    """Sum of e in the direct kernels' order: per-lane strided chains, then lanes, waves, blocks (numpy adds row by row)."""
    stride = grid * W.BLOCK
    pad = np.zeros(((n + stride - 1) // stride) * stride)
    pad[:n] = e
    lanes = np.zeros(stride)
    for row in pad.reshape(-1, stride):
        lanes = lanes + row
    return lanes.reshape(grid, 4, 64).sum(2).sum(1).sum()


FINITE_KINDS = [k for k in W.POPULATIONS]


@pytest.mark.parametrize("n", [1, 65, 2049, 30011])
@pytest.mark.parametrize("kind", FINITE_KINDS)
def test_numpy_direct_reductions_meet_the_tolerances(kind, n):
    ll, lp, lq = W.population(kind, n, 7)
    worst = 0.0
    for b0, b in ((0.0, 0.07), (0.3, 1.0)):
        lw = W.log_weights(ll, lp, lq, b0, b)
        m, n_nan = W.max_and_nan(lw)
        assert n_nan == 0
        if m == -math.inf:
            continue
        L = W.chain_len(n, NUM_CU)
        grid = W.reduce_grid(n, NUM_CU)
        S1, S2, t1, t2 = W.sums(lw, m, 0.0, L)
        with np.errstate(all="ignore"):
            e = np.exp(lw - m)
        perm = np.random.default_rng(n).permutation(n)
        for s1, s2 in ((_kernel_order_sum(e, n, grid), _kernel_order_sum(e * e, n, grid)), (e[perm].sum(), (e * e)[perm].sum())):
            worst = max(worst, W.units(s1, S1, t1), W.units(s2, S2, t2))
        mean_u = float(S1 / LD(n))
        shift = float((m + np.log(float(S1))) - math.log(n))
        mp = m + shift
        m2, S1p, tm2, t1p = W.m2_lse(lw, m, mean_u, shift, mp, L)
        with np.errstate(all="ignore"):
            d = e - mean_u
            e2 = np.exp((lw + shift) - mp)
        worst = max(worst, W.units((d * d).sum(), m2, tm2), W.units(e2.sum(), S1p, t1p))
        w, tw = W.normalized_weights(ll, lp, lq, b0, b, L)
        with np.errstate(all="ignore"):
            got = np.exp((lw + shift) - (mp + math.log(e2.sum())))
        worst = max(worst, W.units(got, w, tw))
    print(f"numpy direct {kind} n={n}: worst error {worst:.3g} of the tolerance")
    assert worst < 1


@pytest.mark.parametrize("b0", [0.0, 0.4, 1.0 - 2.0 ** -20])
@pytest.mark.parametrize("kind", FINITE_KINDS)
def test_numpy_progression_meets_the_tolerances(kind, b0):
    n = 2049
    ll, lp, lq = W.population(kind, n, 8)
    m_one, _ = W.max_and_nan(W.log_weights(ll, lp, lq, b0, 1.0))
    assert math.isfinite(m_one)
    L = W.bis_chain_len(n, NUM_CU)
    worst = 0.0
    for order in (None, np.random.default_rng(3).permutation(n)):
        S1, S2 = W.emulate_round(ll, lp, lq, *W.first_round_grid(b0, m_one), order=order)
        for j in range(16):
            beta = W.bis_node_beta(j + 1, 4, b0)
            m = W.node_shift(m_one, beta, b0)
            R1, R2, t1, t2 = W.progression_sums(ll, lp, lq, b0, beta, m, L)
            worst = max(worst, W.units(S1[j], R1, t1), W.units(S2[j], R2, t2))
    print(f"numpy progression {kind} beta0={b0}: worst error {worst:.3g} of the tolerance")
    assert worst < 1


def test_numpy_progression_on_deep_grids_meets_the_tolerances():
    """Later rounds: sixteen nodes around beta* at the search's last level, one cell and 2^(LU - 8) cells apart, on every
    small search case - the floats of deep nodes against the progression's exact steps."""
    worst, rounds = 0.0, 0
    for case in [c for c in W.named_search_cases() if c[1] < 100000] + W.random_search_cases()[::2]:
        kind, n, seed, b0, target, tol = case
        ll, lp, lq = W.population(kind, n, seed)
        m_one, _ = W.max_and_nan(W.log_weights(ll, lp, lq, b0, 1.0))
        if not math.isfinite(m_one) or not (1.0 - b0 > tol):
            continue
        LU = W.search_levels(b0, tol) - 1
        Ks = int(round((W.decided(case)[0] - b0) / (1.0 - b0) * 2 ** LU))
        for stride in (1, max(1, 2 ** (LU - 8))):
            Kf = min(max(1, Ks - 7 * stride), 2 ** LU - 15 * stride)
            if Kf < 1:
                continue
            S1, S2 = W.emulate_round(ll, lp, lq, *W.later_round_grid(b0, m_one, Kf, stride, LU))
            rounds += 1
            for j in range(16):
                beta = W.bis_node_beta(Kf + j * stride, LU, b0)
                R1, R2, t1, t2 = W.progression_sums(ll, lp, lq, b0, beta, W.node_shift(m_one, beta, b0), W.bis_chain_len(n, NUM_CU), tol_beta=tol)
                worst = max(worst, W.units(S1[j], R1, t1), W.units(S2[j], R2, t2))
    print(f"numpy progression, {rounds} deep rounds: worst error {worst:.3g} of the tolerance")
    assert worst < 1 and rounds > 100


@pytest.mark.parametrize("kind", ["synth", "sorted_up", "sorted_down", "neginf_chunk", "dominant", "peaked3e4", "offset1e6"])
def test_numpy_block_rescale_meets_the_tolerances(kind):
    n, b0 = 3 * 4096 + 5, 0.013
    ll, lp, lq = W.population(kind, n, 9)
    S1, S2, M, mb = W.emulate_round0_blocks(ll, lp, lq, b0)
    assert M == W.max_and_nan(W.log_weights(ll, lp, lq, b0, 1.0))[0]
    block_m = np.repeat(mb, W.ISW_CHUNK)[:n]
    worst = 0.0
    for j in range(16):
        beta = W.bis_node_beta(j + 1, 4, b0)
        m = W.node_shift(M, beta, b0)
        R1, R2, t1, t2 = W.progression_sums(ll, lp, lq, b0, beta, m, W.bis_chain_len(n, NUM_CU), block_m, M)
        worst = max(worst, W.units(S1[j], R1, t1), W.units(S2[j], R2, t2))
    print(f"numpy block rescale {kind}: worst error {worst:.3g} of the tolerance, block maxima span {np.ptp(mb[np.isfinite(mb)]):.3g}")
    assert worst < 1


# ---- the formulas have teeth --------------------------------------------------------------------------------------------------------------
def test_plausible_mistakes_land_outside_the_tolerances():
    n, b0 = 2049, 0.0
    ll, lp, lq = W.population("synth", n, 10)
    m_one, _ = W.max_and_nan(W.log_weights(ll, lp, lq, b0, 1.0))
    L = W.bis_chain_len(n, NUM_CU)
    grid0 = W.first_round_grid(b0, m_one)
    nodes = [W.bis_node_beta(j + 1, 4, b0) for j in range(16)]
    shifts = [W.node_shift(m_one, b, b0) for b in nodes]
    ref = [W.progression_sums(ll, lp, lq, b0, b, m, L) for b, m in zip(nodes, shifts)]
    dist = {}

    def far(S1, S2, refs=ref):
        return max(max(W.units(S1[j], r[0], r[2]), W.units(S2[j], r[1], r[3])) for j, r in enumerate(refs))

    # 1 the last particle dropped
    dist["last particle dropped"] = far(*W.emulate_round(ll[:-1], lp[:-1], lq[:-1], *grid0))
    # 2 the tail of a two-particle trip dropped when i2 >= n: two blocks of 512 threads, stride 1024 - particle 2048 opens a
    #   trip whose partner 3072 does not exist
    stride = 1024
    i = np.arange(n)
    keep = ~(((i // stride) % 2 == 0) & (i + stride >= n))
    assert (~keep).sum() == 1
    dist["trip tail dropped (has2)"] = far(*W.emulate_round(ll[keep], lp[keep], lq[keep], *grid0))
    # 3 S2 accumulated as e instead of e e
    S1, _ = W.emulate_round(ll, lp, lq, *grid0)
    dist["S2 = sum e"] = far(S1, S1)
    # 4 the shift of candidate j used for candidate j + 1 (reported next to m_{j+1}: off by exp(m_{j+1} - m_j))
    S1, S2 = W.emulate_round(ll, lp, lq, *grid0)
    f = np.exp(np.diff(np.array([shifts[0] - (shifts[1] - shifts[0])] + shifts)))
    dist["shift of candidate j - 1"] = far(S1 * f, S2 * f * f)
    # 5 m taken from the previous call's keys (a search at beta0 = 0.3 ran before: its m(1) is 0.7 of this one)
    m_prev, _ = W.max_and_nan(W.log_weights(ll, lp, lq, 0.3, 1.0))
    dist["m of the previous call"] = far(*W.emulate_round(ll, lp, lq, *W.first_round_grid(b0, m_prev)))
    # 6, 7 on the block-wise first round: merged without the rescale; a dead block counted with m_b = 0
    nb = 3 * 4096 + 5
    for kind, label, kw in (("sorted_up", "blocks merged without the rescale", dict(rescale=False)),
                            ("neginf_chunk", "dead block counted with m_b = 0", dict(dead_block_m="0"))):
        bl, bp, bq = W.population(kind, nb, 9)
        bl = bl - 900.0  # every log-weight far below zero: a maximum of 0 is not among them
        M, _ = W.max_and_nan(W.log_weights(bl, bp, bq, 0.013, 1.0))
        good = W.emulate_round0_blocks(bl, bp, bq, 0.013)
        bad = W.emulate_round0_blocks(bl, bp, bq, 0.013, **kw)
        mb = np.repeat(good[3], W.ISW_CHUNK)[:nb]
        refs = [W.progression_sums(bl, bp, bq, 0.013, b, W.node_shift(M, b, 0.013), W.bis_chain_len(nb, NUM_CU), mb, M)
                for b in (W.bis_node_beta(j + 1, 4, 0.013) for j in range(16))]
        assert far(good[0], good[1], refs) < 1
        dist[label] = far(bad[0], bad[1], refs)
        if kind == "neginf_chunk":
            assert bad[2] == 0.0 and good[2] == M < -800  # the reported m(1) is wrong too: compared bit for bit on the device
    for label, v in dist.items():
        print(f"mistake '{label}': {v:.3g} x the tolerance")
        assert v > 100, (label, v)
    assert len(dist) == 7


def test_direct_kernel_mistakes_land_outside_the_tolerances():
    """The same for the direct reductions: a dropped last particle and a skipped second grid-stride pass."""
    n = 2049
    ll, lp, lq = W.population("synth", n, 11)
    lw = W.log_weights(ll, lp, lq, 0.0, 0.3)
    m, _ = W.max_and_nan(lw)
    S1, S2, t1, t2 = W.sums(lw, m, 0.0, W.chain_len(n, NUM_CU))
    e = np.exp(lw - m)
    assert W.units(e[:-1].sum(), S1, t1) > 100
    assert W.units(e[: n // 2].sum(), S1, t1) > 100


# ---- non-finite contract -------------------------------------------------------------------------------------------------------------------
def test_nonfinite_contract_table():
    rows = {c: W.nonfinite_contract(c) for c in W.NONFINITE_CLASSES}
    for c, r in rows.items():
        print(r)
    r = rows["some_neginf"]
    assert r["n_nan"] == 0 and math.isfinite(r["S1"]) and 0 < r["ess"] <= 200 and r["found"] and not r["raises"]
    r = rows["all_neginf"]  # lse(-inf ...) = -inf + log(sum exp(nan)): NaN sums, every ESS comparison false, beta* = beta0
    assert r["m"] == -math.inf and r["n_nan"] == 0 and math.isnan(r["S1"]) and math.isnan(r["ess"]) and r["beta_star"] == 0.0
    assert not r["found"] and r["weights"] == "1/N"
    r = rows["posinf_row"]  # the maximum is +inf: inf - inf in its own row, NaN sums
    assert r["m"] == math.inf and r["n_nan"] == 0 and math.isnan(r["S1"]) and r["beta_star"] == 0.0 and not r["found"]
    for c in ("inf_minus_inf_row", "nan_row"):
        r = rows[c]
        assert r["n_nan"] == 1 and r["raises"] and not r["found"] and math.isnan(r["S1"])


# ---- the decidability cap ------------------------------------------------------------------------------------------------------------------
def test_every_named_search_case_is_decidable():
    bad = [c for c in W.named_search_cases() if c[1] < 100000 and not W.decided(c)[1]]
    assert not bad, bad


def test_the_large_named_search_cases_are_decidable():
    bad = [c for c in W.named_search_cases() if c[1] > 100000 and not W.decided(c)[1]]
    assert not bad, bad


def test_random_sweep_stays_inside_the_decidability_cap():
    cases = W.random_search_cases()
    bad = [c for c in cases if not W.decided(c)[1]]
    print(f"undecidable: {len(bad)} of {len(cases)}: {bad}")
    assert len(cases) == 100 and len(bad) * 50 <= len(cases), bad


def test_reference_decisions_lose_meaning_with_a_large_common_offset():
    """The magnitude of |lq| at which the reference's own fp64 ESS drifts by more than a search can resolve (DESIGN.md section
    3.16 quotes these figures): with a common offset c in ll and lq every log-weight is the difference of two products of
    magnitude t c, each rounded once, so every log-weight moves by up to 2 u t c and ESS/N = S1^2 / S2 by up to four times that
    (each sum once, S1 squared), whatever the order of the sums.  The fp64 and the long-double run of the SAME expression stay
    within that bound (plus the bound of an offset-free population); the roundings are independent, so what one sees is
    far below it (about sqrt(N) times), and above the offset-free bound from 1e9 on."""
    ll, lp, lq = W.population("synth", 2049, 12)
    t = 0.17
    free = None
    for off in (0.0, 1e3, 1e6, 1e9, 1e12):
        a, b = W._eff_f64(ll + off, lp, lq + off, 0.0, t), float(W._eff_ld(ll + off, lp, lq + off, 0.0, t))
        drift = abs(a - b) / b
        if free is None:
            lw = W.log_weights(ll, lp, lq, 0.0, t)
            free = W.U * (4 * np.abs(lw).max() + 4 * math.log(2049) + 2 * math.log2(2049) + 16)  # the roundings without an offset
            assert drift <= free
        bound = 8 * W.U * t * off + free
        print(f"common offset {off:g}: fp64 ESS/N off by {drift:.3g} relative (bound {bound:.3g})")
        assert drift <= bound
        assert off < 1e9 or drift > free  # from 1e9 on the offset's share is what one sees
