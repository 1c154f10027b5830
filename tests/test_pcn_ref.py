"""tests/pcn_ref.py - the plain restatement the pCN / tpCN kernels are compared with (tests/test_gpu_pcn.py) - pinned to the C oracle,
shown to catch planted mistakes through the very comparison the device tests use, and the condition of the razor band: for every
case of the shared table the restatement alone leaves at most razor_cap(n) rows undecided.  CPU only."""
import numpy as np
import pytest

import pcn_ref as P


def _om(oracle, mixes):
    return [oracle.Mixture(*m) for m in mixes]


@pytest.mark.parametrize("shape", [1.0, 1.5, 3.25, 18.75, 72.75])
def test_gamma_unit_is_the_oracles(oracle, shape):
    for gid0, step in ((0, 0), (2**32 - 3, 7), (2**40, 2**32 - 1)):
        got = P.gamma_unit(shape, 99, gid0, 300, step)
        ref = np.array([oracle.gamma_unit(shape, 99, gid0 + i, step) for i in range(300)])
        np.testing.assert_allclose(got, ref, rtol=1e-14)  # (numpy's and libm's log / cos: an ulp or two)
        assert abs(got.mean() / shape - 1) < 5 / np.sqrt(300 * shape) + 0.02


def test_correction_and_adaptation_are_the_oracles(oracle):
    q = np.array([0.0, 1e-9, 0.3, 7.0, 150.0, 1e6])
    for d, nu in ((1, 1.0), (33, 5.5), (140, 1e6)):
        np.testing.assert_allclose(P.ref_corr(q, nu, d), oracle.tpcn_corr(q, d, nu), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(P.ref_corr(q, 0.0, 7), 0.5 * q)
    for rho, c, t in ((0.4, 30, 0), (0.4, 290, 3), (1e-4, 0, 5), (0.99, 300, 0), (0.5, 70, 2047)):
        assert P.adapt_rho(rho, c, 300, 0.234, t) == pytest.approx(oracle.pcn_adapt(rho, c / 300, 0.234, t), rel=1e-15)
    assert P.adapt_rho(1e-4, 0, 300, 0.234, 0) == 1e-4 and P.adapt_rho(0.99, 300, 300, 0.234, 0) == 0.99


@pytest.mark.parametrize("adapt,n_steps", [(0, 5), (1, 5), (2, 6), (2, 5), (3, 7), (3, 2)])
def test_lagged_adaptation_replays_the_per_step_updates_late(adapt, n_steps):
    """adapt = k >= 2 holds the step size for k steps and then applies the block's updates in order, each with its own count and
    step index; a call that ends inside a block closes it at its last step."""
    counts = [40, 90, 10, 120, 70, 30, 100][:n_steps]
    hist, out = P.adapt_schedule(0.4, counts, 300, 0.234, adapt)
    r, expect = 0.4, []
    for t in range(n_steps):
        k = max(adapt, 1)
        expect.append(r if adapt == 0 or t % k == 0 else expect[-1])
        if adapt and ((t + 1) % k == 0 or t == n_steps - 1):
            for tp in range(t - t % k, t + 1):
                r = P.adapt_rho(r, counts[tp], 300, 0.234, tp)
    np.testing.assert_array_equal(hist, expect)
    assert out == r


@pytest.mark.parametrize("kind", ["pcn", "tpcn"])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 3, 4, 16, 33, 140])
def test_step_is_the_oracles(oracle, d, C, kind):
    """One step against oracle.pcn_step / tpcn_step on a decided row: positions to 1e-12 relative, margins to 1e-10, decisions
    equal off the razor band (|margin| <= 1e-10)."""
    n, nu = 200, 4.5 if kind == "tpcn" else 0.0
    x, ll, lp, lq, mu, L, Linv, mixes = P.problem(n, d, 50 + d + C, C)
    om = _om(oracle, mixes)
    np.testing.assert_allclose(ll, om[0].logpdf(x), rtol=1e-13)
    beta, rho, seed, gid0, step = 0.37, 0.4, 77, 2**32 - 100, 9
    (xn, lln, lpn, lqn), p = P.step(x, ll, lp, lq, beta, mu, L, Linv, rho, mixes, seed, gid0, step, nu)
    xr, llr, lpr, lqr = x.copy(), ll.copy(), lp.copy(), lq.copy()
    with oracle.accept_margins(n) as m:
        if nu > 0:
            acc = oracle.tpcn_step(xr, llr, lpr, lqr, beta, mu, L, Linv, rho, nu, om[0], om[1], om[2], seed, gid0, step)
        else:
            acc = oracle.pcn_step(xr, llr, lpr, lqr, beta, mu, L, Linv, rho, om[0], om[1], om[2], seed, gid0, step)
        margins = m.copy()
    np.testing.assert_allclose(p["margin"], margins, rtol=0, atol=1e-10)
    ok = np.abs(margins) > 1e-10
    assert np.array_equal(p["accept"][ok], margins[ok] > 0) and abs(int(p["accept"].sum()) - acc) <= (~ok).sum()
    assert 0 < acc < n
    np.testing.assert_allclose(xn[ok], xr[ok], rtol=1e-12, atol=1e-12)
    for a, b in ((lln, llr), (lpn, lpr), (lqn, lqr)):
        np.testing.assert_allclose(a[ok], b[ok], rtol=1e-12, atol=1e-12)


def test_f32_noise_step_is_the_oracles(oracle):
    x, ll, lp, lq, mu, L, Linv, mixes = P.problem(150, 9, 3, 2)
    om = _om(oracle, mixes)
    (xn, *_), p = P.step(x, ll, lp, lq, 0.5, mu, L, Linv, 0.3, mixes, 5, 11, 2, 3.0, mode="f32")
    xr, c = x.copy(), [ll.copy(), lp.copy(), lq.copy()]
    with oracle.accept_margins(150) as m:
        oracle.tpcn_step(xr, *c, 0.5, mu, L, Linv, 0.3, 3.0, om[0], om[1], om[2], 5, 11, 2, noise="f32")
        margins = m.copy()
    np.testing.assert_allclose(p["margin"], margins, rtol=0, atol=1e-10)
    ok = np.abs(margins) > 1e-10
    np.testing.assert_allclose(xn[ok], xr[ok], rtol=1e-12, atol=1e-12)


def test_whitened_state_loop_equals_the_x_state_loop_in_exact_storage():
    """With nothing rounded to a storage type the two loops of `mutate` are the same chain (the whitened one re-evaluates the
    densities at the end: equal to rounding)."""
    x, ll, lp, lq, mu, L, Linv, mixes = P.problem(120, 8, 4, 2)
    a = P.mutate(x, ll, lp, lq, 0.4, mu, L, Linv, 0.35, mixes, 3, 0, 4, 2, 5.0, ft=np.longdouble, store=None, state="x")
    b = P.mutate(x, ll, lp, lq, 0.4, mu, L, Linv, 0.35, mixes, 3, 0, 4, 2, 5.0, ft=np.longdouble, store=None, state="y")
    assert np.array_equal(a["counts"], b["counts"])
    np.testing.assert_allclose(a["x"].astype(float), b["x"].astype(float), rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(a["ll"].astype(float), b["ll"].astype(float), rtol=1e-14, atol=1e-14)


# ---- planted mistakes: each must fail the comparison of the device tests on a case of their table -------------------------------
def _planted_case(bug):
    want = dict(corr_sign=lambda c: c["nu"] > 0, q1_padded=lambda c: P.pad_dim(c["d"]) > c["d"],
                a_no_root=lambda c: True, shape_padded=lambda c: P.pad_dim(c["d"]) > c["d"] + 1 and c["nu"] > 0,
                u_tile_local=lambda c: c["n"] > 64, ragged_last_lane=lambda c: c["n"] % 64 != 0, no_guard=lambda c: True)[bug]
    return [c for c in P.CASES if c["state"] == "x" and c["n_steps"] == 1 and c["mode"] == "f64" and want(c)]


@pytest.mark.parametrize("bug", P.BUGS)
def test_planted_mistake_fails_the_device_comparison(bug):
    cases = _planted_case(bug)
    assert cases
    caught = 0
    for c in cases[:6]:
        (x, ll, lp, lq, mu, L, Linv, mixes), ref, (tx, tc, tm) = P.case_reference(c)
        beta = c["beta"]
        if bug == "no_guard":  # the guard shows where a product 0 * -inf arises: beta = 0 with a carried -inf likelihood
            beta, ll = 0.0, np.where(np.arange(c["n"]) % 3 == 0, -np.inf, ll)
            ref = P.mutate(x, ll, lp, lq, beta, mu, L, Linv, c["rho"], mixes, 4242 + c["seed"], 1000, 1, 5, c["nu"],
                           store=P.STORE[c["store"]])
        args = (x, ll, lp, lq, beta, mu, L, Linv, c["rho"], mixes, 4242 + c["seed"], 1000, 5, c["nu"])
        good, pg = P.step(*args, store=P.STORE[c["store"]])
        P.compare(dict(zip(("x", "ll", "lp", "lq"), good)), ref, ref["margins"], tx, tc, tm)  # the unspoilt output passes
        bad, pb = P.step(*args, store=P.STORE[c["store"]], bug=bug)
        try:
            P.compare(dict(zip(("x", "ll", "lp", "lq"), bad)), ref, ref["margins"], tx, tc, tm)
        except AssertionError:
            caught += 1
        else:
            # a fused step shows its decisions and accepted proposals only: a mistake may pass where it changes neither (the
            # last row rejected either way; a few padded coordinates that move no margin across zero), and nowhere else
            assert np.array_equal(good[0], bad[0]) and bug in ("ragged_last_lane", "q1_padded", "shape_padded"), (bug, P.case_id(c))
    assert caught > 0, bug


# ---- the condition of the razor band ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_reference_alone_stays_within_the_razor_cap(c):
    _, ref, (tx, tc, tm) = P.case_reference(c)
    und = P.razor(ref["margins"], tm)
    assert und.sum() <= P.razor_cap(c["n"]), (int(und.sum()), tm)
    # the tolerances stay far below what any of the planted mistakes moves (O(rho)), and the chain moves
    assert tx < 1e-4 and tm < 5e-3
    if c["n"] >= 63:
        assert 0.02 < ref["counts"].mean() / c["n"] < 0.98


def test_case_table_reaches_every_structure():
    ids = [P.case_id(c) for c in P.CASES]
    assert len(set(ids)) == len(ids)
    ns = {c["n"] for c in P.CASES if c["d"] == 8 and not c["offset"]}
    assert {1, 63, 64, 65, 255, 256, 257, 3001} <= ns
    assert {1, 15, 16, 17, 127, 128, 129, 1999} <= {c["n"] for c in P.CASES if c["d"] == 64}
    assert sum(c["n"] > 10**5 for c in P.CASES) == 0  # (the grid-stride case builds its own inputs on the device side)
