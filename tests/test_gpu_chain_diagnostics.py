"""The chain-diagnostics kernels (csrc/asmc_diag.hip) against the direct-summation restatement of
tests/autocorr_ref.py, whose fixtures tests/test_chain_diagnostics.py guards against razor-edge windows.

Tolerances (derived in DESIGN.md §3.23, from the number format and the reference's own sums, never from the kernels' output):
    rho     |device - restatement| <= 8 gamma_n A_j[k],  n = S W,  gamma_n = n u / (1 - n u),  u = 2^-53
    window  equal
    tau     2 (window + 1) times the largest rho bound up to the window
    R-hat   relative 8 gamma_n (1 + kappa), kappa the mass-to-value ratio of the one sum in it that cancels
"""
import numpy as np
import pytest
import torch

import autocorr_ref as R
from autocorr_ref import special_fixtures

pytestmark = pytest.mark.gpu

ACF_KERNELS = {"k_chain_moments", "k_chain_acf_block", "k_chain_acf_finish"}
RHAT_KERNELS = {"k_chain_moments": 1, "k_chain_rhat_part": 2, "k_chain_rhat": 2}  # launches of one chain_rhat


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A HIP fault is sticky: end the session there instead of running on."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device fault: {exc}", returncode=3)


def test_lag_block_of_the_binding():
    from aspire_amd import _lib

    assert _lib.load().asmc_chain_acf_kb() == _lib.ASMC_DIAG_KB == R.KB


def check_autocorr(eng, x, dev=None, label="", kb=None):
    """x: the host chain [S, W, d] (its own dtype); dev: the device tensor to hand over (default: a copy of x)."""
    S, W, d = x.shape
    dev = torch.as_tensor(x, device=eng.device) if dev is None else dev
    ref = R.autocorr_direct(x)
    tau, window, rho = eng.chain_autocorr(dev, return_rho=True, kb=kb)
    assert tau.shape == (d,) and window.shape == (d,) and rho.shape == (d, S)
    assert np.array_equal(window, ref["window"]), (label, window, ref["window"])
    assert np.array_equal(np.isnan(tau), np.isnan(ref["tau"])), (label, tau, ref["tau"])
    worst = 0.0
    for j in range(d):
        if np.isnan(ref["tau"][j]):
            assert np.isnan(rho[j]).all() or np.isnan(rho[j, 0])
            continue
        w = int(window[j])
        bound = R.rho_bound(S, W, ref["mass"][:w + 1, j])
        err = np.abs(rho[j, :w + 1] - ref["rho"][:w + 1, j])
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (label, j, float(np.max(err / bound)))
        assert np.isnan(rho[j, w + 1:]).all()  # nothing is written behind the window
        assert abs(tau[j] - ref["tau"][j]) <= 2 * (w + 1) * float(np.max(bound)), (label, j, tau[j], ref["tau"][j])
    return tau, window, rho, worst


def check_rhat(eng, x, dev=None, label=""):
    S, W, d = x.shape
    dev = torch.as_tensor(x, device=eng.device) if dev is None else dev
    ref, kappa = R.split_rhat_direct(x)
    got = eng.chain_rhat(dev)
    assert got.shape == (d,)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (label, got, ref)
    ok = ~np.isnan(ref)
    tol = 8.0 * R.gamma(S * W) * (1.0 + kappa[ok]) * ref[ok]
    assert np.all(np.abs(got[ok] - ref[ok]) <= tol), (label, np.abs(got[ok] - ref[ok]) / tol)
    return got


@pytest.mark.parametrize("S,W,d", R.GPU_SHAPES, ids=lambda v: str(v))
def test_shapes(eng, S, W, d):
    """Every ragged end: S around the lag block and no multiple of it, lags beyond the chain, one walker, walkers that fill no
    block, d that divides no wave (3, 33); both storage types; coordinates that finish in different lag blocks."""
    for dt in (np.float64, np.float32):
        x = R.fixture(S, W, d, dt)
        label = f"{S}x{W}x{d} {np.dtype(dt).name}"
        tau, window, rho, worst = check_autocorr(eng, x, label=label)
        if S == 1:
            assert np.isnan(tau).all() and np.all(window == 0)
        check_rhat(eng, x, label=label)
    print(f"{S}x{W}x{d}: worst rho error / bound {worst:.3f}; windows {window.min()} .. {window.max()}")


def test_a_chain_too_short_for_its_correlation(eng):
    """phi = 0.99 at 50 steps: tau_{S-1} of the zero-padded estimator is 0, so the window is found at the latest at lag S - 1 = 49
    (tests/test_chain_diagnostics.py::test_the_window_is_always_found_by_the_last_lag) - here before it, and behind the phi = 0.5
    coordinate's."""
    x = special_fixtures()["short-0.99"]
    tau, window, _, _ = check_autocorr(eng, x)
    assert window[1] < window[0] < 49 and window[1] < window[2] < 49


@pytest.mark.parametrize("kb", [16, 32])
@pytest.mark.parametrize("S,W,d", [(131, 257, 33), (67, 7, 3), (33, 1, 8), (15, 257, 32)], ids=lambda v: str(v))
def test_both_lag_blocks(eng, S, W, d, kb):
    """The library carries the lag-block kernel for 16 and 32 lags; ASMC_DIAG_KB is the one the package uses.  Same results, to
    the bound, whichever runs - and the coordinates of the long shapes finish in different blocks of either."""
    for dt in (np.float64, np.float32):
        _, window, _, _ = check_autocorr(eng, R.fixture(S, W, d, dt), label=f"kb={kb}", kb=kb)
    if S == 131:
        assert window.min() < 16 and window.max() >= 32


def test_a_coordinate_that_never_moves(eng):
    sp = special_fixtures()
    x = sp["constant-coordinate"]
    tau, window, _, _ = check_autocorr(eng, x)
    assert np.isnan(tau[2]) and window[2] == x.shape[0] - 1 and np.isfinite(np.delete(tau, 2)).all()
    x = sp["constant-walker"]  # one walker's series alone: its NaN makes the walker mean NaN, as in emcee
    tau, window, _, _ = check_autocorr(eng, x)
    assert np.isnan(tau[1]) and np.isfinite(np.delete(tau, 1)).all()
    check_rhat(eng, x)  # (a zero variance among many leaves R-hat finite)
    assert np.isfinite(eng.chain_rhat(torch.as_tensor(x, device=eng.device))).all()


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_kept_steps_inside_a_larger_allocation(eng, dt):
    """`discard` is pointer arithmetic: guard steps of 1e300 in front of and behind the kept ones change no bit."""
    x = special_fixtures()["guarded"].astype(dt)
    S, W, d = x.shape
    big = torch.full((5 + S + 4, W, d), 1e300 if dt == np.float64 else 3e38, dtype=torch.as_tensor(x).dtype, device=eng.device)
    big[5:5 + S].copy_(torch.as_tensor(x))
    alone = eng.chain_autocorr(torch.as_tensor(x, device=eng.device), return_rho=True)
    inside = eng.chain_autocorr(big[5:5 + S], return_rho=True)
    for a, b in zip(alone, inside):
        assert a.tobytes() == b.tobytes()
    assert eng.chain_rhat(big[5:5 + S]).tobytes() == eng.chain_rhat(torch.as_tensor(x, device=eng.device)).tobytes()
    check_autocorr(eng, x, dev=big[5:5 + S])
    check_rhat(eng, x, dev=big[5:5 + S])


def test_a_rung_of_a_tempered_chain(eng):
    x4 = special_fixtures()["rungs"]
    dev = torch.as_tensor(x4, device=eng.device)
    for r in range(x4.shape[0]):
        check_autocorr(eng, x4[r], dev=dev[r])
        check_rhat(eng, x4[r], dev=dev[r])


def test_two_calls_give_the_same_bits(eng):
    x = torch.as_tensor(R.fixture(131, 257, 33), device=eng.device)
    a, b = eng.chain_autocorr(x, return_rho=True), eng.chain_autocorr(x, return_rho=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert eng.chain_rhat(x).tobytes() == eng.chain_rhat(x).tobytes()


def test_launch_counters(eng):
    """`profile_report` names the kernels of csrc/asmc_diag.hip and nothing else of the library runs: one moments launch, one
    lag-block and one finishing launch per block until the last window is found."""
    x = R.fixture(131, 257, 8)
    dev = torch.as_tensor(x, device=eng.device)
    eng.profile(True)
    try:
        _, window = eng.chain_autocorr(dev)
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    blocks = int(window.max()) // R.KB + 1
    assert blocks > 1 and set(rep) == ACF_KERNELS, rep
    assert rep["k_chain_moments"][0] == 1 and rep["k_chain_acf_block"][0] == blocks and rep["k_chain_acf_finish"][0] == blocks, rep
    eng.profile(True)
    try:
        eng.chain_rhat(dev)
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    assert {k: v[0] for k, v in rep.items()} == RHAT_KERNELS, rep


def test_argument_errors(eng):
    from aspire_amd._lib import AsmcError

    x = torch.zeros((4, 3, 2), dtype=torch.float64, device=eng.device)
    with pytest.raises(AssertionError):
        eng.chain_autocorr(x.transpose(0, 1))
    with pytest.raises(TypeError):
        eng.chain_rhat(x.to(torch.float16))
    with pytest.raises(AsmcError, match="kb is 16 or 32"):
        eng.chain_autocorr(x, kb=8)


@pytest.mark.parametrize("sampler", ["emcee", "minipcn", "pt_minipcn"])
def test_end_to_end(eng, sampler):
    """sample_posterior(autocorr=True) at 256 walkers x d = 4 x 60 steps: the field is the restatement of the returned chain within
    the bound, and the chain is bit for bit the chain of the same seed without the keyword."""
    from aspire_amd import Aspire, Samples
    from aspire_amd.targets import DiagGaussianMixture

    W, d, steps = 256, 4, 60
    lik = DiagGaussianMixture.isotropic(d, mean=1.0, var=1.0, normalized=True)
    pri = DiagGaussianMixture.isotropic(d, mean=0.0, var=4.0, normalized=True)
    kw = {"emcee": dict(nwalkers=W, nsteps=steps), "minipcn": dict(n_walkers=W, n_steps=steps),
          "pt_minipcn": dict(n_walkers=W, n_steps=steps, n_temps=3)}[sampler]

    def run(**extra):
        aspire = Aspire(log_likelihood=lik, log_prior=pri, dims=d, flow_backend="gaussian")
        aspire.fit(Samples(1.5 * np.random.default_rng(0).normal(size=(500, d))))
        return aspire.sample_posterior(n_samples=None, sampler=sampler, engine=eng, rng=np.random.default_rng(1), **kw, **extra)

    out, plain = run(autocorr=True), run()
    assert plain.autocorrelation_time is None
    assert np.asarray(out.x).tobytes() == np.asarray(plain.x).tobytes()
    assert np.asarray(out.log_likelihood).tobytes() == np.asarray(plain.log_likelihood).tobytes()
    tau = np.asarray(out.autocorrelation_time)
    chains = np.asarray(out.chain) if sampler == "pt_minipcn" else np.asarray(out.chain)[None]
    assert tau.shape == ((3, d) if sampler == "pt_minipcn" else (d,))
    for r, chain in enumerate(chains):
        ref = R.autocorr_direct(chain)
        assert R.razor_margin(chain) > 1e-6  # (a sampled chain, not a guarded fixture: say so if it ever lands on the edge)
        for j in range(d):
            w = int(ref["window"][j])
            bound = 2 * (w + 1) * float(np.max(R.rho_bound(steps, W, ref["mass"][:w + 1, j])))
            assert abs(tau.reshape(len(chains), d)[r, j] - ref["tau"][j]) <= bound, (sampler, r, j)
