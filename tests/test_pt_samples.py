"""`PTMCMCSamples` (reference samples.py:810-1205) on numpy arrays: the two evidence estimators against a straight numpy evaluation
of the reference's formulas (tests/pt_ref.py) at the reference's own rel 1e-12, every ValueError it raises, and the container's
methods.  The device path of the estimators is checked in tests/test_gpu_pt.py; the restatement of its reductions here.
"""
import pickle

import numpy as np
import pytest

import pt_ref

LADDERS = {  # (T, ends at 0)
    (2, True): [1.0, 0.0], (2, False): [1.0, 0.3],
    (3, True): [1.0, 0.2, 0.0], (3, False): [1.0, 0.4, 0.05],
    (5, True): [1.0, 0.5, 0.1, 0.01, 0.0], (5, False): [1.0, 0.6, 0.3, 0.1, 0.02],
}


def container(T, S, W, zero, seed=0, d=2, **kw):
    from aspire_amd import PTMCMCSamples

    g = np.random.default_rng(1000 * T + 10 * S + W + seed)
    ll = -3.0 + 4.0 * g.normal(size=(T, S, W))
    betas = np.array(LADDERS[(T, zero)])
    s = PTMCMCSamples.from_chain(chain=g.normal(size=(T, S, W, d)), betas=betas, log_likelihood=ll, log_prior=ll - 1.0, **kw)
    return s, ll, betas


@pytest.mark.parametrize("T", [2, 3, 5])
@pytest.mark.parametrize("S", [1, 4, 10])
@pytest.mark.parametrize("W", [1, 7])
@pytest.mark.parametrize("zero", [True, False])
def test_evidence_matches_the_reference_formulas(T, S, W, zero):
    s, ll, betas = container(T, S, W, zero)
    for frac in (None, 0.1, 0.5):
        kept = S - (int(S * frac) if frac is not None else 0)
        for method in ("variance", "coarse"):
            got = s.log_evidence_thermodynamic_integration(burn_in_fraction=frac, method=method)
            want = pt_ref.reference_ti(ll, betas, frac, method)
            assert all(isinstance(v, float) for v in got)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        if zero:
            got = s.log_evidence_stepping_stone(burn_in_fraction=frac)
            np.testing.assert_allclose(got, pt_ref.reference_stepping_stone(ll, betas, frac), rtol=1e-12, atol=0)
        else:
            with pytest.raises(ValueError, match="hottest chain to be at beta=0"):
                s.log_evidence_stepping_stone(burn_in_fraction=frac)
        assert kept >= 1


def test_the_restated_reductions_give_the_same_numbers():
    """tests/pt_ref.py evidence_table (what asmc_pt_evidence computes) through the container's scalar arithmetic = the formulas."""
    s, ll, betas = container(5, 10, 7, True)
    tab = pt_ref.PTOracleEngine().pt_evidence(__import__("torch").from_numpy(ll.reshape(-1)), 5, 70, 7, 63, pt_ref.trapezoid_coefficients(betas))
    n = 63
    logz = float(np.sum(pt_ref.trapezoid_coefficients(betas)[0] * tab[:5, 0] / n))
    want = pt_ref.reference_ti(ll, betas, 0.1)
    np.testing.assert_allclose([logz, np.sqrt(tab[5, 2] / n / n)], want, rtol=1e-12)
    ss = sum(np.log(tab[j, 2] / n) + tab[j, 1] for j in range(1, 5))
    err = np.sqrt(sum(tab[j, 3] / (tab[j, 2] / n) ** 2 for j in range(1, 5)) / n**2)
    np.testing.assert_allclose([ss, err], pt_ref.reference_stepping_stone(ll, betas, 0.1), rtol=1e-12)


def test_non_finite_values_propagate_as_in_the_reference():
    s, ll, betas = container(3, 10, 7, True)
    for value, rung in ((-np.inf, 2), (np.nan, 1), (np.inf, 2)):
        bad = ll.copy()
        bad[rung, 5, 3] = value
        s.log_likelihood = bad.reshape(-1)
        with np.errstate(invalid="ignore"):
            for method in ("variance", "coarse"):
                np.testing.assert_array_equal(s.log_evidence_thermodynamic_integration(method=method), pt_ref.reference_ti(bad, betas, 0.1, method))
            np.testing.assert_allclose(s.log_evidence_stepping_stone(), pt_ref.reference_stepping_stone(bad, betas, 0.1), rtol=1e-12)
    const = np.full_like(ll, -2.5)
    s.log_likelihood = const.reshape(-1)
    assert s.log_evidence_thermodynamic_integration() == (-2.5, 0.0)
    assert s.log_evidence_stepping_stone()[1] == pytest.approx(np.sqrt(2 / 63), rel=1e-15)


def test_every_value_error_of_the_reference():
    from aspire_amd import PTMCMCSamples

    s, ll, betas = container(3, 4, 2, True)
    nob = PTMCMCSamples.from_chain(chain=np.zeros((3, 4, 2, 2)), log_likelihood=ll)
    for fn in (nob.log_evidence_thermodynamic_integration, nob.log_evidence_stepping_stone):
        with pytest.raises(ValueError, match="Betas must be provided"):
            fn()
    with pytest.raises(ValueError, match="hottest chain to be at beta=0"):
        container(3, 4, 2, False)[0].log_evidence_stepping_stone()
    with pytest.raises(ValueError, match="No samples available after burn-in for TI"):
        s.log_evidence_thermodynamic_integration(burn_in_fraction=1.0)
    with pytest.raises(ValueError, match="No samples available after burn-in for stepping-stone"):
        s.log_evidence_stepping_stone(burn_in_fraction=1.0)
    with pytest.raises(ValueError, match="Invalid method"):
        s.log_evidence_thermodynamic_integration(method="bootstrap")
    chain = np.zeros((3, 4, 2, 2))
    for bad, msg in (([[1.0, 0.5, 0.0]], "1D"), ([1.0, 0.0], "Length of betas"), ([0.9, 0.5, 0.0], "start at 1"),
                     ([1.0, 0.5, 0.5], "decreasing"), ([1.0, 0.2, 0.4], "decreasing")):
        with pytest.raises(ValueError, match=msg):
            PTMCMCSamples.from_chain(chain=chain, betas=np.array(bad))
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        PTMCMCSamples.from_chain(chain=np.zeros((4, 2)))
    with pytest.raises(NotImplementedError, match="at_temperature"):
        s[:3]
    with pytest.raises(ValueError, match="exceeds available samples"):
        s.subsample(9)


def test_container_methods():
    from aspire_amd import MCMCSamples, PTMCMCSamples

    s, ll, betas = container(3, 10, 7, True, thin=2, burn_in=1)
    assert s.n_temps == 3 and s.chain.shape == (3, 10, 7, 2) and isinstance(s, MCMCSamples)
    cold, hot = s.cold_chain(), s.at_temperature(2)
    assert type(cold) is MCMCSamples and cold.chain_shape == (10, 7) and cold.thin == 2 and cold.burn_in == 1
    assert np.array_equal(cold.log_likelihood, ll[0].reshape(-1)) and np.array_equal(hot.chain, s.chain[2])
    out = s.post_process(burn_in=2, thin=3)  # the step axis is axis 1
    assert isinstance(out, PTMCMCSamples) and out.chain_shape == (3, 3, 7) and out.thin == 6 and out.burn_in == 3
    assert np.array_equal(out.chain, s.chain[:, 2::3]) and np.array_equal(out.log_prior, (ll - 1.0)[:, 2::3].reshape(-1))
    assert np.array_equal(out.betas, betas) and s.post_process() is s
    sub = s.subsample(20, rng=np.random.default_rng(3))
    assert sub.chain_shape == (3, 20) and sub.thin == 2 and sub.burn_in == 1 and np.array_equal(sub.betas, betas)
    for t in range(3):  # rows of their own rung, none twice, densities with them
        pool = {row.tobytes(): v for row, v in zip(s.chain[t].reshape(-1, 2), ll[t].reshape(-1))}
        keys = [row.tobytes() for row in sub.chain[t]]
        assert len(set(keys)) == 20 and all(k in pool for k in keys)
        assert [pool[k] for k in keys] == list(sub.log_likelihood.reshape(3, 20)[t])
    mcmc = MCMCSamples.from_chain(chain=np.zeros((6, 3, 2)))  # the hooks leave the parent as it was
    assert mcmc.post_process(burn_in=1, thin=2).chain_shape == (3, 3) and type(mcmc.to_numpy()) is MCMCSamples


def test_round_trips_carry_betas_and_chain_shape(monkeypatch, tmp_path):
    import torch
    from fake_h5 import FakeFile

    from aspire_amd import PTMCMCSamples, io

    monkeypatch.setattr(io, "open_h5", lambda path, mode="r": FakeFile(path, mode))
    monkeypatch.setattr(io, "h5py_available", lambda: True)
    s, ll, betas = container(3, 4, 2, True, thin=2, burn_in=1)
    with io.open_h5(tmp_path / "pt.h5", "w") as fp:
        s.save(fp, path="samples")
    with io.open_h5(tmp_path / "pt.h5", "r") as fp:
        loaded = PTMCMCSamples.load(fp, path="samples")
    again = pickle.loads(pickle.dumps(s))
    t = s.to_namespace(torch)
    back = t.to_numpy()
    for other in (loaded, again, back):
        assert isinstance(other, PTMCMCSamples) and tuple(other.chain_shape) == (3, 4, 2) and other.chain.shape == (3, 4, 2, 2)
        assert np.array_equal(np.asarray(other.betas), betas) and np.array_equal(np.asarray(other.log_likelihood), ll.reshape(-1))
        assert other.log_evidence_stepping_stone() == s.log_evidence_stepping_stone()
    assert isinstance(t.betas, torch.Tensor) and t.betas.dtype == torch.float64 and isinstance(back.betas, np.ndarray)
    assert t.log_evidence_thermodynamic_integration() == s.log_evidence_thermodynamic_integration()  # (host tensors: host arithmetic)
