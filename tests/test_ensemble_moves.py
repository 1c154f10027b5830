"""The DE and snooker moves and move mixtures of the "emcee_smc" / "emcee" samplers on the CPU test double: the four-way split, the
DE pairs, the parsing of `moves=`, the per-step schedule, the stationarity of each move's restatement, end-to-end runs with a
resumed checkpoint, and the ABI.

Specification: include/asmc.h asmc_ensemble_*, DESIGN.md §3.26 (emcee is absent: the snooker factor is derived there).  The device
kernels are checked against tests/ensemble_ref.py in tests/test_gpu_ensemble_moves.py.
"""
import math
import os
import re

import numpy as np
import pytest

import ensemble_ref as E
import stretch_ref as S
from chain_ref import ChainOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234_5678_9ABC


class ChainEnsembleEngine(ChainOracleEngine, E.EnsembleOracleEngine):
    """The "emcee" sampler's test double with the DE / snooker entry points."""


# ---- the split ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 6, 7, 17, 4097])
def test_four_way_split_is_a_bijection_with_the_specified_sizes(n):
    gr = E.groups(n, 4, 3, 0, SEED)
    assert [len(g) for g in gr] == [math.ceil((n - g) / 4) for g in range(4)] and min(len(g) for g in gr) >= 1
    assert sorted(np.concatenate(gr).tolist()) == list(range(n))
    s = S.sigma(np.arange(n), n, 3, 0, SEED)
    for g in range(4):
        assert np.all(s[gr[g]] % 4 == g)
    # S = 2 is the stretch move's split, bit for bit
    halves = E.groups(n, 2, 3, 0, SEED)
    for h in (0, 1):
        assert np.array_equal(halves[h], S.draws(n, h, 3, 0, SEED)[0])
        assert np.array_equal(E.draws(n, "de", h, 3, 0, SEED)["k"], halves[h])


@pytest.mark.parametrize("n", [4, 5, 7, 17, 4097])
def test_de_pairs_are_distinct_and_in_the_other_half(n):
    s = S.sigma(np.arange(n), n, 5, 2, SEED)
    for h in (0, 1):
        dr = E.draws(n, "de", h, 5, 2, SEED)
        assert np.all(dr["j1"] != dr["j2"])
        assert np.all(s[dr["j1"]] % 2 == 1 - h) and np.all(s[dr["j2"]] % 2 == 1 - h) and np.all(s[dr["k"]] % 2 == h)
        assert np.all((dr["u_acc"] > 0) & (dr["u_acc"] < 1)) and np.all(np.isfinite(dr["xi"]))


def test_de_pairs_with_four_walkers_take_both_orders():
    seen = set()
    for step in range(40):
        dr = E.draws(4, "de", 0, step, 0, SEED)
        other = sorted(E.groups(4, 2, step, 0, SEED)[1].tolist())
        for j1, j2 in zip(dr["j1"], dr["j2"]):
            assert sorted((int(j1), int(j2))) == other
            seen.add(int(j1) < int(j2))
    assert seen == {True, False}


@pytest.mark.parametrize("n", [4, 7, 4097])
def test_snooker_partners_come_one_from_each_other_group_and_are_shuffled(n):
    s = S.sigma(np.arange(n), n, 9, 1, SEED)
    perms = set()
    for g in range(4):
        dr = E.draws(n, "snooker", g, 9, 1, SEED)
        others = [o for o in range(4) if o != g]
        assert np.array_equal(s[dr["c"]] % 4, np.tile(others, (len(dr["k"]), 1)))
        assert np.all((dr["r"] >= 0) & (dr["r"] < 6))
        for i in range(len(dr["k"])):
            assert sorted((dr["z"][i], dr["z1"][i], dr["z2"][i])) == sorted(dr["c"][i])
            assert (dr["z"][i], dr["z1"][i], dr["z2"][i]) == tuple(dr["c"][i][E.PERMS[dr["r"][i]]])
        perms |= set(dr["r"].tolist())
    assert n < 100 or perms == set(range(6))
    assert [tuple(p) for p in E.PERMS] == sorted(tuple(p) for p in E.PERMS)  # lexicographic order


# ---- option parsing ----------------------------------------------------------------------------------------------------------------
def test_moves_are_exported_with_emcees_signatures():
    import aspire_amd
    from aspire_amd import DEMove, DESnookerMove, StretchMove

    assert {"StretchMove", "DEMove", "DESnookerMove"} <= set(aspire_amd.__all__)
    assert (StretchMove().a, StretchMove().nsplits, StretchMove(live_dangerously=True).live_dangerously) == (2.0, 2, True)
    assert (DEMove().sigma, DEMove().gamma0, DEMove().nsplits, DEMove(1e-3, 0.5).gamma0) == (1e-5, None, 2, 0.5)
    assert (DESnookerMove().gammas, DESnookerMove().nsplits, DESnookerMove(gammas=1.2).gammas) == (1.7, 4, 1.2)


def test_every_accepted_form_of_moves():
    from aspire_amd import DEMove, DESnookerMove, StretchMove
    from aspire_amd.moves import is_default_path, parse_moves

    assert is_default_path(None) and is_default_path(StretchMove(1.5)) and not is_default_path([StretchMove()])
    assert not is_default_path(DEMove())
    one = parse_moves(None)
    assert [s.kind for s in one.specs] == ["stretch"] and one.weights == (1.0,) and one.specs[0].params(8) == (2.0, 0.0)
    de = parse_moves(DEMove())
    assert (de.specs[0].kind, de.specs[0].nsplits, de.weights) == ("de", 2, (1.0,))
    assert de.specs[0].params(32) == (2.38 / math.sqrt(64.0), 1e-5)  # gamma0=None: 2.38 / sqrt(2 d)
    assert parse_moves(DEMove(sigma=0.1, gamma0=0.7)).specs[0].params(32) == (0.7, 0.1)
    sn = parse_moves(DESnookerMove(gammas=1.3))
    assert (sn.specs[0].kind, sn.specs[0].nsplits, sn.specs[0].params(5)) == ("snooker", 4, (1.3, 0.0))
    eq = parse_moves([DEMove(), DESnookerMove(), StretchMove()])
    assert [s.kind for s in eq.specs] == ["de", "snooker", "stretch"] and eq.weights == pytest.approx((1 / 3,) * 3)
    mix = parse_moves([(DEMove(), 8.0), (DESnookerMove(), 2.0)])
    assert mix.weights == pytest.approx((0.8, 0.2)) and sum(mix.weights) == pytest.approx(1.0) and not mix.live_dangerously
    assert parse_moves([(DEMove(live_dangerously=True), 1), DESnookerMove()]).live_dangerously
    assert "de" in mix.names and "snooker" in mix.names

    # recognised by the type's name and its attributes, as emcee's own objects would be
    foreign = type("DESnookerMove", (), {"gammas": 1.1, "nsplits": 4, "randomize_split": True})()
    assert parse_moves(foreign).specs[0].params(3) == (1.1, 0.0)


@pytest.mark.parametrize("weight", [0.0, -1.0, np.inf, np.nan])
def test_bad_weights(weight):
    from aspire_amd import DEMove, DESnookerMove
    from aspire_amd.moves import parse_moves

    with pytest.raises(ValueError, match="positive and finite"):
        parse_moves([(DEMove(), 0.8), (DESnookerMove(), weight)])


def test_unsupported_moves_name_what_is_supported():
    from aspire_amd import DEMove, DESnookerMove, StretchMove
    from aspire_amd.moves import parse_moves

    class WalkMove:
        pass

    for bad in (WalkMove(), "stretch", [WalkMove()], DEMove(nsplits=4), DESnookerMove(nsplits=2), StretchMove(nsplits=4),
                DEMove(randomize_split=False)):
        with pytest.raises(NotImplementedError, match=r"supported: .*StretchMove.*DEMove.*DESnookerMove.*nsplits=4"):
            parse_moves(bad)
    with pytest.raises(ValueError, match="finite"):
        parse_moves(DEMove(gamma0=np.inf))
    with pytest.raises(ValueError, match="empty"):
        parse_moves([])


def _smc(d, eng, seed=4, **kw):
    from aspire_amd.flows import GaussianFlow
    from aspire_amd.samplers.emcee_smc import HipEmceeSMC
    from aspire_amd.targets import DiagGaussianMixture

    lik = DiagGaussianMixture.isotropic(d, normalized=False)
    return HipEmceeSMC(log_likelihood=lik, log_prior=lik, dims=d, prior_flow=GaussianFlow(d, sigma=2.0, engine=eng, seed=3), xp=np,
                       engine=eng, rng=np.random.default_rng(seed), **kw)


def _mcmc(eng, d=4, seed=0):
    from test_mcmc_samplers import make

    return make("emcee", d=d, seed=seed, eng=eng)


def test_engines_without_the_entry_points_keep_both_pinned_messages():
    """What tests/test_emcee_smc.py and tests/test_mcmc_samplers.py pin, on their test doubles: the capability check comes before
    any attribute of the move is read, and its message has both `moves` and `StretchMove`."""
    from aspire_amd import DEMove, DESnookerMove, StretchMove

    class Bare:  # (no attribute at all)
        pass

    Bare.__name__ = "DEMove"
    for bad in (Bare(), DEMove(), [StretchMove()], [(DEMove(), 0.8), (DESnookerMove(), 0.2)], "stretch"):
        with pytest.raises(NotImplementedError, match=r"(?s)moves.*StretchMove"):
            _smc(2, S.StretchOracleEngine()).sample(64, sampler_kwargs={"nsteps": 2, "moves": bad}, store_sample_history=False)
        with pytest.raises(NotImplementedError, match=r"(?s)moves.*StretchMove"):
            _mcmc(ChainOracleEngine()).sample(nwalkers=10, nsteps=3, moves=bad)


def test_walker_rules():
    from aspire_amd import DEMove

    with pytest.raises(ValueError, match="at least four walkers"):
        _smc(1, E.EnsembleOracleEngine()).sample(3, sampler_kwargs={"nsteps": 2, "moves": DEMove()}, store_sample_history=False)
    with pytest.raises(ValueError, match="at least four walkers"):
        _mcmc(ChainEnsembleEngine(), d=1).sample(nwalkers=3, nsteps=3, moves=DEMove())
    with pytest.raises(RuntimeError, match="red-blue move"):
        _mcmc(ChainEnsembleEngine()).sample(nwalkers=7, nsteps=3, moves=DEMove())
    assert _mcmc(ChainEnsembleEngine()).sample(nwalkers=7, nsteps=3, moves=DEMove(live_dangerously=True)).chain_shape == (3, 7)
    assert _mcmc(ChainEnsembleEngine()).sample(nwalkers=7, nsteps=3, moves=DEMove(), live_dangerously=True).chain_shape == (3, 7)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
def test_schedule_is_a_function_of_the_seed_with_the_weights_frequencies():
    from aspire_amd import DEMove, DESnookerMove
    from aspire_amd.moves import parse_moves

    mix = parse_moves([(DEMove(), 0.8), (DESnookerMove(), 0.2)])
    a, b = mix.schedule(77, 4000), mix.schedule(77, 4000)
    assert np.array_equal(a, b) and not np.array_equal(a, mix.schedule(78, 4000))
    assert np.array_equal(a, np.random.default_rng(77).choice(2, size=4000, p=[0.8, 0.2]))
    assert abs(int((a == 0).sum()) - 3200) <= 4.0 * math.sqrt(4000 * 0.8 * 0.2)
    assert np.array_equal(parse_moves(DEMove()).schedule(77, 10), np.zeros(10))


class CountingRng:
    """A generator that counts what is drawn from it."""

    def __init__(self, seed):
        self._g, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        attr = getattr(self._g, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.calls.append(name)
            return attr(*a, **k)

        return call


def test_default_path_draws_what_it_drew_and_mixtures_draw_nothing_more():
    from aspire_amd import DEMove, DESnookerMove, StretchMove

    runs = {}
    for name, moves in (("none", None), ("stretch", StretchMove(2.0)), ("mix", [(DEMove(), 0.8), (DESnookerMove(), 0.2)])):
        rng = CountingRng(4)
        sp = _smc(2, E.EnsembleOracleEngine())
        post = sp.sample(256, sampler_kwargs={"nsteps": 4, "moves": moves}, store_sample_history=False, rng=rng)
        runs[name] = (np.asarray(post.x), list(rng.calls), sp.last_mutation_path)
    # the stand-in of this test double is StretchOracleEngine's code: the same bits as a run on it
    ref = _smc(2, S.StretchOracleEngine()).sample(256, sampler_kwargs={"nsteps": 4}, store_sample_history=False,
                                                  rng=np.random.default_rng(4))
    assert np.array_equal(runs["none"][0], np.asarray(ref.x)) and np.array_equal(runs["none"][0], runs["stretch"][0])
    assert runs["none"][1] == runs["stretch"][1]
    assert "stretch move" in runs["none"][2] and "asmc_ensemble" not in runs["none"][2]
    assert re.search(r"0\.8 de \+ 0\.2 snooker", runs["mix"][2])
    # one seed per mutation from the sampler's generator, mixture or not: the schedule comes from that seed
    per_mutation = [c for c in runs["none"][1] if c == "integers"]
    assert len(per_mutation) >= 2
    assert not np.array_equal(runs["mix"][0], runs["none"][0])


def test_mixture_mutation_takes_one_draw_from_the_generator(monkeypatch):
    from aspire_amd import DEMove, DESnookerMove

    counts = {}
    for name, moves in (("none", None), ("mix", [(DEMove(), 0.8), (DESnookerMove(), 0.2)])):
        sp = _smc(2, E.EnsembleOracleEngine())
        sp.sample(256, sampler_kwargs={"nsteps": 3, "moves": moves}, store_sample_history=False, n_steps=None)
        rng = CountingRng(5)
        sp.rng = rng
        particles = sp._wrap(*(sp.engine.asarray(v) for v in (np.random.default_rng(0).normal(size=(64, 2)), np.zeros(64), np.zeros(64),
                                                             np.zeros(64))), 0.5)
        sp.mutate(particles, 0.5)
        counts[name] = list(rng.calls)
    assert counts["none"] == counts["mix"] == ["integers"]


# ---- stationarity ------------------------------------------------------------------------------------------------------------------
def _correlated_gaussian_run(kinds, weights, snooker_log_factor=True, n=4000, steps=100, seed=11):
    """tests/test_emcee_smc.py's correlated Gaussian (same ensemble size, step count and seed), one move per step."""
    cov = np.array([[1.0, 0.9], [0.9, 1.0]])
    prec = np.linalg.inv(cov)
    g = np.random.default_rng(seed)
    x = g.multivariate_normal([0.0, 0.0], cov, size=n)

    def logp(z):
        return -0.5 * np.einsum("ni,ij,nj->n", z, prec, z)

    ll, zero = logp(x), np.zeros(n)
    lp, lq = zero.copy(), zero.copy()
    schedule = np.random.default_rng(99).choice(len(kinds), size=steps, p=weights)
    accepted = 0
    for t in range(steps):
        kind = kinds[schedule[t]]
        nsplits = 2 if kind == "de" else 4
        for grp in range(nsplits):
            if kind == "de":
                y, logf, _ = E.propose_de(x, grp, 2.38 / math.sqrt(2.0 * 2), 1e-5, 99, 0, t)
            else:
                y, logf, _ = E.propose_snooker(x, grp, 1.7, 99, 0, t, log_factor=snooker_log_factor)
            z = np.zeros(len(y))
            acc, _ = E.accept(x, nsplits, grp, y, logf, 1.0, ll, lp, lq, logp(y), z, z, 99, 0, t)
            accepted += int(acc.sum())
    return x, cov, accepted / (n * steps)


@pytest.mark.parametrize("kinds,weights", [(("de",), (1.0,)), (("snooker",), (1.0,)), (("de", "snooker"), (0.8, 0.2))],
                         ids=["de", "snooker", "mixture"])
def test_numpy_moves_keep_a_correlated_gaussian_stationary(kinds, weights):
    """At beta = 1 each move, and the mixture, leaves N(0, Sigma) invariant: the thresholds, ensemble size and step count of
    test_numpy_move_keeps_a_correlated_gaussian_stationary.  Without the snooker's factor (d - 1)(log |y - z| - log |x_k - z|) the
    snooker does not (checked by hand with snooker_log_factor=False: the ensemble contracts, its variances end at 0.64, far
    outside the tolerance)."""
    x, cov, rate = _correlated_gaussian_run(kinds, weights)
    assert 0.1 < rate < 0.95
    assert np.all(np.abs(x.mean(axis=0)) < 0.1)
    np.testing.assert_allclose(np.cov(x.T), cov, atol=0.1)


def test_snooker_degenerate_rows_in_the_restatement():
    """Half the rows are copies of one row: r0 = 0 slots keep x_k with logf = -inf and are rejected; nothing is NaN."""
    g = np.random.default_rng(3)
    x = g.normal(size=(64, 3))
    x[::2] = x[0]
    y, logf, dr = E.propose_snooker(x, 0, 1.7, 5, 0, 0)
    dup = np.all(x[dr["k"]] == x[dr["z"]], axis=1)
    assert dup.any() and not dup.all()
    assert np.all(np.isfinite(y)) and not np.any(np.isnan(logf))
    assert np.all(np.isneginf(logf[dup])) and np.array_equal(y[dup], x[dr["k"]][dup]) and np.all(np.isfinite(logf[~dup]))
    ll = np.zeros(64)
    acc, _ = E.accept(x, 4, 0, y, logf, 1.0, ll, ll.copy(), ll.copy(), np.zeros(len(y)), np.zeros(len(y)), np.zeros(len(y)), 5, 0, 0)
    assert not acc[dup].any() and np.all(np.isfinite(x))


# ---- end to end on the doubles -----------------------------------------------------------------------------------------------------
class Collector:
    def __init__(self):
        self.states = []

    def __call__(self, state):
        self.states.append(dict(state))


def _mixture():
    from aspire_amd import DEMove, DESnookerMove

    return [(DEMove(), 0.8), (DESnookerMove(), 0.2)]


def test_emcee_smc_with_the_mixture_and_a_resumed_run():
    d = 2
    col = Collector()
    kw = dict(sampler_kwargs={"nsteps": 6, "moves": _mixture()}, store_sample_history=False)
    sp = _smc(d, E.EnsembleOracleEngine())
    post = sp.sample(512, checkpoint_callback=col, checkpoint_every=1, **kw)
    assert np.asarray(post.x).shape == (512, d) and np.isfinite(float(post.log_evidence)) and np.isfinite(float(post.log_evidence_error))
    assert abs(float(post.log_evidence) - math.log(math.pi)) < 0.5
    h = sp.history
    assert len(h.mcmc_acceptance) == len(h.beta) == len(h.mcmc_autocorr) and all(0.02 < a < 1.0 for a in h.mcmc_acceptance)
    assert "de" in sp.last_mutation_path and "snooker" in sp.last_mutation_path
    assert len(col.states) >= 2
    sp2 = _smc(d, E.EnsembleOracleEngine(), seed=999)  # (the generator comes from the checkpoint)
    post2 = sp2.sample(512, resume_from=col.states[len(col.states) // 2], **kw)
    assert np.array_equal(np.asarray(post2.x), np.asarray(post.x)) and float(post2.log_evidence) == float(post.log_evidence)
    assert sp2.history.mcmc_acceptance[-2:] == h.mcmc_acceptance[-2:]


@pytest.mark.parametrize("moves", ["de", "snooker", "mixture"])
def test_emcee_with_the_new_moves(moves):
    from aspire_amd import DEMove, DESnookerMove

    mv = {"de": DEMove(), "snooker": DESnookerMove(), "mixture": _mixture()}[moves]
    sp = _mcmc(ChainEnsembleEngine())
    out = sp.sample(nwalkers=24, nsteps=40, moves=mv)
    assert out.chain_shape == (40, 24) and np.all(np.isfinite(np.asarray(out.x)))
    assert 0.02 < sp.history.mcmc_acceptance[-1] < 1.0 and moves.replace("mixture", "snooker") in sp.last_mutation_path
    again = _mcmc(ChainEnsembleEngine()).sample(nwalkers=24, nsteps=40, moves=mv)
    assert np.array_equal(np.asarray(out.x), np.asarray(again.x))
    assert not np.array_equal(np.asarray(out.x), np.asarray(_mcmc(ChainEnsembleEngine()).sample(nwalkers=24, nsteps=40).x))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_33_declares_the_new_entry_points():
    from aspire_amd import _lib

    assert _lib.ASMC_ABI_VERSION == 33
    header = open(os.path.join(ROOT, "include", "asmc.h")).read()
    assert "#define ASMC_ABI_VERSION 33" in header
    for sym in ("asmc_ensemble_propose", "asmc_ensemble_accept"):
        assert sym in _lib.SIGNATURES and re.search(rf"\bint {sym}\(", header)
    lib = _lib.load()
    assert lib.asmc_abi_version() == 33 and hasattr(lib, "asmc_ensemble_propose") and hasattr(lib, "asmc_ensemble_accept")
