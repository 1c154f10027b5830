"""Ensemble moves of the `"emcee_smc"` and `"emcee"` samplers: stand-ins for emcee's move classes, the parsing of `moves=` and the
per-step move schedule.

emcee is not a dependency, so `StretchMove`, `DEMove` and `DESnookerMove` here only carry the settings, with emcee's constructor
signatures; the moves themselves run in the HIP kernels (csrc/asmc_stretch.hip, csrc/asmc_ensemble.hip).
A move is recognised by its type's name and its attributes, so emcee's own objects work where emcee is installed.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

SUPPORTED = ("moves=None (emcee's default StretchMove(a=2.0)), StretchMove(a) and DEMove(sigma, gamma0) with nsplits=2, "
             "DESnookerMove(gammas) with nsplits=4, each with randomize_split=True, a list of them (equal weights) or a list of "
             "(move, weight) pairs")


class _RedBlue:
    def __init__(self, nsplits=2, randomize_split=True, live_dangerously=False):
        self.nsplits, self.randomize_split, self.live_dangerously = int(nsplits), bool(randomize_split), bool(live_dangerously)

    def __repr__(self):
        args = ", ".join(f"{k}={v!r}" for k, v in vars(self).items())
        return f"{type(self).__name__}({args})"


class StretchMove(_RedBlue):
    """emcee.moves.StretchMove(a=2.0, **kwargs): Goodman & Weare's stretch move."""

    def __init__(self, a=2.0, **kwargs):
        self.a = a
        super().__init__(**kwargs)


class DEMove(_RedBlue):
    """emcee.moves.DEMove(sigma=1e-5, gamma0=None, **kwargs): differential evolution; gamma0=None is 2.38 / sqrt(2 d)."""

    def __init__(self, sigma=1.0e-5, gamma0=None, **kwargs):
        self.sigma, self.gamma0 = sigma, gamma0
        super().__init__(**kwargs)


class DESnookerMove(_RedBlue):
    """emcee.moves.DESnookerMove(gammas=1.7, **kwargs): the snooker update, on four groups."""

    def __init__(self, gammas=1.7, **kwargs):
        self.gammas = gammas
        kwargs.setdefault("nsplits", 4)
        super().__init__(**kwargs)


@dataclass(frozen=True)
class MoveSpec:
    kind: str  # "stretch", "de" or "snooker"
    nsplits: int
    p0: float | None  # stretch: a; de: gamma0 (None: 2.38 / sqrt(2 d)); snooker: gammas
    p1: float = 0.0  # de: sigma

    def params(self, d: int) -> tuple[float, float]:
        return (2.38 / math.sqrt(2.0 * d) if self.p0 is None else self.p0), self.p1


@dataclass(frozen=True)
class MoveSet:
    specs: tuple
    weights: tuple  # normalised
    live_dangerously: bool
    default: bool = False  # moves=None or one StretchMove: the stretch kernels alone, two walkers suffice, its own path name

    @property
    def names(self) -> str:
        return " + ".join(f"{w:.3g} {s.kind}" for s, w in zip(self.specs, self.weights))

    @property
    def path(self) -> str:
        """What a sampler's `last_mutation_path` says about a mutation by these moves."""
        if self.default:
            return "stretch move: propose / densities / accept per half-sweep (asmc_stretch_*)"
        return (f"ensemble moves ({self.names}), one per step: propose / densities / accept per group-sweep (asmc_ensemble_*, "
                "asmc_stretch_*)")

    def schedule(self, seed: int, nsteps: int) -> np.ndarray:
        """The move of every step of a mutation, a function of the mutation's seed alone (one move per step, as emcee's
        EnsembleSampler.sample draws it)."""
        if len(self.specs) == 1:
            return np.zeros(nsteps, dtype=np.int64)
        return np.random.default_rng(seed).choice(len(self.specs), size=nsteps, p=np.asarray(self.weights))


def is_default_path(moves) -> bool:
    """moves=None or one StretchMove: the sampler's original code path (asmc_stretch_* alone, no schedule)."""
    return moves is None or type(moves).__name__ == "StretchMove"


def _finite(name, value) -> float:
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"{name} must be finite, got {value}")
    return value


def _one(move) -> tuple[MoveSpec, bool]:
    name = type(move).__name__
    want = {"StretchMove": 2, "DEMove": 2, "DESnookerMove": 4}.get(name)
    if want is None:
        raise NotImplementedError(f"the move {move!r} is not implemented by the HIP kernels; supported: {SUPPORTED}")
    nsplits = getattr(move, "nsplits", want)
    if nsplits != want or not getattr(move, "randomize_split", True):
        raise NotImplementedError(f"{name} with nsplits={nsplits}, randomize_split={getattr(move, 'randomize_split', True)} is not "
                                  f"implemented; supported: {SUPPORTED}")
    if name == "StretchMove":
        a = float(getattr(move, "a", 2.0))
        if not 1.0 < a < np.inf:
            raise ValueError(f"the stretch scale a must be finite and > 1, got {a}")
        spec = MoveSpec("stretch", 2, a)
    elif name == "DEMove":
        g0 = getattr(move, "gamma0", None)
        spec = MoveSpec("de", 2, None if g0 is None else _finite("DEMove's gamma0", g0), _finite("DEMove's sigma", getattr(move, "sigma", 1.0e-5)))
    else:
        spec = MoveSpec("snooker", 4, _finite("DESnookerMove's gammas", getattr(move, "gammas", 1.7)))
    return spec, bool(getattr(move, "live_dangerously", False))


def parse_moves(moves) -> MoveSet:
    """`moves=` in emcee's forms: None, one move, a list of moves, a list of (move, weight) pairs."""
    if moves is None:
        moves = [StretchMove()]
    if isinstance(moves, (str, bytes, dict)) or not isinstance(moves, (list, tuple)):
        moves = [moves]
    if len(moves) == 0:
        raise ValueError("moves is an empty list")
    pairs = [m if isinstance(m, (list, tuple)) else (m, 1.0) for m in moves]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("every entry of a list of moves is a move or a (move, weight) pair")
    weights = np.array([float(w) for _, w in pairs])
    if not (np.all(np.isfinite(weights)) and np.all(weights > 0.0)):
        raise ValueError(f"the weights of moves must be positive and finite, got {weights.tolist()}")
    parsed = [_one(m) for m, _ in pairs]
    return MoveSet(tuple(s for s, _ in parsed), tuple((weights / weights.sum()).tolist()), any(live for _, live in parsed))


def require_engine(engine, moves) -> None:
    """Anything but the default path needs the engine's DE / snooker entry points; checked before any attribute of `moves` is
    read."""
    if not (hasattr(engine, "ensemble_propose") and hasattr(engine, "ensemble_accept")):
        raise NotImplementedError(f"moves={moves!r} needs an engine with ensemble_propose / ensemble_accept (the DE and snooker "
                                  f"kernels), which {type(engine).__name__} lacks; without them: moves=None (emcee's default "
                                  "StretchMove(a=2.0)) or a single StretchMove(a=...)")


def run_step(engine, spec: MoveSpec, d: int, z, beta: float, ll, lp, lq, logj, densities, seed: int, shard: int, step: int, t: int) -> None:
    """One Markov step of `spec` in place: its group-sweeps of propose -> densities(y) = (ll, lp, lq, logj) -> accept."""
    p0, p1 = spec.params(d)
    for g in range(spec.nsplits):
        if spec.kind == "stretch":
            y, logf = engine.stretch_propose(z, g, p0, seed, shard, step, t)
        else:
            y, logf = engine.ensemble_propose(z, spec.kind, spec.nsplits, g, p0, p1, seed, shard, step, t)
        ll_new, lp_new, lq_new, logj_new = densities(y)
        if spec.kind == "stretch":
            engine.stretch_accept(z, g, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, t, logj=logj,
                                  logj_new=logj_new)
        else:
            engine.ensemble_accept(z, spec.nsplits, g, y, logf, beta, ll, lp, lq, ll_new, lp_new, lq_new, seed, shard, step, t,
                                   logj=logj, logj_new=logj_new)
