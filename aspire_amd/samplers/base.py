"""Sampler base classes (reference src/aspire/samplers/base.py:19-286, samplers/mcmc.py:14-110).

The constructor contract is the reference's `aspire.samplers` entry-point contract
(samplers/base.py:40-50) so the classes here could be registered into a real aspire install.
"""
from __future__ import annotations

import logging
import math
import pickle
from pathlib import Path
from typing import Any, Callable

import numpy as np
import torch

from .._xp import is_torch, is_torch_namespace, to_numpy
from ..comm import Comm, default_comm
from ..samples import Samples, get_default_engine
from ..targets import DiagGaussianMixture, GaussianMixture

logger = logging.getLogger(__name__)


def track_calls(func):
    """utils.py:1003-1029: remember the positional and keyword arguments of every call of a sampler's `sample` method
    (`config_dict` reports them; the checkpoint state carries that config).  The log lives on the instance, keyed by the
    method's qualified name, so a subclass's `sample` and the base `sample` it calls keep separate logs as in the
    reference."""
    import functools

    @functools.wraps(func)
    def wrapper(self, *args, **kwargs):
        log = self.__dict__.setdefault("_call_log", {}).setdefault(func.__qualname__, {"args": [], "kwargs": []})
        log["args"].append(args)
        log["kwargs"].append(kwargs)
        return func(self, *args, **kwargs)

    return wrapper


MAX_CHUNK = 2048  # steps whose accept counts the device holds (ASMC_MAX_PCN_STEPS): one read-back per chunk


def pcn_adapt(rho: float, acc: float, target: float, t: int) -> float:
    """Step-size adaptation of this repository's pCN spec, identical to the device
    version in k_pcn_adapt: log rho += (acc - target)/(t+1)^0.75, rho clipped to [1e-4, 0.99]."""
    r = math.exp(math.log(rho) + (acc - target) / (t + 1) ** 0.75)
    return min(max(r, 1e-4), 0.99)


class IdentityTransform:
    """transforms.py:125-139 — the default "smc" preconditioning for unbounded problems
    (aspire.py:337-341: affine_transform=False, bounded_to_unbounded=False)."""

    def __init__(self, xp=None, dtype=None):
        self.xp, self.dtype = xp, dtype

    def fit(self, x):
        return x

    def forward(self, x):
        return x, None

    def inverse(self, z):
        return z, None

    def new_instance(self, xp=None):
        return IdentityTransform(xp=xp or self.xp, dtype=self.dtype)

    def config_dict(self):
        return {}


class Sampler:
    """samplers/base.py:19-91."""

    def __init__(self, log_likelihood: Callable, log_prior: Callable, dims: int, prior_flow, xp: Callable,
                 dtype: Any | str | None = None, parameters: list[str] | None = None,
                 preconditioning_transform: Callable | None = None, engine=None, comm: Comm | None = None):
        self.prior_flow = prior_flow
        self._log_likelihood = log_likelihood
        self._log_prior = log_prior
        self.dims = dims
        self.xp = xp if xp is not None else np
        self.backend_str = "torch" if is_torch_namespace(self.xp) else "numpy"
        self.dtype = dtype
        self.parameters = parameters
        self.history = None
        self.n_likelihood_evaluations = 0
        self._last_checkpoint_state: dict | None = None
        self._last_checkpoint_bytes: bytes | None = None
        self.preconditioning_transform = preconditioning_transform or IdentityTransform(xp=self.xp)
        self._engine = engine
        self._comm = comm

    # ---- engine / communicator ----------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            self._engine = get_default_engine()
        return self._engine

    @property
    def comm(self) -> Comm:
        if self._comm is None:
            self._comm = default_comm(getattr(self.engine, "device", "cpu"))
        return self._comm

    @property
    def x_torch_dtype(self):
        if self.dtype is None:
            return torch.float64
        if isinstance(self.dtype, torch.dtype):
            return self.dtype
        return {"float32": torch.float32, "float64": torch.float64}[np.dtype(self.dtype).name]

    def fit_preconditioning_transform(self, x):
        return self.preconditioning_transform.fit(x)

    def _transformed(self) -> bool:
        T = self.preconditioning_transform
        return not (isinstance(T, IdentityTransform) or getattr(T, "is_identity", False))

    def _enter_preconditioned(self, x: torch.Tensor):
        """The one entry of a chain into the preconditioned space: T is refitted to the rows x; returns (z = T(x), log|det
        dT^-1/dz| at z, T), or (x, None, None) under the identity.  `fit` gets the communicator so that sharded populations fit
        the global moments; on one rank that is `fit(x)` bit for bit for every class of transforms.py (they only ask
        `comm.sharded`), so the single-rank chain samplers enter here too."""
        e, T = self.engine, self.preconditioning_transform
        if not self._transformed():
            self.fit_preconditioning_transform(x)
            return x, None, None
        if getattr(T, "engine", None) is None and hasattr(T, "engine"):
            T.engine = e
        try:
            z = T.fit(x, comm=self.comm)
        except TypeError:  # a user-supplied transform with the reference's fit(x) signature
            z = T.fit(x)
        z = e.asarray(z, dtype=x.dtype)
        return z, e.asarray(T.inverse(z)[1]), T

    def sample(self, n_samples: int) -> Samples:
        raise NotImplementedError

    # ---- user callables -------------------------------------------------------------------
    def _user_view(self, x_dev: torch.Tensor, **known):
        """The `samples` object handed to user callables: arrays in the sampler's namespace."""
        if is_torch_namespace(self.xp):
            return Samples(x_dev, xp=torch, parameters=self.parameters, **known)
        conv = {k: (None if v is None else to_numpy(v)) for k, v in known.items()}
        return Samples(to_numpy(x_dev), xp=np, parameters=self.parameters, **conv)

    def _to_dev(self, v) -> torch.Tensor:
        return self.engine.asarray(v if is_torch(v) else np.asarray(v, dtype=np.float64))

    def log_likelihood(self, samples) -> Any:
        """samplers/base.py:81-87 (counts evaluations)."""
        self.n_likelihood_evaluations += len(samples)
        return self._log_likelihood(samples)

    def log_prior(self, samples) -> Any:
        return self._log_prior(samples)

    def _builtin_density(self, f, differentiable: bool):
        """How the target `f` is evaluated without the user view - x -> log-density -, or None for a user callable.  The one
        place a target class is dispatched: the mixture kernel for `DiagGaussianMixture`, `evaluate` for `GaussianMixture` (an
        engine without its kernel calls it like any callable); `differentiable`: through their torch `__call__` / `evaluate`."""
        e = self.engine
        if isinstance(f, DiagGaussianMixture):
            return f if differentiable else (lambda x: e.mixture_logpdf(x, f.device_mixture(e)))
        if isinstance(f, GaussianMixture) and (differentiable or hasattr(e, "fullmix_logpdf")):
            return lambda x: f.evaluate(e, x)
        return None

    def _eval_prior_likelihood(self, x_dev: torch.Tensor, log_q_dev: torch.Tensor | None = None, differentiable: bool = False):
        """log_prior then log_likelihood at x (prior first and stored on the samples object passed to
        the likelihood, as reference smc/base.py:512-513 / docs/recipes.rst rely on).  `differentiable`: x is part of an
        autograd graph (split HMC / NUTS); the values keep their graph and the view's `log_prior` is left as the tensor."""
        prior = self._builtin_density(self._log_prior, differentiable)
        likelihood = self._builtin_density(self._log_likelihood, differentiable)
        view = None
        if prior is not None:
            lp = prior(x_dev)
        else:
            view = self._user_view(x_dev, log_q=log_q_dev)
            lp = self._to_dev(self.log_prior(view))
        if likelihood is not None:
            self.n_likelihood_evaluations += x_dev.shape[0]
            ll = likelihood(x_dev)
        else:
            if view is None:
                view = self._user_view(x_dev, log_q=log_q_dev)
            view.log_prior = lp if differentiable else view.array_to_namespace(lp if is_torch_namespace(view.xp) else to_numpy(lp))
            ll = self._to_dev(self.log_likelihood(view))
        return lp, ll

    def _proposal_densities(self, z_prop, T, x_dtype, log_q=None, inverted=None):
        """(x', ll', lp', lq', log|J|' or None) at the proposals z' of a chain in the space of T (None: x itself): back to x
        through T^-1, log q, then prior and likelihood.  `log_q` is the sampler's rule for lq':
          None              the proposal flow at x', which the callables' view carries as `log_q` (the SMC samplers);
          a callable        the same by (z', x', log|J|') -> lq' (`HipSMC`: the flow straight from the preconditioned coordinate);
          a tensor          its first rows, the flow is not asked ("minipcn", "emcee": zeros, the target has no log q term);
          "prior"           lq' := lp' ("pt_minipcn": the slot carries the prior's value).
        `inverted` = (x', log|J|', lq' or None) from a propose kernel that applied T^-1 itself: only what is missing runs."""
        e = self.engine
        lq_new = None
        if inverted is not None:
            x_prop, logj_new, lq_new = inverted
            if lq_new is None:
                lq_new = self._flow_log_prob(x_prop)
        elif T is None:
            x_prop, logj_new = z_prop, None
        else:
            x_prop, logj_new = T.inverse(z_prop)
            x_prop, logj_new = e.asarray(x_prop, dtype=x_dtype), e.asarray(logj_new)
        if lq_new is None and (log_q is None or callable(log_q)):
            lq_new = self._flow_log_prob(x_prop) if log_q is None else log_q(z_prop, x_prop, logj_new)
        lp_new, ll_new = self._eval_prior_likelihood(x_prop, lq_new)
        if lq_new is None:
            lq_new = lp_new if isinstance(log_q, str) else log_q[:x_prop.shape[0]]
        return x_prop, ll_new, lp_new, lq_new, logj_new

    def _flow_log_prob(self, x_dev: torch.Tensor) -> torch.Tensor:
        """prior_flow.log_prob(x) (smc/base.py:510); host (numpy-namespace) flows get a host copy."""
        dev_flow = None
        if hasattr(self.prior_flow, "device_coupling") and hasattr(self.engine, "coupling_logprob"):
            try:  # float32 coupling flow of a supported shape: fp32 MFMA kernel instead of the torch modules
                dev_flow = self.prior_flow.device_coupling(self.engine)
            except (ValueError, RuntimeError):  # unsupported dtype / shape: the flow's own torch modules evaluate it
                dev_flow = None
        if dev_flow is not None:
            return self.engine.coupling_logprob(x_dev if x_dev.is_contiguous() else x_dev.contiguous(), dev_flow)
        flow_xp = getattr(self.prior_flow, "xp", None)
        arg = x_dev if (flow_xp is None or is_torch_namespace(flow_xp)) else to_numpy(x_dev)
        return self._to_dev(self.prior_flow.log_prob(arg))

    # ---- config / checkpoint plumbing (samplers/base.py:93-276, minimal) -------------------
    def config_dict(self, include_sample_calls: str | bool = "last") -> dict:
        """samplers/base.py:93-141."""
        config = {"sampler_class": self.__class__.__name__}
        if include_sample_calls is not False:
            if include_sample_calls is True:
                include_sample_calls = "all"
            if not isinstance(include_sample_calls, str):
                raise ValueError("include_sample_calls must be a string ('last' or 'all') or False."
                                 f"Received: {include_sample_calls} of type {type(include_sample_calls)}")
            calls = self.__dict__.get("_call_log", {}).get(getattr(type(self).sample, "__qualname__", ""))
            if calls is None:
                return config
            if include_sample_calls.lower() == "last":
                config["sample_calls"] = {"args": calls["args"][-1] if calls["args"] else None,
                                          "kwargs": calls["kwargs"][-1] if calls["kwargs"] else None}
            elif include_sample_calls.lower() == "all":
                config["sample_calls"] = {"args": {str(i): v for i, v in enumerate(calls["args"])},
                                          "kwargs": {str(i): v for i, v in enumerate(calls["kwargs"])}}
            else:
                raise ValueError("Invalid value for include_sample_calls. Must be 'last', 'all', or False.")
        return config

    def _checkpoint_extra_state(self) -> dict:
        """samplers/base.py:150-152."""
        return {}

    def _restore_extra_state(self, state: dict) -> None:
        """samplers/base.py:154-156."""
        _ = state

    def build_checkpoint_state(self, samples, iteration: int | None = None, meta: dict | None = None,
                               include_sample_calls: str | bool = "last") -> dict:
        """samplers/base.py:158-178: same keys, same order."""
        state = {"sampler": self.__class__.__name__, "iteration": iteration, "samples": samples,
                 "config": self.config_dict(include_sample_calls=include_sample_calls),
                 "parameters": self.parameters, "meta": meta or {}}
        state.update(self._checkpoint_extra_state())
        return state

    def serialize_checkpoint(self, state: dict, protocol: int | None = None) -> bytes:
        """samplers/base.py:180-187."""
        return pickle.dumps(state, protocol=pickle.HIGHEST_PROTOCOL if protocol is None else int(protocol))

    def default_checkpoint_callback(self, state: dict) -> None:
        """samplers/base.py:189-192: keep the latest checkpoint (state + pickled bytes) on the sampler."""
        self._last_checkpoint_state = state
        self._last_checkpoint_bytes = self.serialize_checkpoint(state)

    def _rank_path(self, file_path) -> Path:
        """Sharded runs: every rank checkpoints its own shard into its own file (`name.rank<r>.ext`)."""
        file_path = Path(file_path)
        if not self.comm.sharded:
            return file_path
        return file_path.with_name(f"{file_path.stem}.rank{self.comm.rank}{file_path.suffix}")

    def default_file_checkpoint_callback(self, file_path: str | Path | None):
        """samplers/base.py:194-216: overwrite `/checkpoint/state` of an HDF5 file (needs h5py); additionally a `.pkl`
        path writes the same pickled bytes to a plain file (h5py is not part of every image)."""
        if file_path is None:
            return self.default_checkpoint_callback
        file_path = self._rank_path(file_path)
        lower = file_path.name.lower()
        if not lower.endswith((".h5", ".hdf5", ".pkl", ".pickle")):
            raise ValueError("Checkpoint file must be an HDF5 file (.h5 or .hdf5) or a pickle file (.pkl).")

        def _callback(state: dict) -> None:
            if lower.endswith((".h5", ".hdf5")):
                from ..io import open_h5

                with open_h5(file_path, "a") as h5_file:
                    self.save_checkpoint_to_hdf(state, h5_file, path="checkpoint", dsetname="state")
                self.default_checkpoint_callback(state)
            else:
                self.default_checkpoint_callback(state)
                with open(file_path, "wb") as fp:
                    fp.write(self._last_checkpoint_bytes)

        return _callback

    def save_checkpoint_to_hdf(self, state: dict, h5_file, path: str = "sampler_checkpoints", dsetname: str | None = None,
                               protocol: int | None = None) -> None:
        """samplers/base.py:218-236: the state as ONE pickled `S1` byte dataset `<path>/<dsetname>`; `h5_file` is an open
        h5py.File or anything with its group protocol."""
        from ..io import dump_state

        if dsetname is None:
            dsetname = f"iter_{state.get('iteration', 'unknown')}"
        dump_state(state, h5_file, path=path, dsetname=dsetname, protocol=protocol or pickle.HIGHEST_PROTOCOL)

    def load_checkpoint_from_file(self, file_path: str | Path, h5_path: str = "checkpoint", dsetname: str = "state") -> dict:
        """samplers/base.py:238-253."""
        file_path = Path(file_path)
        if file_path.name.lower().endswith((".h5", ".hdf5")):
            from ..io import load_state, open_h5

            with open_h5(file_path, "r") as h5_file:
                return load_state(h5_file, h5_path, dsetname)
        with open(file_path, "rb") as f:
            return pickle.loads(f.read())

    def restore_from_checkpoint(self, source):
        """samplers/base.py:255-276."""
        if isinstance(source, (str, Path)):
            p = Path(source)
            state = self.load_checkpoint_from_file(p if p.exists() else self._rank_path(p))
        elif isinstance(source, (bytes, bytearray)):
            state = pickle.loads(source)
        elif isinstance(source, dict):
            state = source
        else:
            raise TypeError("Unsupported checkpoint source type.")
        samples_saved = state.get("samples")
        if samples_saved is None:
            raise ValueError("Checkpoint missing samples.")
        self._restore_extra_state(state)
        return samples_saved, state

    @property
    def last_checkpoint_state(self):
        return self._last_checkpoint_state

    @property
    def last_checkpoint_bytes(self):
        return self._last_checkpoint_bytes


class MCMCSampler(Sampler):
    """samplers/mcmc.py:14-110."""

    def __init__(self, log_likelihood, log_prior, dims, prior_flow, xp, dtype=None, parameters=None,
                 preconditioning_transform=None, rng=None, engine=None, comm=None):
        super().__init__(log_likelihood, log_prior, dims, prior_flow, xp, dtype, parameters,
                         preconditioning_transform, engine=engine, comm=comm)
        self.rng = rng or np.random.default_rng()

    def draw_initial_samples(self, n_samples: int) -> Samples:
        """samplers/mcmc.py:49-110: draw from the proposal flow until n rows have finite log-prior and
        log-likelihood; a non-finite log_q is an error.  State stays on device; the finite-mask
        compaction is the asmc_compact_valid kernel."""
        e = self.engine
        n_drawn = 0
        parts = []
        while n_drawn < n_samples:
            x, log_q = self.prior_flow.sample_and_log_prob(n_samples)
            x = e.asarray(x, dtype=self.x_torch_dtype)
            log_q = self._to_dev(log_q)
            n_nan, n_inf = e.count_nonfinite(log_q)
            if n_nan or n_inf:
                raise ValueError(
                    "Proposal returned non-finite log probabilities. "
                    "aspire assumes the proposal is a valid, normalized "
                    "probability distribution and should therefore only "
                    "return samples with finite log probabilities.")
            lp, ll = self._eval_prior_likelihood(x, log_q)
            xv, llv, lpv, lqv = e.compact_valid(x, ll, lp, log_q)
            n_valid = xv.shape[0]
            if n_valid < x.shape[0]:
                logger.debug("Proposal returned %d invalid samples with non-finite log prior or log "
                             "likelihood. These samples will be discarded.", x.shape[0] - n_valid)
            if n_valid > 0:
                parts.append((xv, llv, lpv, lqv))
                n_drawn += n_valid
        if len(parts) == 1:
            xv, llv, lpv, lqv = parts[0]
        else:
            xv, llv, lpv, lqv = (torch.cat([p[i] for p in parts], dim=0) for i in range(4))
        if n_drawn > n_samples:
            xv, llv, lpv, lqv = (t[:n_samples].contiguous() for t in (xv, llv, lpv, lqv))
        out = Samples(x=xv, xp=torch, parameters=self.parameters)
        # set after construction (as the reference does, mcmc.py:82-87) so no IS weights are formed
        out.log_likelihood, out.log_prior, out.log_q = llv, lpv, lqv
        return out

    # ---- the un-fused pCN step loops ------------------------------------------------------------------------
    def _pcn_split_steps(self, z, ll, lp, lq, ref, st, densities, *, beta, seed, n_steps, target, n_global, gid0=0, step0=0,
                         logj=None, noise="f64", session=True, fused=None, on_step=None):
        """`n_steps` pCN / tpCN steps of the rows z in place, densities between a propose and an accept launch, step size and
        accept counts resident on the device (one read-back per chunk of 2048 steps).  While the engine grants one (`session`;
        d = 4, 8, 16, 32) the chain runs as a whitened-state session: the state stays coordinate-major on the device, a step is
        one mat-vec in the propose kernel and an LDS-free accept kernel.  Otherwise propose / accept on the row-major state.
        ref = (mu, L, Linv, nu); st["rho"]: the step size, updated; `densities(z', inverted=None)`: `_proposal_densities` with the
        sampler's rule for log q; `logj`: the carried log-Jacobian, which follows the accepted state inside the accept kernel;
        `fused` = (transform tables, premapped log q arguments): T^-1 (and log q) inside the session's propose kernel;
        `on_step(step, sess)`: the chain recorder (sess None: the rows are current).  Returns (accept counts per step - global
        under a count hook -, whether a session ran)."""
        e = self.engine
        mu, L, Linv, nu = ref
        counts, done, in_session = [], 0, False
        while done < n_steps:
            chunk = min(n_steps - done, MAX_CHUNK)
            sess = None
            if session and hasattr(e, "pcn_ysplit_begin"):
                sess = e.pcn_ysplit_begin(z, beta, mu, L, Linv, seed, gid0, st["rho"], target, True, nu, noise)
                session = sess is not None  # (refused: this width has no whitened-state kernels, the engine is not asked again)
                in_session = in_session or session
            if sess is None:
                e.pcn_split_begin(st["rho"])
            for t in range(chunk):
                step = step0 + done + t
                if sess is None:
                    z_prop, q0, q1 = e.pcn_propose(z, mu, L, Linv, 0.0, seed, gid0, step, nu=nu)
                    _, ll_new, lp_new, lq_new, logj_new = densities(z_prop)
                    e.pcn_accept(z, z_prop, ll, lp, lq, ll_new, lp_new, lq_new, q0, q1, beta, seed, gid0, step, logj_old=logj,
                                 logj_new=logj_new, want_count=False)
                    e.pcn_split_adapt(n_global, target, t, True)
                else:
                    if fused is not None:
                        _, ll_new, lp_new, lq_new, logj_new = densities(None, e.pcn_ysplit_propose_tr(sess, step, *fused))
                    else:
                        _, ll_new, lp_new, lq_new, logj_new = densities(e.pcn_ysplit_propose(sess, step))
                    e.pcn_ysplit_accept(sess, step, ll, lp, lq, ll_new, lp_new, lq_new, n_global, t, logj=logj, logj_new=logj_new)
                if on_step is not None:
                    on_step(step, sess)
            n_acc, _, st["rho"] = e.pcn_split_end(chunk) if sess is None else e.pcn_ysplit_end(sess, chunk)
            counts.append(n_acc)
            done += chunk
        return (np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64)), in_session

    def _pcn_round_trip_steps(self, z, ll, lp, lq, ref, st, densities, *, beta, seed, n_steps, target, n_global, gid0=0, step0=0,
                              logj=None):
        """The same steps with one host round trip each (engines without the split entry points; sharded runs without a count
        hook): the accept count comes back, the ranks add theirs, the host adapts the step size.  Returns the global counts."""
        e = self.engine
        mu, L, Linv, nu = ref
        counts = np.zeros(n_steps)
        for t in range(n_steps):
            z_prop, q0, q1 = e.pcn_propose(z, mu, L, Linv, st["rho"], seed, gid0, step0 + t, nu=nu)
            _, ll_new, lp_new, lq_new, logj_new = densities(z_prop)
            n_acc = e.pcn_accept(z, z_prop, ll, lp, lq, ll_new, lp_new, lq_new, q0, q1, beta, seed, gid0, step0 + t, logj_old=logj,
                                 logj_new=logj_new)
            counts[t] = float(self.comm.all_gather_f64(np.array([float(n_acc)])).sum())
            st["rho"] = pcn_adapt(st["rho"], counts[t] / n_global, target, t)
        return counts

    chain_checkpoint_path = "checkpoint"  # mcmc.py:17-23: where a chain checkpoint lies in its file
    chain_dataset_name = "mcmc_chain"

    def log_prob(self, z):
        """samplers/mcmc.py:112-126: the target of a chain in the preconditioned space, log L + log pi at x = T^-1(z) plus
        log|det dT^-1/dz|; NaN and +inf count as -inf, as in every accept kernel of this package."""
        e = self.engine
        x, logj = self.preconditioning_transform.inverse(z)
        x = e.asarray(x, dtype=self.x_torch_dtype)
        lp, ll = self._eval_prior_likelihood(x)
        r = ll + lp if logj is None else ll + lp + e.asarray(logj)
        r = torch.where(r < np.inf, r, torch.full_like(r, -np.inf)).reshape(-1)
        return r if is_torch_namespace(self.xp) else to_numpy(r)

    def default_mcmc_chain_file_checkpoint_callback(self, file_path):
        """samplers/mcmc.py:128-167: the chain as a native samples group `checkpoint/mcmc_chain` of an HDF5 file (replaced on
        every call), with `chain_shape`, `iteration`, `stage` and `sampler` as the group's attributes.  A `.pkl` path has no groups:
        the pickled state (samples included, `chain_shape` with them) is the file, as for every other sampler here."""
        if file_path is None:
            return self.default_checkpoint_callback
        plain = self.default_file_checkpoint_callback(file_path)  # (checks the extension first)
        path = self._rank_path(file_path)
        if not path.name.lower().endswith((".h5", ".hdf5")):
            return plain

        def _callback(state: dict) -> None:
            from ..io import open_h5

            samples = state.get("samples")
            if samples is None:
                raise ValueError("Checkpoint missing samples.")
            chain_path = f"{self.chain_checkpoint_path}/{self.chain_dataset_name}"
            with open_h5(path, "a") as h5_file:
                if chain_path in h5_file:
                    del h5_file[chain_path]
                samples.save(h5_file, path=chain_path, flat=False)
                attrs = h5_file[chain_path].attrs
                if getattr(samples, "chain_shape", None) is not None:
                    attrs["chain_shape"] = np.asarray(samples.chain_shape, dtype=int)
                if state.get("iteration") is not None:
                    attrs["iteration"] = int(state["iteration"])
                if state.get("meta", {}).get("stage") is not None:
                    attrs["stage"] = str(state["meta"]["stage"])
                if state.get("sampler") is not None:
                    attrs["sampler"] = str(state["sampler"])
            self.default_checkpoint_callback(state)

        return _callback

    def checkpoint_mcmc_chain(self, samples, iteration: int | None = None, checkpoint_callback=None,
                              checkpoint_every: int | None = None, checkpoint_file_path: str | None = None) -> None:
        """samplers/mcmc.py:169-191."""
        if checkpoint_every is not None and checkpoint_every <= 0:
            return
        if checkpoint_callback is None and checkpoint_file_path is not None:
            checkpoint_callback = self.default_mcmc_chain_file_checkpoint_callback(checkpoint_file_path)
        if checkpoint_callback is None:
            return
        checkpoint_callback(self.build_checkpoint_state(samples=samples, iteration=iteration, meta={"stage": "mcmc_chain"}))
