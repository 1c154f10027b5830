#!/usr/bin/env python3
"""Launch census of the pCN mutation drivers: what each dispatch path of `asmc_pcn_mutate_flow` / `asmc_pcn_mutate` launches and
what it returns, recorded once and compared ever after (tests/test_gpu_mutation_census.py).

    python3 tools/record_mutation_census.py            # writes tests/golden/mutation_census.json (needs the GPU)

Run it on the build whose behaviour is the reference - the commit BEFORE a refactor of the drivers - and commit the file.  Per case
it holds profile_report()'s label -> launch count, profile_variants()'s symbol -> count, SHA-256 digests of x, ll, lp, lq (and of a
chain target's recorded slots), the returned accept counts, the step-size history and the final rho.  Every case is run twice:
a case whose digests differ between the two recordings keeps its census and loses its digests (listed under "unstable").  The
error table lists single-fault calls of asmc_pcn_mutate_flow with the return code recorded; the test adds that nothing was
launched and that x stayed untouched.

n = 193: three full 64-row tiles plus one row, twelve 16-particle groups plus one particle.  5 steps, adaptation on."""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "mutation_census.json")
N, STEPS, STEP0, BETA, RHO, SEED, GID0 = 193, 5, 7, 0.4, 0.3, 4242, 17
COUPLING, MAF = "coupling", "maf"


def _flow_case(name, d, kind=COUPLING, hidden=64, layers=3, env=None, nu=0.0, deferred=False, dtypes=("f64", "f32")):
    return [dict(name=f"{name}-{T}", call="flow", d=d, T=T, kind=kind, hidden=hidden, layers=layers, env=env, nu=nu,
                 deferred=deferred, steps=STEPS) for T in dtypes]


def _mutate_case(name, d, steps=STEPS, env=None, stride=0):
    return [dict(name=f"{name}-f64", call="mutate", d=d, T="f64", env=env, nu=0.0, steps=steps, stride=stride)]


# One case per path of the dispatch (csrc/asmc_pcn_drive.hip).  The fall-back after the padded one-kernel step answers
# UNSUPPORTED has no case: the pre-check admits the shape only where the step takes it, and what is left (no room for the
# coordinate-major scratch, a state of 4 GiB or more) is out of a test's reach.
CASES = sum([
    _flow_case("fused-d32", 32),
    _flow_case("fused-padded-d6", 6),
    _flow_case("regsplit-soa-d32", 32, layers=6),  # six width-64 layers do not fit the one-kernel step's LDS
    _flow_case("regsplit-aos-d32", 32, env="ASMC_PCN_AOS"),
    _flow_case("xstate-d32", 32, env="ASMC_PCN_XSTATE"),
    _flow_case("xstate-nopad-d20", 20, env="ASMC_PCN_NOPAD"),
    _flow_case("flow16-d64", 64, layers=2),
    _flow_case("flow16-padded-d40", 40, layers=2),
    _flow_case("flow16-maf128-d16", 16, kind=MAF, hidden=128, layers=2),
    _flow_case("fused-d32-nu", 32, nu=5.5, dtypes=("f64",)),
    _flow_case("regsplit-soa-d32-nu", 32, layers=6, nu=5.5, dtypes=("f64",)),
    _flow_case("xstate-d32-nu", 32, env="ASMC_PCN_XSTATE", nu=5.5, dtypes=("f64",)),
    _flow_case("flow16-d64-nu", 64, layers=2, nu=5.5, dtypes=("f64",)),
    _flow_case("fused-d32-deferred", 32, deferred=True),
    _flow_case("fused-padded-d6-deferred", 6, deferred=True),
    _mutate_case("mutate-mm-d64", 64),
    _mutate_case("mutate-whitened-d8", 8),
    _mutate_case("mutate-whitened-aos-d8", 8, env="ASMC_PCN_AOS"),
    _mutate_case("mutate-xstate-3steps-d8", 8, steps=3),
    _mutate_case("mutate-padded-d6", 6),
    _mutate_case("mutate-chain-stride2-d8", 8, stride=2),
], [])

# single-fault calls of asmc_pcn_mutate_flow on the fused-d32-f64 inputs
ERRORS = ["rho-0", "rho-1.5", "nu-0.5", "n_steps-0", "n_steps-2049", "n-above-n_max", "work-one-byte-short", "flow-dims-differ",
          "chain-target-set"]


def make_engine():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=1 << 12, d_max=128)


@contextlib.contextmanager
def _env(name):
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        if name:
            del os.environ[name]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


_FLOWS = {}


def _flow(eng, kind, d, layers, hidden):
    key = (id(eng), kind, d, layers, hidden)
    if key not in _FLOWS:
        from conftest import random_coupling_flow, random_maf_flow

        flow = (random_coupling_flow if kind == COUPLING else random_maf_flow)(d, layers, hidden, seed=5 + d + layers)
        _FLOWS[key] = (flow, flow.device_coupling(eng))
    return _FLOWS[key]


def _inputs(eng, d, T, n=N):
    """state, reference Gaussian and single-Gaussian targets of a case: a function of (d, T, n) alone"""
    import torch

    g = np.random.default_rng(1000 + d)
    x = torch.as_tensor(0.9 * g.normal(size=(n, d))).to(torch.float64 if T == "f64" else torch.float32).to(eng.device).contiguous()
    a = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.tril(np.linalg.cholesky(0.8 * (np.eye(d) + 0.2 * a @ a.T)))
    mu, Linv = 0.05 * g.normal(size=d), np.tril(np.linalg.inv(L))
    t_ll = eng.make_mixture([0.0], 0.1 * g.normal(size=(1, d)), 0.7 + 0.6 * g.random(size=(1, d)))
    t_lp = eng.make_mixture([0.0], np.zeros((1, d)), np.ones((1, d)))
    t_lq = eng.make_mixture([0.0], 0.05 * g.normal(size=(1, d)), 0.5 + 0.2 * g.random(size=(1, d)))
    return x, eng.asarray(mu), eng.asarray(L), eng.asarray(Linv), t_ll, t_lp, t_lq


def run_case(eng, c):
    """One case on `eng`: its census, results and digests (the layout of the golden file's entries)."""
    import torch

    x, mu, L, Linv, t_ll, t_lp, t_lq = _inputs(eng, c["d"], c["T"])
    ll, lp = eng.mixture_logpdf(x, t_ll), eng.mixture_logpdf(x, t_lp)
    chain = None
    if c["nu"] > 0:
        # the context keeps the scale variates it drew last (keyed by seed, step range ...): another key's draw in front, so that the
        # case launches its own k_gamma_draw whatever ran before it
        eng.pcn_propose(x, mu, L, Linv, RHO, SEED + 1, GID0, STEP0, nu=c["nu"])
    with _env(c["env"]):
        if c["call"] == "flow":
            dev = _flow(eng, c["kind"], c["d"], c["layers"], c["hidden"])[1]
            lq = eng.coupling_logprob(x, dev)
            args = (x, ll, lp, lq, BETA, mu, L, Linv, t_ll, t_lp, dev, SEED, GID0, RHO, c["steps"], STEP0, 0.234, True, "f64", c["nu"])
            torch.cuda.synchronize()
            eng.profile(True)
            if c["deferred"]:
                handle = eng.pcn_mutate_flow_enqueue(*args)
                n_acc, rho_hist, rho = eng.pcn_mutate_flow_result(handle)
            else:
                n_acc, rho_hist, rho = eng.pcn_mutate_flow(*args)
        else:
            lq = eng.mixture_logpdf(x, t_lq)
            if c["stride"]:
                chain = eng.chain_alloc(c["steps"] // c["stride"], N, c["d"])
                for t in (chain.x, chain.ll, chain.lp):
                    t.zero_()
                eng.chain_set(chain, 0, c["stride"])
            torch.cuda.synchronize()
            eng.profile(True)
            try:
                n_acc, rho_hist, rho = eng.pcn_mutate(x, ll, lp, lq, BETA, mu, L, Linv, t_ll, t_lp, t_lq, SEED, GID0, RHO, c["steps"],
                                                      STEP0, 0.234, True, "f64", c["nu"])
            finally:
                if chain is not None:
                    eng.chain_clear()
        report = {k: v[0] for k, v in eng.profile_report().items()}
        variants = eng.profile_variants()
        eng.profile(False)
    torch.cuda.synchronize()
    digests = {"x": _sha(x), "ll": _sha(ll), "lp": _sha(lp), "lq": _sha(lq)}
    if chain is not None:
        digests.update({"chain_x": _sha(chain.x), "chain_ll": _sha(chain.ll), "chain_lp": _sha(chain.lp)})
    return {"report": report, "variants": variants, "n_accept": [int(v) for v in n_acc], "rho_hist": [float(v) for v in rho_hist],
            "rho": float(rho), "digests": digests}


def run_error(eng, name):
    """One single-fault call of asmc_pcn_mutate_flow: (return code, launches the profile saw, x untouched)."""
    import torch

    from aspire_amd import _lib

    n = eng.n_max + 1 if name == "n-above-n_max" else N
    d = 32
    x, mu, L, Linv, t_ll, t_lp, _ = _inputs(eng, d, "f64", n)
    dev = _flow(eng, COUPLING, 30 if name == "flow-dims-differ" else d, 3, 64)[1]
    ll, lp, lq = eng.full(n, -1.0), eng.full(n, -2.0), eng.full(n, -3.0)
    x0 = x.clone()
    rho = {"rho-0": 0.0, "rho-1.5": 1.5}.get(name, RHO)
    nu = 0.5 if name == "nu-0.5" else 0.0
    steps = {"n_steps-0": 0, "n_steps-2049": 2049}.get(name, STEPS)
    prm = _lib.AsmcPcnParams(d, _lib.ASMC_F64, BETA, mu.data_ptr(), L.data_ptr(), Linv.data_ptr(), t_ll.c_struct(), t_lp.c_struct(),
                             t_lp.c_struct(), SEED, GID0, 0.234, 1, 0, nu)
    nbytes = int(eng.lib.asmc_pcn_flow_work_bytes(n, d, _lib.ASMC_F64))
    work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
    cs = dev.c_struct()
    n_acc = np.zeros(max(steps, 1), dtype=np.int64)
    rho_hist = np.zeros(max(steps, 1))
    rho_io = ctypes.c_double(rho)
    chain = None
    if name == "chain-target-set":
        chain = eng.chain_alloc(STEPS, n, d)
        eng.chain_set(chain, 0, 1)
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        rc = eng.lib.asmc_pcn_mutate_flow(eng._ctx, n, x.data_ptr(), ll.data_ptr(), lp.data_ptr(), lq.data_ptr(), ctypes.byref(prm),
                                          ctypes.byref(cs), work.data_ptr(), nbytes - (name == "work-one-byte-short"), steps, STEP0,
                                          ctypes.byref(rho_io), n_acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          rho_hist.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), eng._stream)
    finally:
        if chain is not None:
            eng.chain_clear()
    launched = {k: v[0] for k, v in eng.profile_report().items()}
    eng.profile(False)
    torch.cuda.synchronize()
    return {"rc": int(rc), "launched": launched, "x_untouched": bool(torch.equal(x, x0))}


def main():
    eng = make_engine()
    out = {"n": N, "steps": STEPS, "cases": {}, "errors": {}, "unstable": []}
    for c in CASES:
        first, second = run_case(eng, c), run_case(eng, c)
        for key in ("report", "variants", "n_accept"):
            assert first[key] == second[key], (c["name"], key, first[key], second[key])
        if first["digests"] != second["digests"] or first["rho_hist"] != second["rho_hist"]:
            out["unstable"].append(c["name"])
            del first["digests"]
        out["cases"][c["name"]] = first
        print(c["name"], first["report"], first["n_accept"], flush=True)
    for name in ERRORS:
        r = run_error(eng, name)
        print(name, r, flush=True)
        out["errors"][name] = {"rc": r["rc"]}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(out['cases'])} cases, {len(out['errors'])} error calls, unstable: {out['unstable']}")


if __name__ == "__main__":
    main()
