#!/usr/bin/env python3
"""Result census of the weight, temperature-search and importance-step kernels (csrc/asmc_weights.hip, asmc_search.hip,
asmc_is_weights.hip): what each call launches and every bit it returns, recorded once and compared ever after
(tests/test_gpu_weights_census.py).

    python3 tools/record_weights_census.py            # writes tests/golden/weights_census.json (needs the GPU)

Run it on the build whose behaviour is the reference - the commit BEFORE a refactor of these files, never the refactored tree -
and commit the file.  Per case it holds profile_report()'s label -> launch count, profile_variants()'s symbol -> count, SHA-256
digests of every device output and the host result vectors verbatim (repr of the doubles).  Every case is recorded twice and
the two recordings must agree: these kernels reduce in a fixed order.  The file also holds the device's compute-unit count:
grids, and with them the order of the additions, depend on it.

Populations: `synth` (smooth) and `neginf20` (a fifth of the rows with zero likelihood) of tests/weights_ref.py, its seeds."""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "weights_census.json")
KINDS = ("synth", "neginf20")
TARGET, TOL = 0.5, 1e-6
SHARD_N = 9001


def _cases():
    out = []
    for kind in KINDS:
        for n in (1, 511, 513, 30011):  # 30011: a ragged last pair of the two-particle trip
            out.append(dict(name=f"find_beta-{kind}-n{n}", call="find_beta", kind=kind, n=n, beta0=0.0))
        out.append(dict(name=f"find_beta-{kind}-n30011-beta0", call="find_beta", kind=kind, n=30011, beta0=0.2))
        out.append(dict(name=f"find_beta-{kind}-n513-nan", call="find_beta", kind=kind, n=513, beta0=0.0, nan=True))
        # resident path, multi-block and ragged; then one chunk per compute unit exactly (resident) and one particle more (streaming)
        for n in (4097, 200000, "cu", "cu+1"):
            out.append(dict(name=f"importance_step-{kind}-n{n}", call="importance_step", kind=kind, n=n, beta0=0.0))
        for world, layout in ((2, "uneq"), (3, "one")):
            for folded in (True, False):
                out.append(dict(name=f"shard-{kind}-w{world}-{layout}-{'folded' if folded else 'decide'}", call="shard", kind=kind,
                                n=SHARD_N, beta0=0.013, world=world, layout=layout, folded=folded))
        for K in (1, 5, 17):
            out.append(dict(name=f"weights_stats-{kind}-K{K}", call="stats", kind=kind, n=30011, beta0=0.0, K=K))
        out.append(dict(name=f"weights_m2_lse-{kind}", call="m2_lse", kind=kind, n=30011, beta0=0.0))
        out.append(dict(name=f"log_weights-{kind}", call="log_weights", kind=kind, n=30011, beta0=0.0))
    return out


CASES = _cases()


def num_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def make_engines():
    """[0]: the engine of every single-rank case (room for one chunk per compute unit and a particle more); [1], [2]: further
    ranks of the sharded cases, emulated on the same device."""
    from aspire_amd.engine import HipEngine

    return [HipEngine(0, n_max=4096 * num_cu() + 4096, d_max=1)] + [HipEngine(0, n_max=1 << 15, d_max=1) for _ in range(2)]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _reprs(a):
    return [repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def _size(n):
    return 4096 * num_cu() + (1 if n == "cu+1" else 0) if isinstance(n, str) else n


_POP = {}


def _population(c):
    import weights_ref as W

    n = _size(c["n"])
    key = (c["kind"], n, bool(c.get("nan")))
    if key not in _POP:
        ll, lp, lq = W.population(c["kind"], n)
        if c.get("nan"):
            lp[n // 2] = np.nan
        _POP.clear()  # (one population at a time: the largest is 25 MB)
        _POP[key] = (ll, lp, lq)
    return _POP[key]


def _dev(eng, *arrs):
    return tuple(eng.asarray(np.ascontiguousarray(a, dtype=np.float64)) for a in arrs)


def _cuts(n, world, layout):
    assert (world, layout) in ((2, "uneq"), (3, "one"))
    return [0, n // 3, n] if world == 2 else [0, 1, 1 + (n - 1) // 3, n]  # (world 3: a rank of one particle in front)


def _betas(K, b0):
    return b0 + (1.0 - b0) * (np.arange(1, K + 1) / K) ** 2


def _run(engines, c):
    """The case's calls; returns (host result vectors, device outputs)."""
    import torch

    from aspire_amd import smc_math
    from aspire_amd.engine import _dptr, _f64p, check

    eng = engines[0]
    ll, lp, lq = _population(c)
    n, b0 = len(ll), c["beta0"]
    host, devs = {}, {}
    if c["call"] == "shard":
        world, cuts = c["world"], _cuts(n, c["world"], c["layout"])
        ranks = engines[:world]
        parts = [_dev(e, ll[cuts[r]:cuts[r + 1]], lp[cuts[r]:cuts[r + 1]], lq[cuts[r]:cuts[r + 1]]) for r, e in enumerate(ranks)]
        recs = [e.empty(40) for e in ranks]  # (not digested: a record's last six entries are never written)
        rounds = max(1, math.ceil(math.log2((1.0 - b0) / TOL) / 4 - 1e-9)) + 2
        allrec = None
        for e in ranks:
            e.profile(True)
        for rnd in range(rounds):
            for e, p, rec in zip(ranks, parts, recs):
                if c["folded"]:
                    e.find_beta_shard_round(*p, b0, TARGET, TOL, world, n, rnd, allrec, rec)
                else:
                    e.find_beta_shard_reduce(*p, b0, rnd, rec)
            allrec = torch.cat(recs).contiguous()
            if not c["folded"]:
                for e in ranks:
                    e.find_beta_shard_decide(allrec, world, n, b0, TARGET, TOL, rnd)
        outs = [e.empty(2) for e in ranks]
        for e, p, o in zip(ranks, parts, outs):
            if c["folded"]:
                e.weights_m2_lse_shard(*p, o, allrec, world, n, b0, TARGET, TOL, rounds)
            else:
                e.weights_m2_lse_shard(*p, o)
        pairs = torch.cat(outs).contiguous()
        devs["pairs"] = pairs
        for r, (e, p) in enumerate(zip(ranks, parts)):
            state = e.empty(40 + 4 * world)
            state[40:40 + 2 * world] = pairs
            state[40 + 2 * world:] = 0.0
            w, carry, tiles = e.normalized_weights_shard(*p, pairs, world, r, r / world, state)
            out = np.zeros(13 + 4 * world)
            check(e.lib.asmc_shard_step_result(e._ctx, _dptr(state), world, _f64p(out), e._stream), "asmc_shard_step_result")
            host[f"result{r}"] = _reprs(out)
            devs.update({f"w{r}": w, f"carry{r}": carry, f"tiles{r}": tiles, f"state{r}": state[:40]})
        return host, devs, ranks
    d = _dev(eng, ll, lp, lq)
    torch.cuda.synchronize()
    eng.profile(True)
    if c["call"] == "find_beta":
        out = np.zeros(13)
        check(eng.lib.asmc_find_beta(eng._ctx, n, *map(_dptr, d), b0, TARGET, TOL, _f64p(out), eng._stream), "asmc_find_beta")
        host["result"] = _reprs(out)
    elif c["call"] == "importance_step":
        st4 = smc_math.pcg64_state(np.random.default_rng(1))
        idx = eng.importance_step(*d, b0, TARGET, TOL, st4, min(n, 64))
        # the (ll, lp, lq, 0) records the kernel packed on its way: a gather of exactly these arrays reads them
        x = d[0].reshape(n, 1)
        every = torch.arange(n, dtype=torch.int64, device=eng.device)
        _, gl, gp, gq = eng.gather(every, x, *d)
        out = np.zeros(16)
        check(eng.lib.asmc_importance_result(eng._ctx, _f64p(out), eng._stream), "asmc_importance_result")
        host["result"] = _reprs(out)
        devs.update(w=eng._is_bufs["w"], cdf=eng._is_bufs["cdf"], idx=idx, tiles=eng.importance_tile_sums(n), rec_ll=gl, rec_lp=gp,
                    rec_lq=gq)
    elif c["call"] == "stats":
        host["result"] = _reprs(eng.weights_stats(*d, b0, _betas(c["K"], b0)))
    elif c["call"] == "m2_lse":
        m, S1 = eng.weights_stats(*d, b0, [0.3])[0][:2]
        shift = float((np.float64(m) + np.log(np.float64(S1))) - np.float64(math.log(n)))
        host["stats"] = _reprs([m, S1])
        host["result"] = _reprs(eng.weights_m2_lse(*d, b0, 0.3, float(m), float(S1) / n, shift, float(m) + shift))
        o = eng.empty(2)
        eng.weights_m2_lse_dev(*d, b0, 0.3, float(m), float(S1) / n, shift, float(m) + shift, o)
        devs["dev"] = o
    elif c["call"] == "log_weights":
        devs["lw"] = eng.log_weights(*d, b0, 0.3, 0.125)
        devs["w"] = eng.normalized_weights(*d, b0, 0.3, 0.125, 1.5)
    return host, devs, [eng]


def run_case(engines, c):
    """One case: its census, host results and digests (the layout of the golden file's entries)."""
    import torch

    report, variants = {}, {}
    try:
        host, devs, used = _run(engines, c)
        for e in used:
            for k, v in e.profile_report().items():
                report[k] = report.get(k, 0) + v[0]
            for k, v in e.profile_variants().items():
                variants[k] = variants.get(k, 0) + v
    finally:
        for e in engines:
            e.profile(False)
    torch.cuda.synchronize()
    return {"report": report, "variants": variants, "host": host, "digests": {k: _sha(v) for k, v in devs.items()}}


def main():
    engines = make_engines()
    out = {"num_cu": num_cu(), "cases": {}}
    for c in CASES:
        first, second = run_case(engines, c), run_case(engines, c)
        assert first == second, (c["name"], first, second)
        out["cases"][c["name"]] = first
        print(c["name"], first["report"], first["host"].get("result", "")[:3], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(out['cases'])} cases on {out['num_cu']} compute units")


if __name__ == "__main__":
    main()
