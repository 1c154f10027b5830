"""Micro-driver of the chain diagnostics (csrc/asmc_diag.hip) on a synthetic AR(1) chain [S, W, d] built on the
device: the lag-block kernel for both block sizes (kb = 16, 32) at lag 0 - where the leading and the trailing stream are the same
rows - and at lag 2 kb, the moments pass, `chain_autocorr` and `chain_rhat` end to end, and, as the yardstick of this data layout,
the recorder's copy kernel (k_chain_rows) on one slot of the same chain.  Every figure is the median of REPS timed repeats after
a warm-up, by HIP events; rates count 2 S W d s bytes per lag block (s: bytes per element) and 2 W d s per copied slot.
Env: S, W, D, DTYPE=f64|f32, PHI (AR(1) coefficient), REPS, OUT (a JSON file beside the printed lines)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd._lib import check  # noqa: E402
from aspire_amd.engine import HipEngine, _dptr  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(v, 4) for v in ms]


def main():
    S, W, d = int(os.environ.get("S", 200)), int(os.environ.get("W", 1 << 20)), int(os.environ.get("D", 32))
    dt = torch.float64 if os.environ.get("DTYPE", "f64") == "f64" else torch.float32
    phi, reps = float(os.environ.get("PHI", 0.8)), int(os.environ.get("REPS", 5))
    elem = 8 if dt == torch.float64 else 4
    eng = HipEngine(0, n_max=1 << 12, d_max=d)
    need = S * W * d * elem + 6 * W * d * 8
    free = eng.free_memory()
    if need > 0.9 * free:
        raise SystemExit(f"the chain and its scratch need {need} bytes, {free} are free: lower S or W")
    chain = eng.chain_alloc(S, W, d, dt)
    g = torch.Generator(device=eng.device).manual_seed(1)
    x = torch.randn((W, d), dtype=dt, device=eng.device, generator=g)
    for t in range(S):  # the recorder writes the slots, as a sampler would
        x = phi * x + (1.0 - phi * phi) ** 0.5 * torch.randn((W, d), dtype=dt, device=eng.device, generator=g)
        eng.chain_record(chain, t, x=x, ll=chain.ll[0], lp=chain.lp[0])
    torch.cuda.synchronize()
    out = dict(S=S, W=W, d=d, dtype=os.environ.get("DTYPE", "f64"), phi=phi, reps=reps, chain_bytes=S * W * d * elem)
    ms, all_ms = timed(lambda: eng.chain_record(chain, S - 1, x=x, ll=chain.ll[0], lp=chain.lp[0]), reps)
    out["copy_slot"] = dict(ms=ms, all_ms=all_ms, bytes=2 * W * d * elem + 32 * W, tb_per_s=(2 * W * d * elem + 32 * W) / ms / 1e9)
    xdt = eng._xdt(chain.x)
    mom = eng.empty((2, W * d))
    moments = lambda: check(eng.lib.asmc_chain_series_moments(eng._ctx, xdt, _dptr(chain.x), S, W, d, d, 0, _dptr(mom[0]),  # noqa: E731
                                                              _dptr(mom[1]), eng._stream))
    ms, all_ms = timed(moments, reps)
    out["moments"] = dict(ms=ms, all_ms=all_ms, bytes=2 * S * W * d * elem, tb_per_s=2 * S * W * d * elem / ms / 1e9)
    for kb in (16, 32):
        part = eng.empty((int(eng.lib.asmc_chain_acf_blocks(W, d)), d, kb))
        for k0 in (0, 2 * kb):
            if k0 >= S:
                continue
            fn = lambda: check(eng.lib.asmc_chain_acf_block(eng._ctx, xdt, _dptr(chain.x), S, W, d, d, k0, kb, _dptr(mom[0]),  # noqa: E731
                                                            _dptr(mom[1]), _dptr(part), eng._stream))
            ms, all_ms = timed(fn, reps)
            moved = 2 * (S - k0) * W * d * elem  # the leading stream stops k0 steps early, the trailing one starts k0 late
            out[f"acf_block_kb{kb}_k{k0}"] = dict(ms=ms, all_ms=all_ms, bytes_model=2 * S * W * d * elem, bytes_read=moved,
                                                  tb_per_s_model=2 * S * W * d * elem / ms / 1e9, tb_per_s_read=moved / ms / 1e9,
                                                  ms_per_lag=ms / kb)
        del part
    for kb in (16, 32):
        res = {}
        ms, all_ms = timed(lambda: res.update(r=eng.chain_autocorr(chain.x, kb=kb)), max(2, reps // 2))
        tau, window = res["r"]
        out[f"chain_autocorr_kb{kb}"] = dict(ms=ms, all_ms=all_ms, lag_blocks=int(window.max()) // kb + 1, tau=[round(float(v), 3) for v in tau[:4]],
                                             window_max=int(window.max()))
    ms, all_ms = timed(lambda: eng.chain_rhat(chain.x), max(2, reps // 2))
    out["chain_rhat"] = dict(ms=ms, all_ms=all_ms)
    for k, v in out.items():
        print(k, json.dumps(v) if isinstance(v, dict) else v)
    if os.environ.get("OUT"):
        os.makedirs(os.path.dirname(os.path.abspath(os.environ["OUT"])), exist_ok=True)
        with open(os.environ["OUT"], "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
