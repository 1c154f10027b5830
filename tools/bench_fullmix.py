"""Times asmc_fullmix_logpdf (k_fullmix, csrc/asmc_fullmix.hip), value only and with the gradient, at 1M x 32 fp64 for C = 1 and
C = 2 and at 1M x 128 for C = 2 (SHAPES=n:d:C,... overrides), with HIP events after warm-up.  Next to each, from the same
process: (i) the HBM floor of the pass - its bytes (x read once, the value written, the gradient written when asked for) over the
copy bandwidth measured here with a device-to-device copy of x - and (ii) GaussianMixture.__call__ (torch ops) on the same tensor,
plus that path's torch.autograd gradient for the gradient form.  Prints one JSON line per shape; OUT=<path> also writes them.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aspire_amd import GaussianMixture  # noqa: E402
from aspire_amd.engine import HipEngine  # noqa: E402


def event_us(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def target(d, C, seed=0):
    g = np.random.default_rng(seed)
    cov = np.zeros((C, d, d))
    for c in range(C):
        Q = np.linalg.qr(g.normal(size=(d, d)))[0]
        cov[c] = (Q * np.geomspace(0.1, 10.0, d)) @ Q.T
        cov[c] = 0.5 * (cov[c] + cov[c].T)
    return GaussianMixture(g.normal(size=(C, d)), cov)


def main():
    assert torch.cuda.is_available(), "bench_fullmix.py needs a HIP device"
    shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", "1000000:32:1,1000000:32:2,1000000:128:2").split(",")]
    reps, warm = int(os.environ.get("REPS", 20)), int(os.environ.get("WARMUP", 3))
    eng = HipEngine(0, n_max=max(s[0] for s in shapes), d_max=128)
    lines = []
    for n, d, C in shapes:
        t = target(d, C)
        tab = t.device_tables(eng)
        g = torch.Generator(eng.device).manual_seed(d)
        x = (1.5 * torch.randn((n, d), device=eng.device, dtype=torch.float64, generator=g)).contiguous()
        y = torch.empty_like(x)
        for _ in range(warm):
            eng.fullmix_logpdf(x, tab)
            eng.fullmix_logpdf(x, tab, want_grad=True)
            y.copy_(x)
        torch.cuda.synchronize()
        t_val = event_us(lambda: eng.fullmix_logpdf(x, tab), reps)
        t_grad = event_us(lambda: eng.fullmix_logpdf(x, tab, want_grad=True), reps)
        t_copy = event_us(lambda: y.copy_(x), reps)
        bw = 2 * x.numel() * 8 / (t_copy * 1e-6)  # bytes read + written per second
        floor_val = (x.numel() * 8 + n * 8) / bw * 1e6
        floor_grad = (2 * x.numel() * 8 + n * 8) / bw * 1e6

        def torch_grad():
            leaf = x.detach().requires_grad_(True)
            torch.autograd.grad(t(leaf).sum(), leaf)

        treps = max(2, reps // 5)
        t(x)
        torch_grad()
        torch.cuda.synchronize()
        t_call = event_us(lambda: t(x), treps)
        t_call_grad = event_us(torch_grad, treps)
        fma_row = C * d * (d + 1) // 2
        lines.append(dict(
            shape=f"{n}x{d} fp64 C={C}", kernel_value_us=round(t_val, 1), kernel_value_grad_us=round(t_grad, 1),
            copy_bandwidth_TBps=round(bw / 1e12, 3), hbm_floor_value_us=round(floor_val, 1), hbm_floor_value_grad_us=round(floor_grad, 1),
            torch_call_us=round(t_call, 1), torch_call_plus_autograd_us=round(t_call_grad, 1),
            speedup_value=round(t_call / t_val, 2), speedup_value_grad=round(t_call_grad / t_grad, 2),
            triangle_fma_per_row=fma_row, value_TFLOPs=round(2 * fma_row * n / (t_val * 1e-6) / 1e12, 2), reps=reps))
        print(json.dumps(lines[-1]), flush=True)
    out = os.environ.get("OUT")
    if out:
        with open(out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
