"""Times the neural-spline-flow kernels (k_nsf_logprob, k_nsf_sample) at N x D, T transforms, hidden width W (default
1M x 32, T = 3, W = 64) with HIP events after warm-up and, in the same process, `NSFFlow.log_prob` of the fp32 torch modules
on the same GPU: what an NSF proposal costs per mutation step without the kernels.  Prints one JSON line; OUT=<path> also writes
it to a file.

Derived figures come from the shapes, not from counters: the three split-fp16 products of every MAC of the three dense layers
(flop per particle and pass), and the weight stream every workgroup pulls through LDS once per round of 8 waves x G groups x 16
particles.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nsf_ref  # noqa: E402

from aspire_amd.engine import HipEngine  # noqa: E402

PEAK_F16_FLOPS = 2.5e15  # dense fp16 MFMA peak of the MI355X (datasheet)
G_LOGPROB = 2            # csrc/asmc_nsf.hip NSF_G_LOGPROB


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    assert torch.cuda.is_available(), "bench_nsf.py needs a HIP device"
    n, d = int(os.environ.get("N", 1_000_000)), int(os.environ.get("D", 32))
    T, w = int(os.environ.get("T", 3)), int(os.environ.get("W", 64))
    reps, warm = int(os.environ.get("REPS", 20)), int(os.environ.get("WARMUP", 3))
    eng = HipEngine(0, n_max=n, d_max=32)
    flow = nsf_ref.random_nsf_flow(d, T, w, seed=3, scale=0.3)
    dev = flow.device_coupling(eng)
    g = torch.Generator(eng.device).manual_seed(d)
    x = (torch.randn((n, d), device=eng.device, dtype=torch.float64, generator=g) * 1.5 * flow.scale.double().to(eng.device)
         + flow.loc.double().to(eng.device)).contiguous()
    on_gpu = flow.to(eng.device)  # (the device copy is packed already: `to` moves the torch modules only)

    for _ in range(warm):
        eng.coupling_logprob(x, dev)
        eng.coupling_sample(n, torch.float64, dev, 1, 0, 1)
    torch.cuda.synchronize()
    eng.profile(True)
    for i in range(reps):
        eng.coupling_logprob(x, dev)
    for i in range(max(1, reps // 4)):
        eng.coupling_sample(n, torch.float64, dev, 1, 0, 2 + i)
    rep = eng.profile_report()
    eng.profile(False)
    t_logprob, t_sample = rep["k_nsf_logprob"][1], rep["k_nsf_sample"][1]

    # the torch modules in chunks that fit the d (3 K - 1) parameters per row in memory (0.75 GB per 64k rows and transform)
    chunk = int(os.environ.get("CHUNK", 1 << 16))
    xf = x.float()

    def module_pass():
        for i in range(0, n, chunk):
            on_gpu.log_prob(xf[i: i + chunk])

    for _ in range(2):
        module_pass()
    t_module = event_ms(module_pass, max(2, reps // 5))

    ncg = 1 if d <= 16 else 2
    macs = T * (w * 32 + w * w + ncg * 23 * 16 * w)  # per particle and pass, padded shapes as the kernels run them
    flop = 2 * 3 * macs
    words = T * (w // 16 * 512 + (w // 16 + ncg * 23) * (w // 32) * 512)
    rounds = -(-n // (8 * G_LOGPROB * 16))
    ref = on_gpu.log_prob_f64(x[:4096]).cpu().numpy()
    err = np.abs(eng.coupling_logprob(x[:4096].contiguous(), dev).cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)
    out = dict(n=n, d=d, transforms=T, hidden=w, k_nsf_logprob_ms=t_logprob, k_nsf_sample_ms=t_sample, module_log_prob_ms=t_module,
               module_over_kernel=t_module / t_logprob, flop_per_particle=flop, split_fp16_mfma_fraction=flop * n / (t_logprob * 1e-3) / PEAK_F16_FLOPS,
               weight_stream_bytes_per_pass=4 * words * rounds, kernel_max_rel_vs_fp64=float(err.max()))
    line = json.dumps(out)
    print(line)
    if os.environ.get("OUT"):
        os.makedirs(os.path.dirname(os.path.abspath(os.environ["OUT"])), exist_ok=True)
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
