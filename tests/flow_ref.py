"""What tests/test_gpu_flow_kernels.py compares the stand-alone flow kernels of csrc/asmc_flow.hip and csrc/asmc_flow16.hip with,
usable without a device (tests/test_flow_ref.py runs all of it on the CPU).  A test helper: the product never imports it.

  pools      a random flow (the conftest builders; `wide`: standardisation scales log-uniform in [1e-3, 1e3],
             autoregressive flows [1e-2, 1e3]) and >= 4096 input rows
             loc + 1.2 scale N(0, I), rounded to the row type first
  judge      the same fp32 parameters evaluated in fp64 by the torch modules (log q), `draw_ref` for the inverse direction
  yardstick  the fp32 torch module's own error against the judge on the pool's rows, |a - ref| / max(|ref|, 1): maximum and 99th
             percentile.  Computed with the CPU modules, so it is the same number wherever it is computed.  A case that runs fewer
             rows than the pool still uses the POOL's yardstick.
  latent     the counter-based draw the kernels make, from the oracle's fast-noise restatement: coordinate j of particle gid is
             element j % 4 of quad j / 4 (oracle.pcn_noise(seed, gid, draw_id, d, "f32"))
  rounds     rows one grid-stride round of each kernel covers, restated from the launch functions' arithmetic
  BUGS       deliberately wrong restatements of the latent: the comparison of the device tests must catch each

Tolerances; none is taken from a device's output:
  density    max error <= max(1e-6, 4 x yardstick max), p99 error <= max(1e-6, 4 x yardstick p99).  1e-6 relative is the bar the older
             flow tests assert; 4 = test_gpu_nsf.MARGIN (split-fp16 operands carry 22 mantissa bits against fp32's 24).  The
             yardstick's maximum is capped at 5e-7 (tests/test_flow_ref.py), so the bound never exceeds 2e-6.
  draw log q the same rule with the fp32 module's own sample_and_log_prob error as the yardstick and the draws' floor of 2e-6;
             fp32 rows: less the first-order effect of rounding x after the density was formed (`f32_rounding_shift`)
  draw x     per coordinate: pcn_ref.MULT x pcn_ref.XI32 (hardware transcendentals against the libm restatement of the same fp32
             Box-Muller formula) carried through the flow's first-order sensitivity sum_k |dx_j / dz_k| (worst row of a
             sample of the pool, fp64 autograd), plus 4 x the fp32 module's own inversion error on the pool, plus - fp32 rows - one
             float32 rounding of the coordinate
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

import pcn_ref as P
from conftest import flow_log_prob_f64, random_coupling_flow, random_maf_flow, zuko_like_state_dict

M64 = (1 << 64) - 1
MARGIN = 4.0           # test_gpu_nsf.MARGIN
DENSITY_FLOOR = 1e-6   # the bar of test_gpu_maf.py / test_gpu_flow16.py
DRAW_FLOOR = 2e-6      # ... of their draw tests (fp64 rows)
YARD_CAP = 5e-7        # the yardstick's own maximum may not exceed this (a condition, not a measurement)
POOL_ROWS = 4096
KINDS = ("coupling", "maf", "softclip")  # softclip: an autoregressive flow in zuko's affine form (ASMC_AFFINE_SOFTCLIP)
BUGS = ("quad_swap", "quad_reuse", "ragged_last", "pad_shift")
COUPLING, MAF = 0, 1   # include/asmc.h ASMC_FLOW_*


def err(a, ref):
    return np.abs(np.asarray(a, dtype=np.float64) - ref) / np.maximum(np.abs(ref), 1.0)


# ---- flows and pools -------------------------------------------------------------------------------------------------------------
def build_flow(kind, d, n_layers, hidden, seed=3, wide=False):
    if kind == "coupling":
        flow = random_coupling_flow(d, n_layers, hidden, seed=seed)
    elif kind == "maf":
        flow = random_maf_flow(d, n_layers, hidden, seed=seed)
    else:
        from aspire_amd.flows import MAFFlow

        flow = MAFFlow.from_zuko_state_dict(zuko_like_state_dict(d, (hidden, hidden), n_layers, seed=seed + d, scale=0.5))
        g = torch.Generator().manual_seed(seed)
        flow.loc = (0.3 * torch.randn(d, generator=g)).to(flow.loc)
        flow.scale = (0.5 + torch.rand(d, generator=g)).to(flow.scale)
    if wide:
        g = np.random.default_rng(seed + 1000)
        # autoregressive flows from 1e-2: at 1e-3 the float32 rounding of x, magnified by loc / scale, takes the fp32 module's own
        # error on their pools to 1e-6 and past the cap on the yardstick (tests/test_flow_ref.py)
        lo = -3.0 if kind == "coupling" else -2.0
        e = g.uniform(lo, 3.0, size=d)
        e[np.argmin(e)], e[np.argmax(e)] = lo, 3.0  # both ends of the range are there
        flow.scale = torch.as_tensor(10.0 ** e, dtype=torch.float32)
    flow._version += 1
    return flow


def shape_of(flow):
    """(ASMC_FLOW_* kind, dims, layers, hidden width) of a torch flow."""
    from aspire_amd.flows import MAFFlow

    ws, _ = flow.export_layers()
    return (MAF if isinstance(flow, MAFFlow) else COUPLING), int(flow.dims), len(flow.layers), int(ws[0].shape[0])


def judge(flow, x):
    """log q(x): the flow's fp32 parameters, fp64 arithmetic (numpy in, numpy out)."""
    x = np.asarray(x, dtype=np.float64)
    if shape_of(flow)[0] == MAF:
        return flow.log_prob_f64(torch.as_tensor(x)).numpy()
    return flow_log_prob_f64(flow, x)


def module(flow, x):
    """log q(x) by the fp32 torch module."""
    return flow.log_prob(torch.as_tensor(np.asarray(x, dtype=np.float64))).double().numpy()


def f64_copy(flow):
    f = copy.deepcopy(flow)
    f.layers.to(torch.float64)
    f.loc, f.scale, f.dtype = f.loc.double(), f.scale.double(), torch.float64
    return f


@dataclass
class Pool:
    key: tuple
    flow: object
    x: np.ndarray   # [rows, d] float64 values, each exactly representable in the row type
    dtype: str      # "f64" / "f32": the row type the device is handed
    _cache: dict = field(default_factory=dict)

    @property
    def ref(self):
        if "ref" not in self._cache:
            self._cache["ref"] = judge(self.flow, self.x)
        return self._cache["ref"]

    @property
    def label(self):
        kind, d, L, h, rows, dt, wide = self.key
        return f"{kind} d={d} L={L} h={h} {dt}" + (" wide" if wide else "")


def pool(kind, d, n_layers, hidden, rows=POOL_ROWS, dtype="f64", wide=False):
    """The pool of these arguments, built once per process."""
    return _pool(kind, int(d), int(n_layers), int(hidden), int(rows), dtype, bool(wide))


@functools.lru_cache(maxsize=None)
def _pool(kind, d, n_layers, hidden, rows, dtype, wide):
    assert rows >= POOL_ROWS and dtype in ("f64", "f32") and kind in KINDS
    flow = build_flow(kind, d, n_layers, hidden, wide=wide)
    g = np.random.default_rng(5)
    x = flow.loc.double().numpy() + 1.2 * flow.scale.double().numpy() * g.normal(size=(rows, d))
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    return Pool((kind, d, n_layers, hidden, rows, dtype, wide), flow, x, dtype)


def yardstick(p: Pool):
    """(max, p99) of the fp32 module's error against the judge on the pool's rows."""
    if "yard" not in p._cache:
        e = err(module(p.flow, p.x), p.ref)
        p._cache["yard"] = (float(e.max()), float(np.percentile(e, 99)))
    return p._cache["yard"]


def draw_yardstick(p: Pool):
    """(max, p99) of the fp32 module's sample_and_log_prob: its log q against the judge at the rows it returned; and the module's
    own inversion error per coordinate, max over the rows: |x_fp32(z) - x_fp64(z)| at the same latent."""
    if "draw" not in p._cache:
        f = p.flow
        z = torch.randn((min(p.x.shape[0], POOL_ROWS), f.dims), dtype=torch.float32, generator=torch.Generator().manual_seed(99))
        with torch.no_grad():
            x, ladj = f._from_latent(z)
            lq = (f._base_logp(z) - ladj).double().numpy()
            x64, _ = f64_copy(f)._from_latent(z.double())
        e = err(lq, judge(p.flow, x.double().numpy()))
        p._cache["draw"] = (float(e.max()), float(np.percentile(e, 99)), (x.double() - x64).abs().max(0).values.numpy())
    return p._cache["draw"]


def bounds(yard, floor):
    return max(floor, MARGIN * yard[0]), max(floor, MARGIN * yard[1])


RECORD = []  # lines of profiles/flow_errors.txt: what the device run measured


def check_errors(e, yard, floor, label):
    """The comparison of the device tests for a log q: error array `e` against MARGIN x the yardstick, floored.  Prints and records
    yardstick, kernel and ratio before it asserts."""
    bmax, b99 = bounds(yard, floor)
    kmax, k99 = float(np.max(e)), float(np.percentile(e, 99))
    line = (f"{label}: yardstick max {yard[0]:.3g} p99 {yard[1]:.3g} | kernel max {kmax:.3g} p99 {k99:.3g} | "
            f"of the bound {kmax / bmax:.2f} / {k99 / b99:.2f}")
    print(line)
    RECORD.append(line)
    assert np.all(np.isfinite(e)), label
    assert kmax <= bmax, (label, kmax, bmax)
    assert k99 <= b99, (label, k99, b99)
    return kmax / bmax


def f32_rounding_shift(flow, x):
    """First-order bound on what rounding every coordinate of x to float32 moves log q by: sum_j |d log q / d x_j| |x_j| 2^-24
    (test_gpu_nsf._f32_rounding_shift, for any of the flows here)."""
    f = f64_copy(flow)
    with torch.enable_grad():
        xx = torch.as_tensor(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
        z, ladj = f._to_latent(xx)
        (grad,) = torch.autograd.grad((f._base_logp(z) + ladj).sum(), xx)
    return (grad.abs() * xx.detach().abs()).sum(-1).numpy() * 2.0**-24


# ---- the draw --------------------------------------------------------------------------------------------------------------------
def half_split(kind, d):
    """First coordinate of the second half of a tile's coordinates: where the kernels' padding sits in front of (f16_nat, the
    coupling tiles' two halves; maf_coord's upper sixteen)."""
    return d // 2 if kind == COUPLING else min(16, (d + 1) // 2)


def latent(seed, gid0, n, draw_id, d, bug=None, kind=COUPLING, rows=None):
    """z [n, d] of particles gid0 .. gid0 + n - 1 (mod 2^64) of draw `draw_id`; rows: only these of the n.  bug: one of BUGS."""
    import oracle as O

    dd = d + 1 if bug == "pad_shift" else d
    idx = np.arange(n) if rows is None else np.asarray(rows)
    z = np.stack([O.pcn_noise(seed, (gid0 + int(i)) & M64, draw_id, dd, "f32")[0] for i in idx])
    if bug is None:
        return z
    assert bug in BUGS and n >= 2 and d >= 2
    if bug == "quad_swap":  # elements 1 and 2 of every quad that has both (d = 2: elements 0 and 1)
        if d == 2:
            z = z[:, ::-1].copy()
        for q in range(d // 4 + 1):
            if 4 * q + 2 < d:
                z[:, [4 * q + 1, 4 * q + 2]] = z[:, [4 * q + 2, 4 * q + 1]]
    elif bug == "quad_reuse":  # quad 1 is quad 0 again (d <= 4: the first quad's upper elements are its lower ones)
        if d > 4:
            w = min(4, d - 4)
            z[:, 4:4 + w] = z[:, :w]
        else:
            z[:, d // 2:] = z[:, :d - d // 2]
    elif bug == "ragged_last":  # the clamp of the ragged tile's spare lanes reaches row n - 1 as well
        last = np.flatnonzero(idx == n - 1)
        z[last] = O.pcn_noise(seed, (gid0 + n - 2) & M64, draw_id, dd, "f32")[0]
    elif bug == "pad_shift":  # the second half of the tile reads one coordinate too far
        h = half_split(kind, d)
        z = np.concatenate([z[:, :h], z[:, h + 1:]], axis=1)
    return z[:, :d]


def draw_ref(flow, z):
    """(x, log q) of the fp64 inverse at latent z: the modules' own _from_latent on an fp64 copy."""
    f = f64_copy(flow)
    zt = torch.as_tensor(np.asarray(z, dtype=np.float64))
    with torch.no_grad():
        x, ladj = f._from_latent(zt)
        return x.numpy(), (f._base_logp(zt) - ladj).numpy()


def sensitivity(flow, x, rows=64):
    """sum_k |dx_j / dz_k| per coordinate j, worst of `rows` rows of x: the inverse of the forward map's Jacobian dz / dx, which
    fp64 autograd gives in d backward passes (the rows of a batch do not interact)."""
    f = f64_copy(flow)
    d = f.dims
    with torch.enable_grad():
        xx = torch.as_tensor(np.asarray(x[:rows], dtype=np.float64)).clone().requires_grad_(True)
        z, _ = f._to_latent(xx)
        jac = torch.stack([torch.autograd.grad(z[:, k].sum(), xx, retain_graph=True)[0] for k in range(d)], dim=1)  # [rows, k, j]
    inv = torch.linalg.inv(jac)  # [rows, j, k] = dx_j / dz_k
    return inv.abs().sum(-1).max(0).values.numpy()


def x_tolerance(p: Pool):
    """Per-coordinate absolute tolerance of a drawn position against draw_ref (module docstring)."""
    if "tol_x" not in p._cache:
        p._cache["tol_x"] = P.MULT * P.XI32 * sensitivity(p.flow, p.x) + MARGIN * draw_yardstick(p)[2]
    return p._cache["tol_x"]


def compare_draw(x_got, x_ref, tol_x, f32=False, label=""):
    """The comparison of the device tests for drawn positions, row by row: returns the worst |x - ref| / tol.  f32: the rows were
    rounded to float32 on the way out, half a spacing of the coordinate more."""
    x_got, x_ref = np.asarray(x_got, dtype=np.float64), np.asarray(x_ref, dtype=np.float64)
    assert x_got.shape == x_ref.shape and np.all(np.isfinite(x_got)), label
    tol = tol_x[None, :] + (2.0**-24 * np.abs(x_ref) if f32 else 0.0)
    ratio = np.abs(x_got - x_ref) / tol
    worst = float(ratio.max())
    assert worst <= 1.0, (label, worst, np.unravel_index(np.argmax(ratio), ratio.shape))
    return worst


# ---- routing and rounds, restated from csrc/asmc_flow.hip and csrc/asmc_flow16.hip ---------------------------------------------------
def layout(kind, d, hidden):
    """asmc_flow_layout for the affine kinds."""
    if hidden not in (32, 64, 128):
        return -1
    if kind == COUPLING:
        return -1 if (d < 2 or d % 2 or d > 128) else (1 if d > 32 else 0)
    if kind == MAF:
        return -1 if (d < 1 or d > 128) else (1 if (d > 32 or hidden == 128) else 0)
    return -1


def layer_floats(H, W):
    """FlowDims<H, W>::LAYER: biases in lane order, then the three operand images."""
    return (2 * (W // 32) + H // 16) * 32 + W * H + W * W + 2 * H * W


def layer16_words(kind, D, W):
    """Flow16<KIND, D, W>: (BIAS, LAYER_A) 4-byte words per layer."""
    cs = D // 4 if kind == MAF else D // 8
    ks1, ks2, nb1, nb3 = cs // 8, W // 32, W // 16, cs // 2
    return 2 * W + nb3 * 16, nb1 * ks1 * 512 + nb1 * ks2 * 512 + nb3 * ks2 * 512


def pack_floats(kind, d, n_layers, hidden):
    lay = layout(kind, d, hidden)
    if lay == 0:
        return n_layers * layer_floats(16 if kind == COUPLING else 32, hidden)
    if lay == 1:
        return n_layers * sum(layer16_words(kind, 64 if d <= 64 else 128, hidden))
    return -4  # ASMC_ERR_UNSUPPORTED


def route(kind, d, hidden, op, xt="d", math="split", tpw=1):
    """(kernel, template arguments as the mangled symbol carries them) that asmc_coupling_logprob (op = "logprob") or
    asmc_coupling_sample (op = "sample") launches for this shape; None where the call is refused.  xt: "d" / "f" rows;
    math: ASMC_FLOW_MATH ("split" default, "f32"); tpw: ASMC_FLOW_TPW."""
    lay = layout(kind, d, hidden)
    if lay < 0 or (math == "f32" and (lay == 1 or op == "sample")):
        return None
    if lay == 1:
        return (f"k_flow16_{op}", f"Li{kind}ELi{64 if d <= 64 else 128}ELi{hidden}E{xt}Li512E")
    if kind == COUPLING:
        if op == "sample":
            return ("k_coupling_sample", f"Li16ELi{hidden}E{xt}Li512E")
        if tpw == 2 and hidden <= 64:
            return ("k_coupling_logprob", f"Li16ELi{hidden}E{xt}Li512ELi2ELb0E")
        return ("k_coupling_logprob", f"Li16ELi{hidden}E{xt}Li512ELi1ELb{int(math == 'split')}E")
    if op == "sample":
        return ("k_maf_sample", f"Li32ELi{hidden}E{xt}Li512E")
    return ("k_maf_logprob", f"Li32ELi{hidden}E{xt}Li512ELb{int(math == 'split')}E")


def reachable():
    """Every instantiation of the six kernels that some shape, row type and switch reaches."""
    t = set()
    for kind in (COUPLING, MAF):
        for d in range(1, 129):
            for hidden in (32, 64, 128):
                for xt in "df":
                    for op in ("logprob", "sample"):
                        for math in ("split", "f32"):
                            for tpw in (1, 2):
                                r = route(kind, d, hidden, op, xt, math, tpw)
                                if r is not None:
                                    t.add(r)
    return t


RESIDENT_LIMIT = 150 * 1024  # bytes of layers k_coupling_logprob keeps in LDS together (launch_flow); the draw's limit as well


def coupling_resident(n_layers, hidden):
    return n_layers * layer_floats(16, hidden) * 4 <= RESIDENT_LIMIT


def rows_per_round(kernel, flow, num_cu, tpw=1):
    """Rows one pass of `kernel`'s grid-stride loop covers on a device of num_cu compute units: the grid is capped at
    num_cu x per_cu blocks of eight waves, per_cu = 1 where a block's LDS footprint exceeds 80 KB, else 2."""
    kind, d, n_layers, hidden = shape_of(flow)
    if kernel.startswith("k_flow16"):
        assert layout(kind, d, hidden) == 1
        return num_cu * 2 * 8 * 16
    assert layout(kind, d, hidden) == 0
    lds = n_layers * layer_floats(16 if kind == COUPLING else 32, hidden) * 4
    if kernel == "k_coupling_logprob":
        if not coupling_resident(n_layers, hidden):
            lds = layer_floats(16, hidden) * 4  # streamed: one layer at a time
        return num_cu * (1 if lds > 80 * 1024 else 2) * 8 * 32 * tpw
    assert kernel in ("k_coupling_sample", "k_maf_logprob", "k_maf_sample") and tpw == 1
    return num_cu * (1 if lds > 80 * 1024 else 2) * 8 * 32


# ---- planted rows ------------------------------------------------------------------------------------------------------------------
def plant(x, flow, hs):
    """Rows 100 .. 103 of a copy of x (>= 128 rows): one NaN coordinate, one +inf, one -inf, and - `hs`, the split-fp16 paths - a row
    times 1e6 in standardised units (every coordinate at least 5e5 scales from loc), whose operands leave the fp16 range.
    Returns (rows, the row that only the split-fp16 kernels answer with NaN)."""
    x = x.copy()
    d = x.shape[1]
    assert x.shape[0] >= 128
    x[100, (d - 1) // 2] = np.nan
    x[101, d - 1] = np.inf
    x[102, 0] = -np.inf
    if hs:
        loc, scale = flow.loc.double().numpy(), flow.scale.double().numpy()
        z = (x[103] - loc) / scale
        x[103] = loc + scale * 1e6 * np.where(z < 0, -1.0, 1.0) * np.maximum(np.abs(z), 0.5)
    return x, (103 if hs else None)


# ---- the cases of tests/test_gpu_flow_kernels.py (tests/test_flow_ref.py caps the yardstick of each pool on the CPU) -------------------
# (kind, dims, layers, hidden): layout 0 coupling flows take k_coupling_*<16, hidden, ..>; d = 32 is the vector-load branch, every other
# d the scalar one.  Width 64: 2 layers are resident with two blocks per CU, 4 layers resident with one, 6 layers streamed; width 128:
# 1 layer resident, 2 layers streamed.
L0_COUPLING = [("coupling", 32, 2, 32), ("coupling", 18, 2, 32), ("coupling", 32, 2, 64), ("coupling", 30, 3, 64),
               ("coupling", 32, 1, 128), ("coupling", 2, 2, 128), ("coupling", 32, 4, 64), ("coupling", 32, 6, 64),
               ("coupling", 32, 2, 128)]
L0_MAF = [("maf", 32, 3, 64), ("maf", 17, 2, 32), ("maf", 1, 2, 32), ("maf", 31, 2, 64), ("softclip", 32, 2, 64),
          ("softclip", 17, 2, 32)]
L1 = [("coupling", 34, 2, 32), ("coupling", 64, 2, 64), ("coupling", 62, 1, 128), ("coupling", 66, 2, 32), ("coupling", 128, 2, 64),
      ("coupling", 126, 1, 128), ("maf", 33, 2, 32), ("maf", 64, 2, 64), ("maf", 63, 1, 128), ("maf", 65, 2, 32), ("maf", 128, 2, 64),
      ("maf", 127, 1, 128), ("maf", 12, 2, 128), ("softclip", 64, 2, 64), ("softclip", 100, 2, 32)]
WIDE = [("coupling", 10, 2, 64), ("softclip", 17, 2, 32), ("coupling", 66, 2, 32)]  # scale log-uniform in [1e-3, 1e3] (autoregressive: [1e-2, 1e3])
EDGES_L0 = (1, 31, 32, 33, 255, 256, 257)   # rows around one tile, one block
EDGES_L1 = (1, 15, 16, 17, 33, 127, 128, 129, 257)  # ... one group, one block (and the guard-band sizes 33 and 257)
N_CASE = 1000
# the second grid-stride round: kernel -> (pool, row type); the row count is rows_per_round + 4097 on the device the test runs on
SECOND_ROUND = {"k_coupling_logprob resident": (("coupling", 32, 4, 64), "f64"), "k_coupling_logprob streamed": (("coupling", 32, 2, 128), "f32"),
                "k_maf_logprob": (("maf", 32, 3, 64), "f32"), "k_flow16_logprob coupling": (("coupling", 66, 2, 32), "f64"),
                "k_flow16_logprob maf": (("maf", 33, 2, 32), "f64"),
                "k_coupling_sample": (("coupling", 32, 2, 64), "f64"), "k_maf_sample": (("maf", 17, 2, 32), "f64"),
                "k_flow16_sample coupling": (("coupling", 34, 2, 32), "f64"), "k_flow16_sample maf": (("maf", 33, 2, 32), "f64")}
# ASMC_FLOW_TPW=2 (a child process): widths 32 and 64, both row types, both load branches; rows round the 64-row unit of two tiles
TPW_CASES = [(("coupling", 18, 2, 32), "f64"), (("coupling", 18, 2, 32), "f32"), (("coupling", 32, 2, 64), "f64"), (("coupling", 32, 2, 64), "f32")]
TPW_ROWS = (63, 64, 65, 4099)
TAIL = 4097  # rows of the second round: ragged, and fewer tiles than waves
# (gid0, draw_id) of the draw cases, in rotation: particle indices above 2^32 and across the wrap of 2^64, the ends of the draw counter
DRAW_KEYS = ((0, 1), (2**32 + 5, 0), (2**64 - 3, 2**32 - 1), (1000, 7))
DRAW_SEED = 1234


def is_l0(key):
    return layout(MAF if key[0] != "coupling" else COUPLING, key[1], key[3]) == 0


def density_cases():
    """(pool key, row type, wide, rows, ASMC_FLOW_MATH) of the density test."""
    out = []
    for key in L0_COUPLING + L0_MAF + L1:
        for dt in ("f64", "f32"):
            for math in (("split", "f32") if is_l0(key) else ("split",)):
                out.append((key, dt, False, N_CASE, math))
    for key in WIDE:
        for dt in ("f64", "f32"):
            out.append((key, dt, True, N_CASE, "split"))
    for key, dt, edges in ((("coupling", 18, 2, 32), "f64", EDGES_L0), (("coupling", 32, 2, 64), "f32", EDGES_L0),
                           (("maf", 17, 2, 32), "f64", EDGES_L0), (("maf", 32, 3, 64), "f32", EDGES_L0),
                           (("coupling", 34, 2, 32), "f64", EDGES_L1), (("maf", 65, 2, 32), "f32", EDGES_L1)):
        for n in edges:
            out.append((key, dt, False, n, "split"))
        if is_l0(key):
            out += [(key, dt, False, n, "f32") for n in (33, 257)]
    return out


def draw_cases():
    """(pool key, row type, wide, rows, (gid0, draw_id)) of the draw test: every shape of the density test that the draw takes."""
    out = []
    for key in L0_COUPLING + L0_MAF + L1:
        if key[0] == "coupling" and is_l0(key) and not coupling_resident(key[2], key[3]):
            continue  # refused: test_other_refusals
        for dt in ("f64", "f32"):
            out.append((key, dt, False, N_CASE))
    out += [(key, dt, True, N_CASE) for key in WIDE for dt in ("f64", "f32")]
    for key, dt, edges in ((("coupling", 18, 2, 32), "f32", EDGES_L0), (("maf", 17, 2, 32), "f64", EDGES_L0),
                           (("coupling", 34, 2, 32), "f64", EDGES_L1), (("maf", 65, 2, 32), "f32", EDGES_L1)):
        out += [(key, dt, False, n) for n in edges]
    return [c + (DRAW_KEYS[i % len(DRAW_KEYS)],) for i, c in enumerate(out)]


def case_id(c):
    key, dt, wide, n = c[:4]
    tail = c[4] if isinstance(c[4], str) else f"gid{c[4][0] % 1000}"
    return f"{key[0]}-d{key[1]}-L{key[2]}-h{key[3]}-{dt}{'-wide' if wide else ''}-n{n}-{tail}"


def gpu_pools(num_cu=256):
    """Every pool the device module builds, on a device of num_cu compute units (an MI355X has 256): {pool arguments}."""
    s = {(c[0], POOL_ROWS, c[1], c[2]) for c in density_cases() + draw_cases()}
    for name, (key, dt) in SECOND_ROUND.items():
        rows = rows_per_round(name.split()[0], build_flow(*key), num_cu) + TAIL
        s.add((key, rows, dt, False))
    s |= {(key, max(TPW_ROWS), dt, False) for key, dt in TPW_CASES}
    return sorted(s)
