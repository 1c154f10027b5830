"""fp64 numpy restatement of the neural spline flow (aspire_amd.flows.NSFFlow), written from the formulas of its specification
with plain loops over transforms, coordinates and bins - not a copy of the torch module.  It reads the flow's parameters through
its masked matrices, `loc`, `scale` and every transform's `order` buffer.

    c = ln 1000;  w <- w / (1 + 2|w|/c), h likewise, delta <- delta / (1 + |delta|/c)
    X_0 = -B, X_j = B (2 sum_{m<=j} softmax(w)_m - 1), X_K = +B exactly (Y from h), D_0 = D_K = 1, D_j = exp(delta_j)
    k = #{j in 0..K: X_j < x} - 1; inside <=> 0 <= k < K; outside: y = x, log J = 0
"""
import math

import numpy as np
import torch

C = math.log(1000.0)


def _params(flow):
    # the masked matrices at the flow's own precision (`export_layers()` rounds to fp32, which a float64 flow is not)
    lin = [m for layer in flow.layers for m in layer.net if hasattr(m, "mask")]
    ws = [(m.weight * m.mask).detach().cpu().double().numpy() for m in lin]
    bs = [m.bias.detach().cpu().double().numpy() for m in lin]
    orders = [layer.order.detach().cpu().numpy().astype(np.int64) for layer in flow.layers]
    return ws, bs, orders


def _net(ws, bs, t, x):
    h = np.maximum(ws[3 * t] @ x + bs[3 * t], 0.0)
    h = np.maximum(ws[3 * t + 1] @ h + bs[3 * t + 1], 0.0)
    return ws[3 * t + 2] @ h + bs[3 * t + 2]


def knots(raw, B, two):
    """K + 1 knots from K raw widths (or heights)."""
    K = len(raw)
    r = [v / (1.0 + two * abs(v) / C) for v in raw]
    m = max(r)
    e = [math.exp(v - m) for v in r]
    tot = sum(e)
    out, acc = [-B], 0.0
    for j in range(K - 1):
        acc += e[j] / tot
        out.append(B * (2.0 * acc - 1.0))
    out.append(B)
    return out


def derivs(raw):
    return [1.0] + [math.exp(v / (1.0 + abs(v) / C)) for v in raw] + [1.0]


def bin_of(kn, v):
    return sum(1 for t in kn if t < v) - 1


def spline_forward(x, X, Y, D):
    """(y, log J) of one coordinate."""
    K = len(X) - 1
    k = bin_of(X, x)
    if not (0 <= k < K) or not math.isfinite(x):
        return x, 0.0
    wd, ht = X[k + 1] - X[k], Y[k + 1] - Y[k]
    s = ht / wd
    z = (x - X[k]) / wd
    q = s + (D[k] + D[k + 1] - 2.0 * s) * z * (1.0 - z)
    y = Y[k] + ht * (s * z * z + D[k] * z * (1.0 - z)) / q
    lj = math.log(s * s * (2.0 * s * z * (1.0 - z) + D[k] * (1.0 - z) ** 2 + D[k + 1] * z * z) / (q * q))
    return y, lj


def spline_inverse(y, X, Y, D):
    K = len(X) - 1
    k = bin_of(Y, y)
    if not (0 <= k < K):
        return y
    wd, ht = X[k + 1] - X[k], Y[k + 1] - Y[k]
    s = ht / wd
    eta = y - Y[k]
    t = D[k] + D[k + 1] - 2.0 * s
    a = ht * (s - D[k]) + eta * t
    b = ht * D[k] - eta * t
    c2 = -s * eta
    zeta = 2.0 * c2 / (-b - math.sqrt(b * b - 4.0 * a * c2))
    return X[k] + zeta * wd


def _coord_params(phi, i, K, B):
    P = 3 * K - 1
    row = phi[i * P: (i + 1) * P]
    return knots(row[:K], B, 2.0), knots(row[K: 2 * K], B, 2.0), derivs(row[2 * K:])


def forward(flow, x):
    """(z, log q(x)) for rows x [n, d] (fp64)."""
    ws, bs, _ = _params(flow)
    K, B, d = flow.bins, flow.bound, flow.dims
    loc = flow.loc.detach().cpu().numpy().astype(np.float64)
    scale = flow.scale.detach().cpu().numpy().astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    zs, lq = np.empty_like(x), np.empty(x.shape[0])
    for r in range(x.shape[0]):
        v = (x[r] - loc) / scale
        ladj = -np.log(scale).sum()
        for t in range(len(flow.layers)):
            phi = _net(ws, bs, t, v)
            out = np.empty(d)
            for i in range(d):
                X, Y, D = _coord_params(phi, i, K, B)
                out[i], lj = spline_forward(v[i], X, Y, D)
                ladj += lj
            v = out
        zs[r] = v
        lq[r] = -0.5 * (v * v).sum() - 0.5 * d * math.log(2.0 * math.pi) + ladj
    return zs, lq


def log_prob(flow, x):
    return forward(flow, x)[1]


def inverse(flow, z):
    """x with forward(x) = z, rows [n, d]: transforms in reverse, coordinates in each transform's variable order."""
    ws, bs, orders = _params(flow)
    K, B, d = flow.bins, flow.bound, flow.dims
    loc = flow.loc.detach().cpu().numpy().astype(np.float64)
    scale = flow.scale.detach().cpu().numpy().astype(np.float64)
    z = np.asarray(z, dtype=np.float64)
    xs = np.empty_like(z)
    for r in range(z.shape[0]):
        v = z[r].copy()
        for t in reversed(range(len(flow.layers))):
            xcur = np.zeros(d)
            for i in np.argsort(orders[t]):
                phi = _net(ws, bs, t, xcur)
                X, Y, D = _coord_params(phi, i, K, B)
                xcur[i] = spline_inverse(v[i], X, Y, D)
            v = xcur
        xs[r] = v * scale + loc
    return xs


def random_nsf_flow(d, n_transforms, hidden, seed, scale, dtype=torch.float32):
    """An NSFFlow whose weights are randomised, the last layer included (std scale / sqrt(h / 2), bias 0.3 scale), with a
    non-trivial loc / scale: a fresh or briefly trained flow is the identity and tests nothing."""
    from aspire_amd.flows import NSFFlow

    flow = NSFFlow(d, n_transforms=n_transforms, hidden_features=(hidden, hidden), seed=seed, dtype=dtype)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for layer in flow.layers:
            for m in layer.net:
                if hasattr(m, "mask"):
                    m.weight.copy_((torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * scale / math.sqrt(hidden / 2)).to(dtype))
                    m.bias.copy_((torch.randn(m.bias.shape, generator=g, dtype=torch.float64) * 0.3 * scale).to(dtype))
        flow.loc = (torch.randn(d, generator=g, dtype=torch.float64) * 0.7).to(dtype)
        flow.scale = (0.5 + torch.rand(d, generator=g, dtype=torch.float64) * 1.5).to(dtype)
    flow._version += 1
    return flow
