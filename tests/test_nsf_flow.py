"""NSFFlow (aspire_amd/flows.py): the torch modules against the fp64 numpy restatement of the spline's specification
(tests/nsf_ref.py), the edges of the spline's domain, the autoregressive structure and the host plumbing.  No GPU."""
import math

import numpy as np
import pytest
import torch

import nsf_ref

B = 5.0


def _rows(flow, n, seed, spread=1.5):
    g = np.random.default_rng(seed)
    return flow.loc.double().numpy() + spread * flow.scale.double().numpy() * g.normal(size=(n, flow.dims))


@pytest.mark.parametrize("d,n_tr,hidden", [(1, 2, 16), (5, 2, 32), (32, 3, 64)])
def test_module_matches_the_restatement(d, n_tr, hidden):
    flow = nsf_ref.random_nsf_flow(d, n_tr, hidden, seed=3, scale=0.5, dtype=torch.float64)
    x = _rows(flow, 40, 1)
    got = flow.log_prob(torch.as_tensor(x)).numpy()
    want = nsf_ref.log_prob(flow, x)
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert rel.max() <= 1e-10, rel.max()
    z, _ = flow.forward(torch.as_tensor(x))
    assert np.abs(z.numpy() - nsf_ref.forward(flow, x)[0]).max() <= 1e-9
    back, _ = flow.inverse(z)
    assert np.abs(back.numpy() - x).max() <= 1e-9
    assert np.abs(nsf_ref.inverse(flow, z.numpy()) - x).max() <= 1e-9
    # log_prob_f64 is the same evaluation for a float64 flow
    assert np.abs(flow.log_prob_f64(x).numpy() - got).max() <= 1e-12


def test_planted_rows_at_the_edges_of_the_spline():
    """Exactly +-B, |x| = 7 (the identity, log J = 0) and one ulp either side of an interior knot (value and density continuous)."""
    flow = nsf_ref.random_nsf_flow(3, 1, 16, seed=5, scale=0.7, dtype=torch.float64)
    flow.loc, flow.scale = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    layer = flow.layers[0]
    base = np.array([0.3, -0.4, 0.9])
    # coordinate of degree 1 (index 0): its spline does not depend on x, so its knots are constants
    with torch.no_grad():
        X, _, _ = layer._params(torch.zeros(1, 3, dtype=torch.float64))
    knot = float(X[0, 0, 3])
    rows = []
    for v in (B, -B, 7.0, -7.0, np.nextafter(knot, -np.inf), knot, np.nextafter(knot, np.inf)):
        r = base.copy()
        r[0] = v
        rows.append(r)
    rows = np.array(rows)
    z, _ = flow.forward(torch.as_tensor(rows))
    z = z.numpy()
    lq = flow.log_prob(torch.as_tensor(rows)).numpy()
    zr, lqr = nsf_ref.forward(flow, rows)
    assert np.abs(z - zr).max() <= 1e-10 and np.abs(lq - lqr).max() <= 1e-9
    assert abs(z[0, 0] - B) <= 1e-12  # x = +B: the last bin at zeta = 1
    assert z[1, 0] == -B and z[2, 0] == 7.0 and z[3, 0] == -7.0  # outside: the identity
    # the Jacobian of coordinate 0 outside the box is 1: the transform's log-determinant is that of the other coordinates
    for i in (2, 3):
        one = rows[i: i + 1].copy()
        with torch.no_grad():
            _, l0 = layer.forward(torch.as_tensor(one))
            X1, Y1, D1 = layer._params(torch.as_tensor(one))
        others = sum(nsf_ref.spline_forward(one[0, j], X1[0, j].tolist(), Y1[0, j].tolist(), D1[0, j].tolist())[1] for j in (1, 2))
        assert abs(float(l0) - others) <= 1e-10
    assert np.abs(np.diff(z[4:7, 0])).max() <= 1e-14 and np.abs(np.diff(lq[4:7])).max() <= 1e-9


def test_zero_initialised_flow_is_the_standardised_normal():
    from aspire_amd.flows import NSFFlow

    flow = NSFFlow(6, n_transforms=2, hidden_features=(16, 16), dtype=torch.float64)
    flow.loc = torch.linspace(-1, 1, 6, dtype=torch.float64)
    flow.scale = torch.linspace(0.5, 2, 6, dtype=torch.float64)
    x = _rows(flow, 200, 2, spread=2.5)
    z = (x - flow.loc.numpy()) / flow.scale.numpy()
    want = -0.5 * (z * z).sum(1) - 3.0 * math.log(2 * math.pi) - np.log(flow.scale.numpy()).sum()
    assert np.abs(flow.log_prob(torch.as_tensor(x)).numpy() - want).max() <= 1e-12


@pytest.mark.parametrize("t", [0, 1])
def test_autoregressive_property_in_both_variable_orders(t):
    flow = nsf_ref.random_nsf_flow(6, 2, 32, seed=8, scale=0.6, dtype=torch.float64)
    layer = flow.layers[t]
    order = layer.order.numpy()
    assert np.array_equal(order, np.arange(1, 7) if t == 0 else np.arange(6, 0, -1))
    x = torch.as_tensor(np.random.default_rng(0).normal(size=(1, 6)))
    z0, _ = layer.forward(x)
    for j in range(6):
        xp = x.clone()
        xp[0, j] += 0.37
        z1, _ = layer.forward(xp)
        changed = (z1 != z0)[0].numpy()
        assert changed[j]
        for i in range(6):
            if changed[i]:
                assert order[i] >= order[j]
        assert any(changed[i] for i in range(6) if order[i] > order[j]) or order[j] == 6


def test_export_layers_zeros_coincide_with_the_masks():
    flow = nsf_ref.random_nsf_flow(5, 2, 32, seed=1, scale=0.5)
    ws, bs = flow.export_layers()
    assert len(ws) == 6 and ws[2].shape == (5 * 23, 32) and bs[2].shape == (5 * 23,) and ws[0].dtype == np.float32
    i = 0
    for layer in flow.layers:
        for m in layer.net:
            if hasattr(m, "mask"):
                assert np.array_equal(ws[i] != 0.0, m.mask.numpy() != 0.0)
                i += 1
    # all 23 rows of a coordinate carry the same mask row
    last = flow.layers[0].net[-1].mask.numpy().reshape(5, 23, 32)
    assert np.array_equal(last, np.repeat(last[:, :1], 23, axis=1))


def test_aspire_builds_the_nsf_flow_and_load_flow_maps_the_backend():
    from aspire_amd import Aspire, NSFFlow

    f = lambda s: -0.5 * (s.x * s.x).sum(1)  # noqa: E731
    asp = Aspire(log_likelihood=f, log_prior=f, dims=4, xp=torch, flow_backend="nsf", transforms=2, bins=8, hidden_features=(16, 16),
                 passes=2)
    asp.init_flow()
    assert type(asp._flow) is NSFFlow and len(asp._flow.layers) == 2 and asp._flow.bins == 8
    assert asp._flow._init_args["bins"] == 8 and asp._flow._init_args["bound"] == 5.0

    class Group(dict):  # the group protocol `save` / `load` use
        def create_group(self, k):
            self[k] = Group()
            return self[k]

        def create_dataset(self, k, data):
            self[k] = np.asarray(data) if not isinstance(data, str) else data

    flow = nsf_ref.random_nsf_flow(4, 2, 16, seed=2, scale=0.5)
    store = Group()
    flow.save(store, "flow")
    asp.load_flow(store, "flow")
    assert type(asp._flow) is NSFFlow
    x = torch.as_tensor(_rows(flow, 50, 3), dtype=torch.float32)
    assert torch.equal(asp._flow.log_prob(x), flow.log_prob(x))


def test_device_coupling_refuses_what_the_kernels_do_not_take():
    from aspire_amd.flows import NSFFlow

    class Eng:
        def make_nsf(self, *a, **k):
            raise AssertionError("must be refused before packing")

    for kw in (dict(dtype=torch.float64), dict(bins=4), dict(bound=3.0), dict(hidden_features=(32, 64))):
        with pytest.raises(ValueError):
            NSFFlow(4, **kw).device_coupling(Eng())
    with pytest.raises(ValueError):
        NSFFlow(33, hidden_features=(32, 32)).device_coupling(Eng())


def test_fit_lowers_the_validation_loss_on_a_two_mode_sample():
    from aspire_amd.flows import NSFFlow

    g = np.random.default_rng(4)
    x = np.concatenate([g.normal(-2.0, 0.4, size=(600, 2)), g.normal(2.0, 0.4, size=(600, 2))])
    g.shuffle(x)
    flow = NSFFlow(2, n_transforms=2, hidden_features=(32, 32))
    hist = flow.fit(x, n_epochs=10, batch_size=200, lr=5e-3)
    assert len(hist.validation_loss) == 10 and min(hist.validation_loss[1:]) < hist.validation_loss[0] - 0.05
    xs, lq = flow.sample_and_log_prob(100)
    assert torch.isfinite(xs).all() and torch.isfinite(lq).all()


def test_nsf_pack_floats_on_supported_and_unsupported_shapes():
    try:
        from aspire_amd import _lib

        lib = _lib.load()
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"libasmc_hip.so cannot be loaded here: {exc}")
    for d, h in ((1, 32), (5, 32), (16, 64), (32, 64), (17, 64)):
        assert lib.asmc_nsf_pack_floats(d, 3, h, 8) > 0
    assert lib.asmc_nsf_pack_floats(32, 3, 64, 4) < 0
    assert lib.asmc_nsf_pack_floats(33, 3, 64, 8) < 0
    assert lib.asmc_nsf_pack_floats(32, 3, 48, 8) < 0
    assert lib.asmc_flow_layout(_lib.ASMC_FLOW_NSF, 32, 64) not in (0, 1) and lib.asmc_flow_layout(_lib.ASMC_FLOW_NSF, 32, 64) > 0
    assert lib.asmc_flow_layout(_lib.ASMC_FLOW_NSF, 33, 64) < 0 and lib.asmc_flow_layout(_lib.ASMC_FLOW_NSF, 32, 128) < 0


@pytest.mark.parametrize("d,hidden", [(5, 32), (16, 64), (17, 64), (32, 64)])
def test_nsf_pack_is_the_network_in_mfma_operand_order(d, hidden):
    """asmc_nsf_pack (host only): reading the packed block back the way the kernels do - an output block's image is
    [K step][hi | lo][lane][8 halves], lane (m, g) slot j of K step S is column 16 (2 S + j / 4) + 4 g + j % 4 of row m; output
    block 23 cg + c holds parameter c of the coordinates 16 cg .. 16 cg + 15 - and evaluating the three layers in fp64 gives the
    module's raw spline parameters; padded rows and columns are zero."""
    try:
        from aspire_amd import _lib
        from aspire_amd.engine import pack_nsf

        lib = _lib.load()
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"libasmc_hip.so cannot be loaded here: {exc}")
    flow = nsf_ref.random_nsf_flow(d, 2, hidden, seed=6, scale=0.5)
    ws, bs = flow.export_layers()
    packed = pack_nsf(lib, d, hidden, 8, ws, bs)
    ncg, ks2, nb1 = (1 if d <= 16 else 2), hidden // 32, hidden // 16
    nb3 = 23 * ncg
    n_bias = 2 * hidden + nb3 * 16
    layer_a = nb1 * 512 + nb1 * ks2 * 512 + nb3 * ks2 * 512
    assert packed.size == 2 * (n_bias + layer_a)
    img = packed[2 * n_bias:].view(np.float16)

    def matrix(words0, n_blocks, ks):  # -> [16 n_blocks, 32 ks] fp64
        a = img[2 * words0: 2 * (words0 + n_blocks * ks * 512)].astype(np.float64).reshape(n_blocks, ks, 2, 64, 8).sum(2)
        out = np.zeros((16 * n_blocks, 32 * ks))
        for lane in range(64):
            m, g = lane & 15, lane >> 4
            for S in range(ks):
                for j in range(8):
                    out[np.arange(n_blocks) * 16 + m, 16 * (2 * S + j // 4) + 4 * g + j % 4] = a[:, S, lane, j]
        return out

    x = np.random.default_rng(2).normal(size=d)
    for t in range(2):
        b = packed[t * n_bias: (t + 1) * n_bias].astype(np.float64)
        off = t * layer_a
        A1 = matrix(off, nb1, 1)
        A2 = matrix(off + nb1 * 512, nb1, ks2)
        A3 = matrix(off + nb1 * 512 + nb1 * ks2 * 512, nb3, ks2)
        xin = np.zeros(32)
        xin[:d] = x
        h = np.maximum(A1 @ xin + b[:hidden], 0.0)
        h = np.maximum(A2 @ h + b[hidden: 2 * hidden], 0.0)
        o = (A3 @ h + b[2 * hidden:]).reshape(ncg, 23, 16)  # [cg][parameter][coordinate in the group]
        W1, W2, W3 = (np.asarray(w, dtype=np.float64) for w in ws[3 * t: 3 * t + 3])
        hh = np.maximum(W1 @ x + bs[3 * t], 0.0)
        hh = np.maximum(W2 @ hh + bs[3 * t + 1], 0.0)
        want = (W3 @ hh + bs[3 * t + 2]).reshape(d, 23)
        got = o.transpose(0, 2, 1).reshape(16 * ncg, 23)
        assert np.abs(got[:d] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())  # (hi + lo carries 22 bits of every weight)
        assert np.all(got[d:] == 0.0) and np.all(A1[:, d:] == 0.0)
    bad = [w.copy() for w in ws]
    bad[2][0, 0] = 7e4
    with pytest.raises(Exception, match="fp16 operand range"):
        pack_nsf(lib, d, hidden, 8, bad, bs)
