"""tests/flow_ref.py on the CPU: the yardsticks tests/test_gpu_flow_kernels.py divides by are capped, the references agree with
each other and with pcn_ref, the comparison of the device tests catches every planted defect, and the routing table that module's
header states is the library's (asmc_flow_layout and the pack-size functions are host-only: no device)."""
import numpy as np
import pytest
import torch

import flow_ref as F
import pcn_ref as P

MI355X_CUS = 256


@pytest.fixture(scope="module")
def lib():
    import os

    from aspire_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


@pytest.mark.parametrize("args", F.gpu_pools(MI355X_CUS), ids=lambda a: f"{'-'.join(map(str, a[0]))}-{a[1]}-{a[2]}{'-wide' if a[3] else ''}")
def test_yardstick_of_every_device_pool_is_capped(args):
    """The fp32 module's own maximum error on each pool the device module uses is at most 5e-7: with it the density bound
    max(1e-6, 4 x yardstick) never exceeds 2e-6.  The draw's yardstick (the module's sample_and_log_prob) is held to the same cap."""
    key, rows, dt, wide = args
    p = F.pool(*key, rows=rows, dtype=dt, wide=wide)
    ymax, y99 = F.yardstick(p)
    dmax, d99, _ = F.draw_yardstick(p)
    print(f"{p.label} rows={rows}: density yardstick max {ymax:.3g} p99 {y99:.3g} | draw yardstick max {dmax:.3g} p99 {d99:.3g}")
    assert 0.0 < y99 <= ymax <= F.YARD_CAP, (p.label, ymax)
    assert 0.0 < d99 <= dmax <= F.YARD_CAP, (p.label, dmax)
    assert max(F.bounds((ymax, y99), F.DENSITY_FLOOR)) <= 2e-6


def test_fewer_rows_than_the_pool_keep_the_pools_yardstick():
    p = F.pool("coupling", 18, 2, 32)
    assert p.x.shape[0] == F.POOL_ROWS and F.yardstick(p) is F.yardstick(F.pool("coupling", 18, 2, 32))
    few = F.err(F.module(p.flow, p.x[:33]), p.ref[:33])
    assert few.max() <= F.yardstick(p)[0]


def test_f32_pools_hold_rows_that_are_exact_in_float32():
    p = F.pool("maf", 17, 2, 32, dtype="f32")
    assert np.array_equal(p.x, p.x.astype(np.float32).astype(np.float64))
    q = F.pool("maf", 17, 2, 32, dtype="f64")
    assert not np.array_equal(q.x, q.x.astype(np.float32).astype(np.float64))


def test_wide_pools_span_their_whole_range_of_scale():
    for key in F.WIDE:
        s = F.pool(*key, wide=True).flow.scale.numpy()
        lo = 1e-3 if key[0] == "coupling" else 1e-2  # (autoregressive flows: narrowed until the yardstick met its cap)
        assert s.min() == np.float32(lo) and s.max() == np.float32(1e3), (key, s.min(), s.max())


@pytest.mark.parametrize("key", [("coupling", 18, 2, 32), ("maf", 17, 2, 32), ("softclip", 17, 2, 32), ("coupling", 66, 2, 32), ("maf", 65, 2, 32)])
def test_draw_ref_pushed_back_through_the_fp64_flow_returns_its_latent(key):
    p = F.pool(*key)
    z = F.latent(F.DRAW_SEED, 2**32 + 5, 300, 0, key[1])
    x, lq = F.draw_ref(p.flow, z)
    zb, _ = F.f64_copy(p.flow)._to_latent(torch.as_tensor(x))
    np.testing.assert_allclose(zb.detach().numpy(), z, rtol=0, atol=1e-11)
    np.testing.assert_allclose(lq, F.judge(p.flow, x), rtol=1e-12, atol=1e-11)


@pytest.mark.parametrize("gid0,draw_id", F.DRAW_KEYS)
def test_latent_is_pcn_refs_fast_noise(gid0, draw_id):
    for d in (1, 2, 5, 17, 66):
        z = F.latent(77, gid0, 9, draw_id, d)
        assert np.array_equal(z, P.noise(77, gid0, 9, draw_id, d, mode="f32")[0])
        assert np.array_equal(F.latent(77, gid0, 9, draw_id, d, rows=[0, 8]), z[[0, 8]])
    # coordinate j is element j % 4 of quad j / 4 whatever d is; the particle index wraps at 2^64
    assert np.array_equal(F.latent(77, gid0, 4, draw_id, 9)[:, :5], F.latent(77, gid0, 4, draw_id, 5))
    assert np.array_equal(F.latent(77, 2**64 - 1, 2, draw_id, 4)[1], F.latent(77, 0, 1, draw_id, 4)[0])


@pytest.mark.parametrize("bug", F.BUGS)
@pytest.mark.parametrize("key,n", [(("coupling", 18, 2, 32), 33), (("maf", 17, 2, 32), 257), (("coupling", 66, 2, 32), 17), (("maf", 65, 2, 32), 129),
                                   (("coupling", 10, 2, 64), 33)])
def test_every_planted_defect_is_caught_by_the_device_comparison(key, n, bug):
    """A draw whose latent carries one of BUGS, through the exact fp64 inverse: compare_draw at the device tests' tolerance (fp32
    rows: the wider one) refuses it; the unperturbed draw, rounded to float32, passes."""
    wide = key in F.WIDE and key[1] == 10
    p = F.pool(*key, wide=wide)
    kind = F.shape_of(p.flow)[0]
    gid0, draw_id = F.DRAW_KEYS[1]
    x_ref, _ = F.draw_ref(p.flow, F.latent(F.DRAW_SEED, gid0, n, draw_id, key[1]))
    tol = F.x_tolerance(p)
    assert F.compare_draw(x_ref.astype(np.float32), x_ref, tol, f32=True) <= 1.0
    x_bug, _ = F.draw_ref(p.flow, F.latent(F.DRAW_SEED, gid0, n, draw_id, key[1], bug=bug, kind=kind))
    with pytest.raises(AssertionError):
        F.compare_draw(x_bug, x_ref, tol, f32=True)
    if bug == "ragged_last":  # one row is enough, and it is the last
        assert np.array_equal(x_bug[:-1], x_ref[:-1])


def test_position_tolerance_is_far_below_what_a_defect_moves():
    """MULT x XI32 through the flow's sensitivity plus 4 x the module's inversion error: a few 1e-5 of a coordinate's scale."""
    for key, dt, wide, n, _ in F.draw_cases():
        if n != F.N_CASE or dt != "f64":
            continue
        p = F.pool(*key, dtype=dt, wide=wide)
        t = F.x_tolerance(p) / p.flow.scale.double().numpy()
        assert np.all(t > P.MULT * P.XI32 * 0.5) and np.all(t < 1e-3), (p.label, t.min(), t.max())


def test_density_comparison_catches_an_error_of_a_few_fp32_roundings():
    p = F.pool("coupling", 18, 2, 32)
    F.check_errors(F.err(F.module(p.flow, p.x), p.ref), F.yardstick(p), F.DENSITY_FLOOR, "the module itself")
    off = p.ref * (1.0 + 3e-6)
    with pytest.raises(AssertionError):
        F.check_errors(F.err(off, p.ref), F.yardstick(p), F.DENSITY_FLOOR, "3e-6 relative")
    one = p.ref.copy()
    one[77] += 3e-6 * max(abs(one[77]), 1.0)
    with pytest.raises(AssertionError):
        F.check_errors(F.err(one, p.ref), F.yardstick(p), F.DENSITY_FLOOR, "one row")
    F.RECORD.clear()


def test_planted_rows():
    p = F.pool("maf", 17, 2, 32)
    x, big = F.plant(p.x[:257], p.flow, hs=True)
    ref = F.judge(p.flow, x)
    assert big == 103 and np.all(np.isnan(ref[100:103])) and np.isfinite(ref[103]) and np.all(np.isfinite(np.delete(ref, [100, 101, 102])))
    z = (x[103] - p.flow.loc.double().numpy()) / p.flow.scale.double().numpy()
    assert np.all(np.abs(z) >= 5e5) and F.plant(p.x[:257], p.flow, hs=False)[1] is None
    assert np.array_equal(np.delete(x, [100, 101, 102, 103], axis=0), np.delete(p.x[:257], [100, 101, 102, 103], axis=0))


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_pack_sizes_are_the_librarys(lib):
    for kind, floats in ((F.COUPLING, lib.asmc_coupling_pack_floats), (F.MAF, lib.asmc_maf_pack_floats)):
        for d in range(0, 131):
            for hidden in (16, 32, 64, 128, 256):
                assert lib.asmc_flow_layout(kind, d, hidden) == F.layout(kind, d, hidden), (kind, d, hidden)
                for n_layers in (1, 3):
                    assert floats(d, n_layers, hidden) == F.pack_floats(kind, d, n_layers, hidden), (kind, d, n_layers, hidden)


def test_routing_table():
    """The table of tests/test_gpu_flow_kernels.py's header, row by row."""
    C, M = F.COUPLING, F.MAF
    for d in range(2, 33, 2):  # layout 0 coupling: H = 16 for every supported d
        for W in (32, 64, 128):
            assert F.route(C, d, W, "logprob", "d") == ("k_coupling_logprob", f"Li16ELi{W}EdLi512ELi1ELb1E")
            assert F.route(C, d, W, "logprob", "f", math="f32") == ("k_coupling_logprob", f"Li16ELi{W}EfLi512ELi1ELb0E")
            assert F.route(C, d, W, "logprob", "d", tpw=2) == ("k_coupling_logprob", f"Li16ELi{W}EdLi512ELi{2 if W <= 64 else 1}ELb{int(W > 64)}E")
            assert F.route(C, d, W, "sample", "f") == ("k_coupling_sample", f"Li16ELi{W}EfLi512E")
            assert F.route(C, d, W, "sample", "f", math="f32") is None
    for d in range(1, 33):  # layout 0 autoregressive: H = 32, widths 32 and 64 (width 128 takes layout 1 at any d)
        for W in (32, 64):
            assert F.route(M, d, W, "logprob", "f") == ("k_maf_logprob", f"Li32ELi{W}EfLi512ELb1E")
            assert F.route(M, d, W, "logprob", "d", math="f32") == ("k_maf_logprob", f"Li32ELi{W}EdLi512ELb0E")
            assert F.route(M, d, W, "sample", "d") == ("k_maf_sample", f"Li32ELi{W}EdLi512E")
            assert F.route(M, d, W, "sample", "d", math="f32") is None
        assert F.route(M, d, 128, "logprob", "d") == ("k_flow16_logprob", "Li1ELi64ELi128EdLi512E")
    for kind, dims in ((C, range(34, 129, 2)), (M, range(33, 129))):  # layout 1
        for d in dims:
            for W in (32, 64, 128):
                D = 64 if d <= 64 else 128
                assert F.route(kind, d, W, "logprob", "f") == ("k_flow16_logprob", f"Li{kind}ELi{D}ELi{W}EfLi512E")
                assert F.route(kind, d, W, "sample", "d") == ("k_flow16_sample", f"Li{kind}ELi{D}ELi{W}EdLi512E")
                assert F.route(kind, d, W, "logprob", "f", math="f32") is None and F.route(kind, d, W, "sample", "f", math="f32") is None
    assert F.route(C, 33, 64, "logprob") is None and F.route(C, 130, 64, "logprob") is None and F.route(M, 129, 64, "sample") is None
    t = F.reachable()
    assert len(t) == 16 + 6 + 8 + 4 + 24 + 24
    # compiled, never launched: the H = 32 coupling instantiations (flow_supported admits d <= 32, flow_half_pad then gives 16) and the
    # width-128 autoregressive ones of layout 0
    assert not any(k[0].startswith("k_coupling") and k[1].startswith("Li32E") for k in t)
    assert not any(k[0].startswith("k_maf") and "Li128E" in k[1] for k in t)


def test_every_reachable_instantiation_has_a_case():
    """What the device module's closing census expects to have seen, from the case tables alone."""
    seen = set()
    for key, dt, wide, n, math in F.density_cases():
        seen.add(F.route(F.COUPLING if key[0] == "coupling" else F.MAF, key[1], key[3], "logprob", "d" if dt == "f64" else "f", math))
    for key, dt, wide, n, _ in F.draw_cases():
        seen.add(F.route(F.COUPLING if key[0] == "coupling" else F.MAF, key[1], key[3], "sample", "d" if dt == "f64" else "f"))
    for key, dt in F.TPW_CASES:  # the ASMC_FLOW_TPW=2 child
        seen.add(F.route(F.COUPLING, key[1], key[3], "logprob", "d" if dt == "f64" else "f", tpw=2))
    assert None not in seen
    assert seen == F.reachable(), sorted(F.reachable() - seen)


def test_rows_per_round_restates_the_launch_arithmetic():
    cu = MI355X_CUS
    rpr = lambda k, key: F.rows_per_round(k, F.build_flow(*key), cu)  # noqa: E731
    assert F.coupling_resident(4, 64) and F.coupling_resident(5, 64) and not F.coupling_resident(6, 64)
    assert F.coupling_resident(1, 128) and not F.coupling_resident(2, 128)
    assert rpr("k_coupling_logprob", ("coupling", 32, 2, 64)) == cu * 2 * 256   # 57 KB resident: two blocks per CU
    assert rpr("k_coupling_logprob", ("coupling", 32, 4, 64)) == cu * 256       # 115 KB resident: one
    assert rpr("k_coupling_logprob", ("coupling", 32, 6, 64)) == cu * 2 * 256   # streamed, 29 KB per layer
    assert rpr("k_coupling_logprob", ("coupling", 32, 2, 128)) == cu * 256      # streamed, 89 KB per layer
    assert F.rows_per_round("k_coupling_logprob", F.build_flow("coupling", 32, 2, 64), cu, tpw=2) == cu * 2 * 512
    assert rpr("k_coupling_sample", ("coupling", 32, 4, 64)) == cu * 256
    assert rpr("k_maf_logprob", ("maf", 32, 3, 64)) == cu * 256 and rpr("k_maf_sample", ("maf", 17, 2, 32)) == cu * 2 * 256
    assert rpr("k_flow16_logprob", ("coupling", 66, 2, 32)) == rpr("k_flow16_sample", ("maf", 12, 2, 128)) == cu * 2 * 128
    for name, (key, dt) in F.SECOND_ROUND.items():
        assert rpr(name.split()[0], key) + F.TAIL <= 150_000  # fp64 references stay within seconds
