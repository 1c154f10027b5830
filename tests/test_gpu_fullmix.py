"""asmc_fullmix_logpdf on the device against the long-double restatement (tests/fullmix_ref.py), every shape and edge.

Shape -> kernel (csrc/asmc_fullmix.hip): one family, k_fullmix<T, DL, GRAD>; T = double / float rows (`d` / `f` in the symbol),
GRAD = grad_dev given (`Lb1` / `Lb0`), DL = coordinates per lane of the four lanes that own a row:

      d         DL   padded width   components staged at once (their images share 72 KB of LDS)
    1 ..   4     1        4         all
    5 ..   8     2        8         all
    9 ..  16     4       16         all
   17 ..  32     8       32         all
   33 ..  64    16       64         4: C = 5, 8 take two groups, the rows' running (max, sum) waiting in LDS in between
   65 .. 128    32      128         1: every C > 1 takes C groups over batches of 8 tiles
  d > 128 or C > 8: ASMC_ERR_UNSUPPORTED, nothing launched.

x at a 16-byte aligned address with 16-byte rows is copied with 16-byte loads, otherwise with 8- or 4-byte loads (offset views).
More than 1024 tiles of 64 rows (n = 70001) make the blocks stride over the grid.

Every case asserts from profile_variants() that its instantiation ran, prints its worst error in units of the tolerance, compares
every finite element and requires the restatement's non-finite pattern exactly.
"""
import numpy as np
import pytest
import torch

import fullmix_ref as R

pytestmark = pytest.mark.gpu


def dl_of(d):
    return next(k for k, w in ((1, 4), (2, 8), (4, 16), (8, 32), (16, 64), (32, 128)) if d <= w)


def symbol(dtype, d, grad):
    t = "d" if dtype in (np.float64, torch.float64) else "f"
    return f"k_fullmixI{t}Li{dl_of(d)}ELb{int(grad)}EE"


def run_both(eng, target, x_dev):
    """(value without grad, value with grad, grad) and the census of the two launches."""
    tab = target.device_tables(eng)
    eng.profile(True)
    eng.profile_variants()
    v0 = eng.fullmix_logpdf(x_dev, tab)
    v1, g = eng.fullmix_logpdf(x_dev, tab, want_grad=True)
    census = eng.profile_variants()
    eng.profile(False)
    return v0.cpu().numpy(), v1.cpu().numpy(), g.cpu().numpy(), census


def check_case(eng, target, x, what, x_dev=None):
    dtype = x.dtype.type
    x_dev = eng.asarray(x, dtype=torch.float64 if dtype == np.float64 else torch.float32) if x_dev is None else x_dev
    ref = R.reference(target, x)
    v0, v1, g, census = run_both(eng, target, x_dev)
    for grad in (False, True):
        want = symbol(dtype, target.dims, grad)
        assert sum(c for k, c in census.items() if want in k) == 1, (want, census)
    assert len(census) == 2, census
    assert np.array_equal(v0.view(np.int64), v1.view(np.int64)), f"{what}: the value's bits depend on grad_dev"
    wv, wg = R.compare(ref, v1, g)
    fin = np.isfinite(ref["value"])
    print(f"{what}: n={len(x)} value tol median {np.median(ref['tol_value'][fin]):.3g} worst error {wv:.3f} tol; "
          f"gradient tol median {np.median(ref['tol_grad'][fin]):.3g} worst error {wg:.3f} tol; "
          f"{int((~fin).sum())} non-finite rows match")
    assert wv < 1.0 and wg < 1.0, (what, wv, wg)
    return wv, wg


GRID = R.grid()


@pytest.mark.parametrize("case", range(len(GRID)), ids=[f"d{c[0]}-C{c[1]}-cond{c[2]:g}-{c[3]}-{'box' if c[4] else 'free'}-{c[5].__name__}"
                                                        for c in GRID])
def test_grid(hip_engine, case):
    """Every d x every C, both condition numbers, bounds, fp64 / fp32 rows, flat and singular components (the rotation of
    fullmix_ref.grid), with the rows of the non-finite contract and of the box's edges appended to each."""
    d, C, cond, kind, bounds, dtype, n = GRID[case]
    t, _ = R.make_target(d, C, cond, seed=7, kind=kind, bounds=bounds)
    x = np.concatenate([R.make_rows(t, n, seed=11, dtype=dtype), R.special_rows(t, dtype)])
    check_case(hip_engine, t, x, f"grid d={d} C={C} cond={cond:g} {kind} bounds={bounds} {dtype.__name__}")


@pytest.mark.parametrize("d,C,dtype", [(3, 2, np.float64), (32, 2, np.float32), (64, 5, np.float64), (128, 2, np.float64)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5003])
def test_row_counts(hip_engine, n, d, C, dtype):
    """Tile edges: one row, one short of / exactly / one past a tile of 64, several tiles, many tiles with a ragged end."""
    t, _ = R.make_target(d, C, 1e6 if d == 32 else 1.0, seed=5, kind="plain", bounds=(d == 3))
    check_case(hip_engine, t, R.make_rows(t, n, seed=n, dtype=dtype), f"rows n={n} d={d} C={C} {dtype.__name__}")


def test_grid_stride(hip_engine):
    """n = 70001 at d = 32: 1094 tiles for at most 1024 blocks."""
    t, _ = R.make_target(32, 1, 1.0, seed=3, kind="plain", bounds=True)
    check_case(hip_engine, t, R.make_rows(t, 70001, seed=1), "grid stride n=70001 d=32")


@pytest.mark.parametrize("d,dtype,shift", [(3, np.float64, "row"), (3, np.float32, "row"), (31, np.float32, "row"), (31, np.float64, "row"),
                                           (32, np.float64, "element"), (33, np.float32, "element"), (65, np.float64, "row")])
def test_offset_views(hip_engine, d, dtype, shift):
    """x contiguous [n, d] at an address that is only element-aligned: a view that starts one row in with odd d, or one
    element into a flat buffer."""
    n = 130
    t, _ = R.make_target(d, 2, 1.0, seed=9, kind="plain", bounds=True)
    x = R.make_rows(t, n, seed=2, dtype=dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    if shift == "row":
        buf = torch.zeros((n + 1, d), dtype=tdt, device=hip_engine.device)
        buf[1:] = torch.as_tensor(x)
        xv = buf[1:]
    else:
        buf = torch.zeros(n * d + 1, dtype=tdt, device=hip_engine.device)
        buf[1:] = torch.as_tensor(x).reshape(-1)
        xv = buf[1:].view(n, d)
    assert xv.is_contiguous() and xv.data_ptr() % 16 != 0
    check_case(hip_engine, t, x, f"offset view d={d} {dtype.__name__} {shift}", x_dev=xv)


def test_unsupported_shapes_launch_nothing(hip_engine):
    """d = 129 and C = 9: ASMC_ERR_UNSUPPORTED (-4) before anything is launched."""
    from aspire_amd._lib import ASMC_ERR_UNSUPPORTED, AsmcError

    eng = hip_engine
    for d, C in ((129, 1), (4, 9)):
        tab = eng.make_fullmix(np.zeros(C), np.zeros((C, d)), np.tile(np.eye(d), (C, 1, 1)))
        x = eng.asarray(np.zeros((10, d)))
        eng.profile(True)
        eng.profile_variants()
        for want_grad in (False, True):
            with pytest.raises(AsmcError, match=f"rc={ASMC_ERR_UNSUPPORTED}"):
                eng.fullmix_logpdf(x, tab, want_grad=want_grad)
        assert eng.profile_variants() == {}
        eng.profile(False)


def test_evaluate_falls_back_beyond_the_kernels(hip_engine, caplog):
    """A shape the kernels refuse is evaluated by __call__, with one logger.info per instance."""
    import logging

    from aspire_amd import GaussianMixture

    d = 130
    t = GaussianMixture(np.zeros(d), np.eye(d))
    x = hip_engine.asarray(np.random.default_rng(0).normal(size=(5, d)))
    with caplog.at_level(logging.INFO, logger="aspire_amd.targets"):
        a = t.evaluate(hip_engine, x)
        b = t.evaluate(hip_engine, x)
    assert torch.equal(a, b) and torch.equal(a, t(x))
    assert sum("no kernel" in r.getMessage() for r in caplog.records) == 1
    # a gradient at more than 64 dimensions stays on the array ops (the kernel measured slower there); the value takes the kernel
    t2, _ = R.make_target(100, 2, 1.0, seed=1)
    x2 = hip_engine.asarray(R.make_rows(t2, 70, seed=1))
    hip_engine.profile(True)
    hip_engine.profile_variants()
    with caplog.at_level(logging.INFO, logger="aspire_amd.targets"):
        val = t2.evaluate(hip_engine, x2.clone().requires_grad_(True))
        t2.evaluate(hip_engine, x2.clone().requires_grad_(True))
    assert hip_engine.profile_variants() == {} and val.requires_grad
    assert sum("gradients above 64 dimensions" in r.getMessage() for r in caplog.records) == 1  # its own message, once
    assert sum("no kernel" in r.getMessage() for r in caplog.records) == 1  # (still only the first target's)
    t2.evaluate(hip_engine, x2)
    census = hip_engine.profile_variants()
    hip_engine.profile(False)
    assert len(census) == 1 and symbol(np.float64, 100, False) in next(iter(census)), census


@pytest.mark.parametrize("d", [8, 64])
def test_autograd_function(hip_engine, d):
    """GaussianMixture.evaluate on a tensor that requires grad: ONE launch (the gradient instantiation), and torch.autograd.grad
    of a weighted sum is the weights times the restatement's gradient."""
    eng = hip_engine
    t, _ = R.make_target(d, 4, 1.0, seed=21, kind="plain", bounds=True)
    x = np.concatenate([R.make_rows(t, 200, seed=4), R.special_rows(t)])
    ref = R.reference(t, x)
    w = np.random.default_rng(1).uniform(0.5, 2.0, size=len(x))
    xd = eng.asarray(x).requires_grad_(True)
    eng.profile(True)
    eng.profile_variants()
    val = t.evaluate(eng, xd)
    census = eng.profile_variants()
    eng.profile(False)
    assert len(census) == 1 and symbol(np.float64, d, True) in next(iter(census)) and sum(census.values()) == 1, census
    wd = eng.asarray(w)
    total = torch.where(torch.isfinite(val), wd * val, torch.zeros_like(val)).sum()
    (g,) = torch.autograd.grad(total, xd)
    wv, _ = R.compare(ref, val.detach().cpu().numpy())
    fin = np.isfinite(ref["value"])
    got = g.cpu().numpy()
    assert np.all(got[~fin] == 0.0)
    # w * G: one more rounding of the product, within the 4 ulp of the gradient's tolerance
    scaled = dict(ref, grad=ref["grad"] * w[:, None], tol_grad=ref["tol_grad"] * w[:, None])
    _, wg = R.compare(scaled, val.detach().cpu().numpy(), got)
    print(f"autograd d={d}: worst value error {wv:.3f} tol, worst gradient error {wg:.3f} tol")
    assert wv < 1.0 and wg < 1.0
    v2, g2 = t.evaluate(eng, xd.detach(), grad=True)  # the explicit form: the same launch, the same bits
    assert np.array_equal(v2.cpu().numpy().view(np.int64), val.detach().cpu().numpy().view(np.int64))
    assert np.array_equal((g2.cpu().numpy() * w[:, None])[fin], got[fin])
