"""The chain recorder (csrc/asmc_chain.hip; include/asmc.h asmc_chain_record / asmc_chain_set / asmc_chain_clear) on the HIP engine.

Shapes: n in {7, 257} (less than a tile; more than one block, a ragged last tile), d in {3, 8, 32, 33}, 5 steps, fp32 and fp64.
For each of the pCN dispatch paths the recorder serves -

  mutate   asmc_pcn_mutate with a chain target set on the context, every d: the register kernels on the coordinate-major
           whitened state, on the row-major one (ASMC_PCN_AOS) and on x itself (ASMC_PCN_XSTATE, as calls of fewer than 4 steps),
           d = 3 zero-padded to them, d = 33 zero-padded to the matrix-core kernels; pCN and tpCN;
  ysplit   the asmc_pcn_ysplit_* session, recorded from the session's state (d in {8, 32});
  generic  asmc_pcn_propose / asmc_pcn_accept, recorded from the rows (every d), also as a chain in z = T(x) with a logit
           transform on two coordinates, whose slots hold T^-1(z)

- the checks are: no change without a target (before a set, after a clear, and on a context that never saw one), no disturbance
with one, every slot equal bit for bit to what an independent run of t + 1 steps of the parent entry points returns, and guard
slots and pitch padding untouched.  The stretch move is checked against tests/stretch_ref.py the
way tests/test_gpu_emcee_smc.py checks its kernels, and against the device's own rows.
"""

import numpy as np
import pytest
import torch

import stretch_ref as S

pytestmark = pytest.mark.gpu

STEPS = 5
NS, DS, DTS = (7, 257), (3, 8, 32, 33), ("f32", "f64")
REG = (8, 32)  # widths with register-resident kernels among DS


@pytest.fixture(scope="module")
def eng(hip_engine):
    return hip_engine


@pytest.fixture(scope="module")
def fresh():
    """A context on which no chain target is ever set."""
    from aspire_amd.engine import HipEngine

    e = HipEngine(0, n_max=1 << 12, d_max=128)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A HIP fault is sticky: end the session there instead of running on."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device fault: {exc}", returncode=3)


def tdt(dt):
    return torch.float64 if dt == "f64" else torch.float32


def problem(n, d, dt, device):
    """Walkers, a reference Gaussian with a dense factor, single-component targets for the built-in path."""
    g = np.random.default_rng(1000 * n + 10 * d + (dt == "f32"))
    a = g.normal(size=(d, d)) / np.sqrt(d)
    L = np.linalg.cholesky(a @ a.T + 0.5 * np.eye(d))
    mu = 0.3 * g.normal(size=d)
    x = (mu + g.normal(size=(n, d)) @ L.T)
    to = lambda v, t=torch.float64: torch.as_tensor(np.ascontiguousarray(v)).to(device=device, dtype=t)  # noqa: E731
    mixes = [(np.array([0.0]), 0.2 * g.normal(size=(1, d)), 1.0 + g.random(size=(1, d))) for _ in range(3)]
    return dict(n=n, d=d, x=to(x, tdt(dt)), mu=to(mu), L=to(np.tril(L)), Linv=to(np.tril(np.linalg.inv(L))), mixes=mixes, seed=977 + n + d, nu=0.0)


def torch_densities(x):
    """(ll, lp) of rows on the device (the callables of the split paths), with a hole of -inf."""
    x = x.double()
    q = (x * x).sum(1)
    ll = torch.where(x[:, 0] > 1.2, torch.full_like(q, -np.inf), -0.5 * q)
    return ll, -0.1 * x[:, 1 % x.shape[1]]


def start(P, T=None, eng=None):
    x = P["x"].clone()
    ll, lp = torch_densities(x)
    lq = torch.zeros_like(ll)
    if T is None:
        return x, ll, lp, lq, None
    z, lj = eng.transform_forward(x, T)
    return z, ll, lp, lq, eng.transform_inverse(z, T)[1]


def run_mutate(e, P, steps, chain=None):
    x = P["x"].clone()
    dm = [e.make_mixture(*m) for m in P["mixes"]]
    ll, lp, lq = (e.mixture_logpdf(x, m) for m in dm)
    if chain is not None:
        e.chain_set(chain, 0, 1)
    try:
        n_acc, hist, rho = e.pcn_mutate(x, ll, lp, lq, 1.0, P["mu"], P["L"], P["Linv"], dm[0], dm[1], dm[2], P["seed"], 0, 0.4, steps, 0,
                                        0.234, 1, "f64", P["nu"])
    finally:
        if chain is not None:
            e.chain_clear()
    return dict(x=x, ll=ll, lp=lp, lq=lq, n_acc=n_acc, hist=hist, rho=rho)


def run_ysplit(e, P, steps, chain=None):
    x, ll, lp, lq, _ = start(P)
    sess = e.pcn_ysplit_begin(x, 1.0, P["mu"], P["L"], P["Linv"], P["seed"], 0, 0.4, 0.234, True, P["nu"], "f64")
    assert sess is not None
    zeros = torch.zeros_like(ll)
    for t in range(steps):
        xp = e.pcn_ysplit_propose(sess, t)
        ll_new, lp_new = torch_densities(xp)
        e.pcn_ysplit_accept(sess, t, ll, lp, lq, ll_new, lp_new, zeros, P["n"], t)
        if chain is not None:
            e.chain_record(chain, t, sess=sess, ll=ll, lp=lp)
    n_acc, hist, rho = e.pcn_ysplit_end(sess, steps)
    return dict(x=x, ll=ll, lp=lp, lq=lq, n_acc=n_acc, hist=hist, rho=rho)


def run_generic(e, P, steps, chain=None, T=None):
    z, ll, lp, lq, lj = start(P, T, e)
    zeros = torch.zeros_like(ll)
    e.pcn_split_begin(0.4)
    for t in range(steps):
        zp, q0, q1 = e.pcn_propose(z, P["mu"], P["L"], P["Linv"], 0.0, P["seed"], 0, t, nu=P["nu"])
        xp, lj_new = (zp, None) if T is None else e.transform_inverse(zp, T)
        ll_new, lp_new = torch_densities(xp)
        e.pcn_accept(z, zp, ll, lp, lq, ll_new, lp_new, zeros, q0, q1, 1.0, P["seed"], 0, t, logj_old=lj, logj_new=lj_new, want_count=False)
        e.pcn_split_adapt(P["n"], 0.234, t, True)
        if chain is not None:
            e.chain_record(chain, t, x=z, ll=ll, lp=lp, transform=T)
    n_acc, hist, rho = e.pcn_split_end(steps)
    x = z if T is None else e.transform_inverse(z, T, want_logj=False)[0]  # what the sampler returns: rows in x space
    return dict(x=x, ll=ll, lp=lp, lq=lq, n_acc=n_acc, hist=hist, rho=rho)


def same(a, b, what):
    for k in ("x", "ll", "lp", "lq"):
        ta, tb = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert ta.tobytes() == tb.tobytes(), f"{what}: {k} differs"
    assert np.array_equal(a["n_acc"], b["n_acc"]) and np.array_equal(a["hist"], b["hist"]) and a["rho"] == b["rho"], f"{what}: counts / step sizes"


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class Guarded:
    """A chain with one guard slot on either side and `extra` elements of pitch padding behind every row, all filled with a NaN
    pattern; `chain` is the DeviceChain over the slots in between."""

    def __init__(self, e, n_slots, n, d, dtype, extra=0):
        from aspire_amd.engine import DeviceChain

        self.extra, self.d = extra, d
        self.x = torch.full((n_slots + 2, n, d + extra), float("nan"), dtype=dtype, device=e.device)
        self.ll = torch.full((n_slots + 2, n), float("nan"), dtype=torch.float64, device=e.device)
        self.lp = self.ll.clone()
        self.fill_x, self.fill_s = bits(self.x[0])[0, 0].item(), bits(self.ll[0])[0].item()
        self.chain = DeviceChain(self.x[1:-1, :, :d], self.ll[1:-1], self.lp[1:-1])

    def intact(self):
        torch.cuda.synchronize()
        for s in (0, -1):
            assert bool((bits(self.x[s]) == self.fill_x).all()), "a guard slot of the rows was written"
            assert bool((bits(self.ll[s]) == self.fill_s).all()) and bool((bits(self.lp[s]) == self.fill_s).all()), "a guard slot of the densities"
        if self.extra:
            assert bool((bits(self.x[:, :, self.d:]) == self.fill_x).all()), "the padding beyond d was written"
        assert not bool(torch.isnan(self.chain.x).any()), "a row of the chain was not written"


def check_path(eng, fresh, P, dt, run, extra=0, slots=range(STEPS), **kw):
    g = Guarded(eng, STEPS, P["n"], P["d"], tdt(dt), extra)
    before = run(eng, P, STEPS, **kw)
    same(before, run(fresh, P, STEPS, **kw), "without a target, against a fresh context")
    with_target = run(eng, P, STEPS, chain=g.chain, **kw)
    g.intact()
    same(before, with_target, "with a target")
    same(before, run(eng, P, STEPS, **kw), "after asmc_chain_clear")
    for t in slots:
        r = run(eng, P, t + 1, **kw)
        assert g.chain.x[t].contiguous().cpu().numpy().tobytes() == r["x"].cpu().numpy().tobytes(), f"slot {t}: rows"
        assert g.chain.ll[t].cpu().numpy().tobytes() == r["ll"].cpu().numpy().tobytes(), f"slot {t}: log-likelihood"
        assert g.chain.lp[t].cpu().numpy().tobytes() == r["lp"].cpu().numpy().tobytes(), f"slot {t}: log-prior"
    return g, with_target


def check_whitened_slots(eng, P, g, n_acc):
    """The slots of asmc_pcn_mutate's register-kernel whitened loop that no parent run reaches (a parent call of fewer than 4 steps
    steps on x).  (1) The recorded densities belong to the recorded rows: the built-in density of the stored row in numpy fp64.
    Both evaluations sum d products in fp64 from the same stored row; with S = |log w| + sum |t^2 prec| / 2 each is within
    (d + 2) eps S of the exact value, so they differ by at most twice that; the bound used is 4 (d + 2) eps S.  (2) A row changes
    between two slots exactly where its proposal was accepted - an unchanged y un-whitens to the same bits, an accepted one never to
    the same row - so the number of changed rows is the step's accept count."""
    d, eps = P["d"], np.finfo(np.float64).eps
    for t in range(STEPS):
        rows = g.chain.x[t].contiguous().cpu().numpy().astype(np.float64)
        for k, rec in ((0, g.chain.ll[t]), (1, g.chain.lp[t])):
            logw, mu, prec = P["mixes"][k]
            terms = (rows - mu[0]) ** 2 * prec[0]
            want, S = logw[0] - 0.5 * terms.sum(1), abs(logw[0]) + 0.5 * terms.sum(1)
            assert np.all(np.abs(rec.cpu().numpy() - want) <= 4 * (d + 2) * eps * S), f"slot {t}: density {k} is not the recorded row's"
        if t:
            prev = g.chain.x[t - 1].contiguous().cpu().numpy()
            assert int(np.any(g.chain.x[t].contiguous().cpu().numpy() != prev, axis=1).sum()) == int(n_acc[t]), f"slot {t}: moved rows"


@pytest.mark.parametrize("nu", [0.0, 5.0], ids=["pcn", "tpcn"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("state", ["whitened", "x", "aos"])
def test_mutate_target(eng, fresh, monkeypatch, state, n, d, dt, nu):
    """asmc_pcn_mutate's own loop on every state it keeps: d = 8, 32 on the register kernels, d = 3 zero-padded to them, d = 33
    zero-padded to the matrix cores' 64.  The register kernels' whitened loops (coordinate-major; row-major under ASMC_PCN_AOS)
    serve calls of 4 steps and more, so there slots 3 and 4 have a parent run to equal and slots 0 to 2 get check_whitened_slots;
    on x itself (ASMC_PCN_XSTATE: the loop every short call takes) and on the matrix cores (whitened at any length) all five do."""
    if state != "whitened":
        monkeypatch.setenv("ASMC_PCN_XSTATE" if state == "x" else "ASMC_PCN_AOS", "1")
    P = problem(n, d, dt, eng.device)
    P["nu"] = nu
    short_calls_differ = state != "x" and d != 33
    g, r = check_path(eng, fresh, P, dt, run_mutate, slots=(3, 4) if short_calls_differ else range(STEPS))
    if short_calls_differ:
        check_whitened_slots(eng, P, g, r["n_acc"])


@pytest.mark.parametrize("nu", [0.0, 5.0], ids=["pcn", "tpcn"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", REG)
@pytest.mark.parametrize("n", NS)
def test_ysplit_session(eng, fresh, n, d, dt, nu):
    P = problem(n, d, dt, eng.device)
    P["nu"] = nu
    check_path(eng, fresh, P, dt, run_ysplit)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_generic_rows(eng, fresh, n, d, dt):
    """Rows as they are: back to back (whole 16-byte vectors where d allows), 3 elements of padding (element-wise), 16 bytes of
    padding (pitched vectors)."""
    P = problem(n, d, dt, eng.device)
    for extra in (0, 3, 4 if dt == "f32" else 2):
        check_path(eng, fresh, P, dt, run_generic, extra=extra)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_generic_rows_under_a_logit_transform(eng, fresh, n, d, dt):
    """The chain runs in z = T(x), logit on coordinates 0 and 2 of a box [-6, 6]; slot t holds T^-1(z) by the transform's kernel."""
    P = problem(n, d, dt, eng.device)
    kind = np.zeros(d, dtype=np.int32)
    kind[[0, 2]] = 1
    lower, upper = np.full(d, -6.0), np.full(d, 6.0)
    P["x"] = P["x"].clamp(-5.0, 5.0)

    def run(e, P, steps, chain=None):
        T = e.make_transform(kind, np.zeros(d, dtype=np.int32), lower, upper, None, None, 1e-6, float(-2 * np.log(12.0)), 0.0)
        return run_generic(e, P, steps, chain=chain, T=T)

    check_path(eng, fresh, P, dt, run)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_stretch_move(eng, n, d, dt):
    """chain[t] after t + 1 full steps: the device's own rows bit for bit, and tests/stretch_ref.py's restatement the way
    tests/test_gpu_emcee_smc.py compares one step - proposals bit for bit, logf within its ulp bound, decisions restated from the
    device's logf, rows then exactly."""
    P = problem(n, d, dt, eng.device)
    g = Guarded(eng, STEPS, n, d, tdt(dt), extra=0 if n == 7 else 3)
    x = P["x"].clone()
    xh = x.cpu().numpy().copy()

    def dens(y64):
        q = (y64 * y64).sum(1)
        return -0.5 * q, -0.1 * y64[:, 0], np.zeros_like(q)

    ll, lp, lq = dens(xh.astype(np.float64))
    lld, lpd, lqd = (torch.from_numpy(v.copy()).to(eng.device) for v in (ll, lp, lq))
    seed, a = 0x5EED0123, 2.0
    for t in range(STEPS):
        for h in (0, 1):
            y, logf = eng.stretch_propose(x, h, a, seed, 0, t, t)
            y_ref, logf_ref, _, _ = S.propose(xh, h, a, seed, 0, t)
            y_h, logf_h = y.cpu().numpy(), logf.cpu().numpy()
            assert np.array_equal(y_h, y_ref)
            t1 = logf_ref / max(d - 1, 1)
            assert np.all(np.abs(logf_h - logf_ref) <= (d - 1) * np.spacing(np.abs(t1)) + np.spacing(np.abs(logf_ref)))
            new = dens(y_h.astype(np.float64))
            eng.stretch_accept(x, h, y, logf, 1.0, lld, lpd, lqd, *(torch.from_numpy(v.copy()).to(eng.device) for v in new), seed, 0, t, t)
            S.accept(xh, h, y_h, logf_h, 1.0, ll, lp, lq, *new, seed, 0, t)
        eng.chain_record(g.chain, t, x=x, ll=lld, lp=lpd)
        assert torch.equal(g.chain.x[t], x), f"slot {t}: the device's rows"
        assert np.array_equal(g.chain.x[t].cpu().numpy(), xh), f"slot {t}: the restatement's rows"
        assert np.array_equal(g.chain.ll[t].cpu().numpy(), ll) and np.array_equal(g.chain.lp[t].cpu().numpy(), lp)
    g.intact()
    assert not np.array_equal(g.chain.x[0].cpu().numpy(), g.chain.x[STEPS - 1].cpu().numpy())
