"""Flow mutations of a d without kernels of its own (csrc/asmc_pcn_drive.hip, asmc_pcn_mutate_flow): the state is copied into
zero-padded rows of the next supported width, the one-kernel step runs on the copy - always deferred - the rows are copied
back, and only then does the blocking form wait for the read-back (pcn_flow_padded_tail).  A coupling flow at d = 20 runs
padded to 32 on k_pcn_flow_fused, at d = 40 padded to 64 on k_pcn_flow16.

Each case runs the blocking call and the deferred pair (enqueue, another library launch behind it, result) on equal inputs
and compares x, ll, lp, lq, the accept counts and the step-size history with `torch.equal` / `array_equal`; each call pads
once, un-pads once and launches its step kernel once per step.  n = 64 * 4 + 29: several 64-particle tiles and a ragged last
one; three steps with the step-size adaptation on; f64 state.
"""
import pytest

from test_gpu_fused_stage_image import COUPLING, N_SMALL, N_STEPS, _assert_same, _flow, _mutate, _population, _reference, _targets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from aspire_amd.engine import HipEngine

    return HipEngine(0, n_max=4096, d_max=64)


@pytest.mark.parametrize("d,step_kernel", [(20, "k_pcn_flow_fused"), (40, "k_pcn_flow16")], ids=["d20-fused", "d40-flow16"])
def test_padded_flow_mutation_blocking_equals_deferred(eng, monkeypatch, d, step_kernel):
    dev = _flow(eng, COUPLING, d, 3, 64)
    ref, (t_ll, t_lp) = _reference(eng, d, 61), _targets(eng, d, 1, 62)
    pop = _population(eng, N_SMALL, d, "f64", dev, t_ll, t_lp, 63)
    blocking, rep_b = _mutate(eng, monkeypatch, "image", pop, 0.4, ref, t_ll, t_lp, dev, "f64", profile=True)
    deferred, rep_d = _mutate(eng, monkeypatch, "image", pop, 0.4, ref, t_ll, t_lp, dev, "f64", deferred=True, profile=True)
    _assert_same(deferred, blocking, f"d = {d}: deferred vs blocking")
    for rep in (rep_b, rep_d):
        assert rep["k_pad_rows"][0] == 1 and rep["k_unpad_rows"][0] == 1 and rep[step_kernel][0] == N_STEPS, sorted(rep)
    # every step moved some particles and not all (so does _assert_same over the call); the moves reached the caller's rows
    assert all(0 < a < N_SMALL for a in blocking[4]), blocking[4]
    assert (blocking[0] != pop[0]).any()
