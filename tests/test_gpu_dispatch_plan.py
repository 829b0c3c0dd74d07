"""The plan returned is the plan run: the report words of a real forward plus backward equal what the plan queries (mcp_rollout_fwd_plan /
mcp_rollout_bwd_plan) answer for the same descriptors, sizes, flags, workspace and CU count.  Four small shapes that land in four different
forward families and three sweeps; tests/test_dispatch_plan_cpu.py replays the recorded dispatch table through the same queries without a GPU."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _workload(name):
    from gpu_helpers import dev
    from mc_pilco_amd import ops, workloads

    w = workloads.build(name, device=dev())
    return w.model, w.policy, w.cost, ops.NoiseSpec(seed=7, call=1), w.sample_x0(), w.T, w.p_drop


def _width_case(name):
    import width_models as wm

    c = wm.BY_NAME[name]
    assert c.pms is None
    model, pol, cost, nz, _meas, x0 = wm.packed(c, 16)
    return model, pol, cost, nz, x0, c.T, wm.P_DROP


@pytest.mark.parametrize("make,name", [(_workload, "tiny"), (_workload, "tiny_ur5"), (_width_case, "narrow_disjoint_d6"), (_width_case, "p17_u2_b257")])
def test_report_of_a_real_call_is_the_plan_querys_answer(make, name):
    from mc_pilco_amd import hipabi, ops

    model, pol, cost, nz, x0, T, p_drop = make(name)
    M = x0.shape[0]
    d = hipabi.DISPATCH
    assert not any(getattr(d, f[0]) for f in d._fields_ if not f[0].startswith("ran_")), "a dispatch request was left set"
    st, _inp, status = ops.rollout(model, pol, nz, x0, T, p_drop)
    c, _ = ops.expected_cost(cost, st)
    c.backward()
    assert int(status.item()) == 0
    ran = (d.ran_particles, d.ran_gp_sharded, d.ran_fwd_lean, d.ran_row_split, d.ran_bwd_lean, d.ran_bwd_pipe)
    L = hipabi.lib()
    pc = pol.bind(p_drop)  # (the descriptor the two calls were given: no measurement model in these cases)
    nbytes = L.mcp_rollout_workspace_bytes(C.byref(model.c), C.byref(pc), M, T)
    cus = torch.cuda.get_device_properties(x0.device).multi_processor_count
    fp, bp = hipabi.FwdPlan(), hipabi.BwdPlan()
    # flags: particle_pred, nothing packed yet (the first rollout on this model object)
    assert L.mcp_rollout_fwd_plan(C.byref(model.c), C.byref(pc), M, T, 1, nbytes, cus, C.byref(d), C.byref(fp)) == 0
    assert L.mcp_rollout_bwd_plan(C.byref(model.c), C.byref(pc), M, T, 1, nbytes, cus, C.byref(d), C.byref(bp)) == 0
    plan = (fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, fp.ran_row_split, bp.ran_bwd_lean, bp.ran_bwd_pipe)
    print(name, "ran", ran, "family", fp.family, "sweep", (bp.pfm, bp.um, bp.maxnt, bp.particles, bp.threads))
    assert ran == plan
    assert fp.family in (hipabi.FWD_SMALL_SHARDED, hipabi.FWD_LEAN, hipabi.FWD_TILE_SHARDED, hipabi.FWD_TILE, hipabi.FWD_SMALL)
