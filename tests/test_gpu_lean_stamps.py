"""The lean forward kernel's phase stamps are a property of the instantiation: a stamped twin runs only when the caller passes a stamp
buffer (mcp_dispatch.fwd_stamps).  It must compute exactly what the product instantiation computes, fill the buffer, and a call without
a buffer must not write to one."""
import pytest
import torch

from gpu_helpers import forced_variant
from mc_pilco_amd import hipabi, ops, workloads

pytestmark = pytest.mark.gpu

M, T = 32, 8
POISON = 0x5A5A5A5A5A5A5A5A


def _rollout(w, x0, fv):
    out = ops.rollout_forward_raw(w.model, w.policy, ops.NoiseSpec(seed=5, call=2), x0, T, w.p_drop, meas=w.meas)
    torch.cuda.synchronize()
    assert int(out[3].item()) == 0, "kernel status flags: %s" % ops.status_flags(out[3])
    fv.check(lean_expected=True)
    return out[:3] + out[4:]  # states, inputs, Jacobians (, measurements)


# one case per class of lean instantiation: SE, SE + polynomial(2), SE with the measurement model
@pytest.mark.parametrize("name", ["c1", "c2_script", "pms_script"])
def test_stamped_twin_matches_product(name):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = hipabi.lib()
    w = workloads.build(name, device=dev, M=M, T=T)
    x0 = w.sample_x0()
    buf = torch.full((64,), POISON, dtype=torch.int64, device=dev)
    with forced_variant(204) as fv:  # the lean kernel at four particles per workgroup: the instantiations that have a stamped twin
        try:
            lib.mcp_debug_set_stamp_buffer(None)
            plain = _rollout(w, x0, fv)
            assert bool((buf == POISON).all()), "a call without a stamp buffer wrote to one"
            buf.zero_()
            lib.mcp_debug_set_stamp_block(0)
            lib.mcp_debug_set_stamp_buffer(buf.data_ptr())
            stamped = _rollout(w, x0, fv)
        finally:
            lib.mcp_debug_set_stamp_buffer(None)
        assert len(plain) == (4 if w.meas is not None else 3)
        for what, a, b in zip(("states", "inputs", "jacobians", "measurements"), plain, stamped):
            assert torch.equal(a, b), "%s differ between the stamped and the product instantiation" % what
        v = buf.cpu().tolist()
        # thread 0 has stamped its five barrier intervals, wave 0 the hand-off poll and its own phase V
        assert all(v[i] > 0 for i in (0, 1, 3, 6, 7, 10, 16)), v
        # another call without a buffer leaves the filled buffer as it is
        _rollout(w, x0, fv)
        assert buf.cpu().tolist() == v
