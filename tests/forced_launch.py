"""One forced forward launch with its plan and dispatch report: shared by tests/test_gpu_status_word.py and tests/test_gpu_noise_truth.py."""
import ctypes as C

import numpy as np
import torch

import width_models as wm


def launch(form, c, pk, sample):
    """One rollout of the case ``c`` through the forced form ``form`` (status_models.Form) on ``pk`` = (model, policy, noise, meas, x0) as
    status_models.packed_op gives them.  Returns (states, inputs, measured or None, word, report words, plan)."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    M = form.M
    model, pol, nz, meas, x0 = pk
    L, d = hipabi.lib(), hipabi.DISPATCH
    left = [f[0] for f in d._fields_ if not f[0].startswith("ran_") and getattr(d, f[0])]
    assert not left, "a dispatch request was left set by an earlier test: %s" % left
    cus = torch.cuda.get_device_properties(x0.device).multi_processor_count
    with forced_variant(form.code):
        try:
            if form.policy_split is not None:
                L.mcp_debug_set_policy_split(form.policy_split)
            if form.row_split is not None:
                L.mcp_debug_set_row_split(form.row_split)
            if form.cluster_map is not None:
                L.mcp_debug_set_cluster_map(form.cluster_map)
            if form.xlds is not None or form.gb is not None:
                L.mcp_debug_set_fwd_mode(1 if form.xlds is None else form.xlds, form.gb or 0)
            want_rq = form.request()
            assert all(getattr(d, k) == getattr(want_rq, k) for k in ("fwd_particles", "gp_sharding", "fwd_lean", "policy_split", "row_split", "cluster_map",
                                                                      "fwd_no_xlds", "fwd_gb")), "the hooks did not leave the request the table states"
            # the plan of the call about to be made: same descriptors (the measurement model bound as the call binds it), first call on this model
            pc = pol.bind(wm.P_DROP)
            buf = torch.empty(c.T, M, c.S, dtype=torch.float64, device=x0.device) if meas is not None else None
            ops._set_meas(pol, meas, c.T, M, buf)
            try:
                nbytes = L.mcp_rollout_workspace_bytes(C.byref(model.c), C.byref(pc), M, c.T)
                fp = hipabi.FwdPlan()
                assert L.mcp_rollout_fwd_plan(C.byref(model.c), C.byref(pc), M, c.T, int(sample), nbytes, cus, C.byref(d), C.byref(fp)) == 0
            finally:
                ops._set_meas(pol, None, c.T, M, None)
            with torch.set_grad_enabled(not form.no_grad):
                st, inp, status = ops.rollout(model, pol, nz, x0, c.T, wm.P_DROP, particle_pred=sample, meas=meas)
            rep = (int(d.ran_particles), int(d.ran_gp_sharded), int(d.ran_fwd_lean), int(d.ran_row_split))
            mbuf = getattr(st.grad_fn, "meas_buf", None) if not form.no_grad else None
            assert form.no_grad or st.grad_fn is not None
        finally:
            L.mcp_debug_set_policy_split(-1)
            L.mcp_debug_set_row_split(-1)
            L.mcp_debug_set_cluster_map(-1)
            L.mcp_debug_set_fwd_mode(-1, 0)
    return st.detach().cpu().numpy(), inp.detach().cpu().numpy(), None if mbuf is None else mbuf.cpu().numpy(), int(status.item()), rep, fp


def against(name, got, want, bound, out):
    """max |got - want| over the entries finite in ``want``; a finite mask that differs, or an error not below ``bound``, adds a line to ``out``."""
    fm = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fm):
        bad = np.argwhere(np.isfinite(got) != fm)
        out.append("%s: finite mask differs at %d entries, first (t, m, i) = %s (kernel %r, oracle %r)" % (
            name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
        fm = fm & np.isfinite(got)
    err = float(np.abs(got[fm] - want[fm]).max()) if fm.any() else 0.0
    if not err < bound:
        out.append("%s: %.3e on the finite entries (bound %.1e)" % (name, err, bound))
    return err
