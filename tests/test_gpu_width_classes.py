"""The fused rollout, the cost kernels and the adjoint sweep at the width classes the cart-pole and UR5 shapes do not reach: every case of
tests/width_models.py against the CPU oracle (same X / alpha / Kinv, same recorded eps, masks and position noise), through the kernel variants its
shape admits, with the dispatch report asserted.

Sizes: T in {2, 3, 4}; N = 24 .. 60 per GP (Npad 32 / 48 / 64); M = 5 on the 1 / 2 / 4-particle forms (one full cluster and a ragged one), M = 17 and 33
on the 16-particle forms (a tile and a ragged one; two and one).  Bounds are those of the short recorded rollouts (test_gpu_lean_chain.py,
test_gpu_parity.py): 1e-9 absolute on states and inputs, 1e-11 relative on the expected cost, 1e-8 of the oracle's largest entry on every gradient
(log_ls, centers, weight, bias, x0), status word 0.

Coverage (instantiation -> cases; each is compared with the oracle and asserts through the dispatch report that the form ran):

  sweep <8,2>   / 256            narrow_traj_d7 (B 17), narrow_overlap_d7 (17), narrow_disjoint_d6 (129; forced widths run the general sweep)
  sweep <8,2>   / 1024           narrow_b257, g1_plain_d16 (B 600), narrow_b1024
  sweep <16,4>  / 256            d8_u3_pms (through U; measurement model: the PMS form of a non-<8,2> class), d25_s16_g8 and speed_mixed_p9 (through P),
                                 delta_d11_u3 (through U)
  sweep <16,4>  / 1024           d15_p10_g3 (B 257, through P), u4_b513 (B 513, through U)
  sweep <24,6>  / 256            u5_g5_d16 (through U), ur5_angles_pms (P = 24 and U = 6: the top of its accumulators; measurement model)
  sweep <24,6>  / 512            p17_u2_b257 (through P; 8 / 4 / 2 / 1 particles per workgroup requested; pipelined and sequential)
  sweep <32,8>  / 256            p25_u2 (through P), d31_traj_p32, d32_u8_pms (measurement model)
  sweep <32,8>  / 512            u7_g7_b257 (through U; pipelined and sequential)
  pipelined sweep                p17_u2_b257, u7_g7_b257 (ran_bwd_pipe == 1; == 0 when forced off)
  tile class 0                   narrow_traj_d7 (D 7, P 8, U 2: its top), narrow_overlap_d7
  tile class 1, one row tile     d8_u3_pms (D 8), d15_p10_g3 (D + 1 = 16 exactly), p17_u2_b257 (D 12)
  tile class 1, two row tiles    g1_plain_d16 and u5_g5_d16 (D 16), ur5_angles_pms (D 24, P 24: its top)
  tile class 2 by width          d25_s16_g8 (D 25), p25_u2 (P 25), u7_g7_b257 (U 7), d31_traj_p32 (D 31: the top of the tile kernel);
                                 a forced GP-sharded 16-particle launch runs the unsharded tile kernel
  D = 32 fallback                d32_u8_pms (a forced 16 runs the 4-particle kernel)
  G = 1 / prime / 8              g1_plain_d16 (forced sharding runs unsharded) / d15_p10_g3 (3), u5_g5_d16 (5), u7_g7_b257 (7) / d25_s16_g8, d31_traj_p32,
                                 d32_u8_pms
  S = 16, U = 8                  d25_s16_g8, d31_traj_p32, d32_u8_pms / d32_u8_pms
  plain policy at T > 1          g1_plain_d16 (narrow), d25_s16_g8, delta_d11_u3, u5_g5_d16, u7_g7_b257, d32_u8_pms (wide)
  traj narrow / angles wide      narrow_traj_d7 / ur5_angles_pms, p25_u2, p17_u2_b257
  overlapping index lists        narrow_overlap_d7 (ran_fwd_lean == ran_bwd_lean == 0; narrow_disjoint_d6 shows both at 1)
  lean forward at B > 256        narrow_b257, narrow_b1024 (ran_fwd_lean == 1 on request: that kernel has no limit on B; the lean SWEEP stops at 256)
  mixed not_vel                  speed_mixed_p9, u5_g5_d16, u7_g7_b257
  var_scale != 1                 speed_mixed_p9
  delta model                    delta_d11_u3;  bias, u_max per input: d8_u3_pms, d32_u8_pms
  a different N per GP           d15_p10_g3, delta_d11_u3, p17_u2_b257, speed_mixed_p9

The sweep width: the dispatch report has no field for the particles per workgroup the sweep ran, and the library halves a forced width it cannot
launch (no such instantiation, or the prefetched record does not fit).  ``wm.sweep_widths`` restates which widths a case can launch, and every variant
requests the largest of them not above the width it names, so the requested width is one the rules say is launched as asked; that it did run is
derived from the code, not asserted.

A wide policy (P > 16 or U > 4) with B > 512 has no sweep instantiation: it is refused where it is created and by mcp_rollout_fwd
(test_wide_policy_beyond_512_basis_functions_is_refused)."""

import numpy as np
import pytest
import torch

import width_models as wm

pytestmark = pytest.mark.gpu

M_SMALL, M_TILE, M_TILE2 = 5, 17, 33


def _variants(c):
    """(forward code, backward particles per workgroup or None, pipe request or None, M) for a case: the unsharded small-tile kernels, the sharded
    one, the lean request on narrow models, the 16-particle kernel unsharded and GP-sharded, automatic dispatch; on the 512-thread wide sweeps every
    particle width and the pipelined form on and off."""
    k = wm.classes(c)
    ok = wm.sweep_widths(c)

    def fit(pb):  # the largest width the sweep can launch for this case that is not above ``pb``
        return max(w for w in ok if w <= pb)

    v = [(1, 1, None, M_SMALL), (2, fit(2), None, M_SMALL), (4, fit(4), None, M_SMALL), (104, fit(4), None, M_SMALL), (16, fit(4), None, M_TILE),
         (116, fit(2), None, M_TILE2), (0, None, None, M_TILE), (0, None, None, M_SMALL)]
    if c.D <= 8 and c.P <= 8 and c.U <= 2:
        v += [(204, None, None, M_SMALL), (201, None, None, M_SMALL)]
    if c.name in ("d15_p10_g3", "u5_g5_d16"):
        v += [(101, 1, None, M_SMALL), (102, fit(2), None, M_SMALL)]
    if k["pipe"]:
        v += [(1, 1, 1, M_SMALL), (1, 1, 0, M_SMALL), (4, fit(8), None, M_TILE)]
    return v


def _expected(c, code):
    """What the library reports for a forced forward code on this shape: (particles per workgroup, GP-sharded, lean forward or None = not pinned)."""
    k = wm.classes(c)
    ppw, sharded, lean = code % 100, code >= 100, code >= 200
    if ppw == 16:
        if k["tile"] is None:
            return 4, False, False  # (no tile kernel at D + 1 > 32: the 4-particle kernel, unsharded)
        return 16, sharded and k["tile_sharded"], False
    lean_possible = (c.G >= 2 and c.kind != "traj" and not wm.lists_overlap(c) and c.S <= 8)  # (the lean FORWARD kernel has no limit on B)
    return ppw, sharded and c.G >= 2, (None if (lean and lean_possible) else False)


ALL = [(c, v) for c in wm.CASES for v in _variants(c)]


def _id(cv):
    c, (code, pb, pipe, M) = cv
    return "%s-f%d-b%s%s-M%d" % (c.name, code, "a" if pb is None else pb, "" if pipe is None else "-pipe%d" % pipe, M)


def _abserr(a, b):
    return float(np.abs(a.detach().cpu().numpy() - np.asarray(b)).max())


def _relerr(a, b):
    b = np.asarray(b)
    return float(np.abs(a.detach().cpu().numpy() - b).max() / max(np.abs(b).max(), 1e-300))


def _run(c, code, pb, pipe, M, want_gx0, philox=None):
    """One rollout + expected cost + backward through the forced variant.  Returns (states, inputs, cost, policy, x0 with .grad, report).
    ``philox``: a NoiseSpec without buffers (wm.packed)."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    model, pol, cost, nz, meas, x0 = wm.packed(c, M, philox)
    if want_gx0:
        x0.requires_grad_(True)
    L = hipabi.lib()
    with forced_variant(code, bwd_particles=pb):
        try:
            if pipe is not None:
                L.mcp_debug_set_bwd_pipe(pipe)
            st, inp, status = ops.rollout(model, pol, nz, x0, c.T, wm.P_DROP, meas=meas)
            d = hipabi.DISPATCH
            rep = dict(particles=int(d.ran_particles), sharded=int(d.ran_gp_sharded), fwd_lean=int(d.ran_fwd_lean), row_split=int(d.ran_row_split))
            cst, _ = ops.expected_cost(cost, st)
            cst.backward()
            rep.update(bwd_lean=int(d.ran_bwd_lean), bwd_pipe=int(d.ran_bwd_pipe))
        finally:
            L.mcp_debug_set_bwd_pipe(-1)
    assert int(status.item()) == 0
    return st, inp, cst, pol, x0, rep


@pytest.mark.parametrize("cv", ALL, ids=_id)
def test_rollout_cost_and_gradients_vs_oracle(cv):
    from gpu_helpers import forced_variant

    c, (code, pb, pipe, M) = cv
    k = wm.classes(c)
    ost, oin, oc, og = wm.oracle(c, M)
    st, inp, cst, pol, x0, rep = _run(c, code, pb, pipe, M, c.gx0)
    print(c.name, "D %d P %d U %d G %d B %d:" % (c.D, c.P, c.U, c.G, c.B), k, "| ran", rep)
    # ---- the form that ran ----
    if code:
        ppw, sharded, lean = _expected(c, code)
        assert rep["particles"] == ppw, "forced %d particles per workgroup, %d ran" % (ppw, rep["particles"])
        assert bool(rep["sharded"]) == sharded
        if lean is not None:
            assert bool(rep["fwd_lean"]) == lean
    else:
        assert rep["particles"] in (1, 2, 4, 16)
        if k["tile"] is None:
            assert rep["particles"] != 16
    assert rep["row_split"] == 0  # (two workgroups per (tile, GP) need Npad >= 128)
    pb_eff = forced_variant(code, bwd_particles=pb).pb  # (0: the automatic sweep, which may be the lean one)
    wide = wm.lists_overlap(c) or c.G < 2 or c.P > 8 or c.U > 2 or c.S > 8 or c.kind == "traj"
    if wide:
        assert rep["fwd_lean"] == 0
    if wide or c.B > 256 or pb_eff:  # (the lean sweep takes up to 256 basis functions; the lean forward kernel has no such limit)
        assert rep["bwd_lean"] == 0
    if c.name in ("narrow_disjoint_d6", "narrow_b257", "narrow_b1024"):  # (the widths of narrow_overlap_d7 with disjoint lists: the report does tell them apart)
        if code >= 200:
            assert rep["fwd_lean"] == 1
        if pb_eff == 0:
            assert rep["bwd_lean"] == (1 if c.B <= 256 else 0)
    if pipe is not None:
        assert rep["bwd_pipe"] == pipe
    elif not k["pipe"]:
        assert rep["bwd_pipe"] == 0
    elif pb_eff in (0, 1):
        assert rep["bwd_pipe"] == 1  # (one particle per workgroup on a 512-thread wide sweep with a wave to spare)
    # ---- parity ----
    errs = [_abserr(st, ost), _abserr(inp, oin), abs(float(cst) - oc) / abs(oc), _relerr(pol.log_ls.grad, og[0]), _relerr(pol.centers.grad, og[1]),
            _relerr(pol.weight.grad, og[2])]
    if c.bias:
        errs.append(_relerr(pol.bias.grad, og[3]))
    if c.gx0:
        errs.append(_relerr(x0.grad, og[4]))
    print("errs states, inputs (abs), cost, gradients (rel):", " ".join("%.2e" % e for e in errs))
    assert all(float(np.abs(g).max()) > 0.0 for g in og[:3])
    assert errs[0] < 1e-9 and errs[1] < 1e-9
    assert errs[2] < 1e-11
    assert max(errs[3:]) < 1e-8


TILE_CASES = [c for c in wm.CASES if wm.classes(c)["tile"] is not None]


@pytest.mark.parametrize("M", [M_TILE, M_TILE2])
@pytest.mark.parametrize("c", TILE_CASES, ids=lambda c: c.name)
def test_every_output_element_is_written(monkeypatch, c, M):
    """states, inputs, jac and the measurements start as NaN: the 16-particle kernel (GP-sharded where the class has that launch) leaves none, at a
    ragged last tile.  Each case runs at its OWN T, which is 2 for eight of them and 3 or 4 for the others -- not at T = 2 throughout: the T = 2 cases are
    the shortest rollout that has a Jacobian, the longer ones add the steps between the first and the last."""
    from gpu_helpers import forced_variant
    from mc_pilco_amd import hipabi, ops

    model, pol, _, nz, meas, x0 = wm.packed(c, M)
    real_empty = torch.empty

    def nan_empty(*shape, **kw):  # (the output arrays are the call's only float tensors of three or more dimensions)
        t = real_empty(*shape, **kw)
        if t.dtype == torch.float64 and t.dim() >= 3:
            t.fill_(float("nan"))
        return t

    code = 116 if M == M_TILE2 else 16
    with forced_variant(code):
        monkeypatch.setattr(torch, "empty", nan_empty)
        out = ops.rollout_forward_raw(model, pol, nz, x0, c.T, wm.P_DROP, need_jac=True, meas=meas)
        monkeypatch.undo()
        assert hipabi.DISPATCH.ran_particles == 16
        assert bool(hipabi.DISPATCH.ran_gp_sharded) == (code == 116 and wm.classes(c)["tile_sharded"])
    assert int(out[3].item()) == 0
    assert tuple(out[2].shape) == (c.T - 1, M, c.G, c.D)
    names = ["states", "inputs", "jac"] + (["meas"] if meas is not None else [])
    for name, t in zip(names, [out[0], out[1], out[2]] + ([out[4]] if meas is not None else [])):
        assert not bool(torch.isnan(t).any()), name


@pytest.mark.parametrize("c", [wm.BY_NAME[n] for n in ("d15_p10_g3", "u5_g5_d16", "d31_traj_p32", "d32_u8_pms", "delta_d11_u3")], ids=lambda c: c.name)
def test_particles_per_workgroup_reproduce_each_other(c):
    """Forced 1, 2, 4 and 16 particles per workgroup (and the GP-sharded 4) on the same 17 particles: trajectories within 1e-9, gradients within
    1e-8 of each other (the variant bounds of test_gpu_parity.py)."""
    ref = None
    for code in (4, 2, 1, 16, 104):
        st, inp, cst, pol, _, rep = _run(c, code, None, None, M_TILE, False)
        assert rep["particles"] == _expected(c, code)[0]
        got = [st.detach(), inp.detach(), pol.log_ls.grad.clone(), pol.centers.grad.clone(), pol.weight.grad.clone()]
        if ref is None:
            ref = got
            continue
        for i, (a, b) in enumerate(zip(got, ref)):
            if i < 2:
                assert float((a - b).abs().max()) < 1e-9
            else:
                assert float((a - b).abs().max() / b.abs().max()) < 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the B limit of the wide sweeps
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _wide_policy_args(P, U, B):
    from gpu_helpers import G as GG

    rng = np.random.RandomState(P + 10 * U + B)
    S = P // 2
    return ("traj", S, torch.log(GG(1.0 + rng.rand(P))).reshape(1, -1), GG(rng.randn(B, P)), GG(rng.randn(U, B)), 1.0, True), dict(target_traj=np.zeros((2, S)))


@pytest.mark.parametrize("P,U,B", [(24, 6, 513), (32, 8, 1024), (18, 2, 513), (8, 5, 1024)])
def test_wide_policy_beyond_512_basis_functions_is_refused(P, U, B):
    """The sweeps of the <24,6> and <32,8> classes (P > 16 or U > 4) have one thread per basis function in workgroups of up to 512: a policy of such
    a width with more than MCP_MAX_BASIS_WIDE = 512 basis functions cannot be differentiated, so it is refused where it is created, and
    mcp_rollout_fwd refuses the descriptor too (MCP_ERR_LIMIT) -- the forward does not accept what the backward cannot differentiate.  The same
    widths at B = 512 are served."""
    import ctypes as C

    from gpu_helpers import G as GG
    from mc_pilco_amd import hipabi as abi
    from mc_pilco_amd import ops

    args, kw = _wide_policy_args(P, U, B)
    with pytest.raises(ValueError, match="512"):
        ops.PackedPolicy(*args, **kw)
    # the C ABI itself: the descriptor of a served policy with B raised past the limit (its arrays are large enough: they are the refused policy's)
    a512, _ = _wide_policy_args(P, U, 512)
    pol = ops.PackedPolicy(*a512, **kw)
    pol.centers, pol.weight = args[3], args[4]
    pc = pol.bind(0.0)
    S, M = pol.S, 5
    x0 = GG(np.zeros((M, S)))
    states, inputs = torch.empty(1, M, S, dtype=torch.float64, device=x0.device), torch.empty(1, M, U, dtype=torch.float64, device=x0.device)
    status = torch.zeros(1, dtype=torch.int32, device=x0.device)
    nz = ops.NoiseSpec().to_c()

    def fwd():
        return abi.lib().mcp_rollout_fwd_ex(None, C.byref(pc), C.byref(nz), M, 1, 1, abi.ptr(x0), abi.ptr(states), abi.ptr(inputs), None, abi.ptr(status),
                                            None, 0, abi.stream(), C.byref(abi.DISPATCH))

    assert fwd() == 0
    pc.B = B
    assert abi.ERRORS[fwd()] == "MCP_ERR_LIMIT"
