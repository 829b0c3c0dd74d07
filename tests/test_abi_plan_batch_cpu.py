"""CPU: the batched planner on this side of the GPU.  The layout of mcp_plan_batch through gcc on include/mcpilco_hip.h against the ctypes
mirror (mc_pilco_amd.hipabi.PlanBatch), as tests/test_abi_plan_cpu.py does for mcp_plan_ext; the three batched entries
(mcp_plan_batch_rollout, mcp_plan_batch_update, mcp_cem_batch_update) declared in the header, bound with the declaration's argument list and
exported; the ABI version, sizeof(mcp_mppi) and mcp_plan_ext, which they leave alone; what the entries refuse, with which code, on the
pattern of tests/test_plan_refusals_cpu.py (a refused call returns before any HIP call: device pointers are dummy addresses that nothing
reads); what ops.PackedPlanBatch, the three ops, policy_learning.mppi.plan_batch and Policy.MPPI_controller.forward refuse on the host.

Every expected code is written out: -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  The batch descriptor's checks sit among the plan's in the entries' one
order: NULL pointers (batch included); sizes (-1; B < 1 with them); limits (-2; B > MCP_PLAN_MAX_B and B K P > MCP_MPPI_MAX_M with them);
values (-1; a negative particle_stride and a short xi / eps stride with them)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from test_abi_cpu import declared_symbols
from test_mppi_refusals_cpu import A_PTR, cost, mppi
from test_open_refusals_cpu import PTR, abi, model
from test_plan_refusals_cpu import OUT2, S_PTR, ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcpilco_hip.h")
FIELDS = ["B", "x0_per_particle", "particle_stride", "xi_stride", "eps_stride"]
PTRS = {"const mcp_model*": "Model", "const mcp_mppi*": "MPPI", "const mcp_plan_ext*": "PlanExt", "const mcp_plan_batch*": "PlanBatch",
        "const mcp_cost*": "Cost", "const mcp_cost_inputs*": "CostInputs", "const mcp_noise*": "Noise"}
CTYPE = {"int": C.c_int, "const double*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p, "uint32_t*": C.c_void_p, "void*": C.c_void_p}
ENTRIES = (("mcp_plan_batch_rollout", 14, "const mcp_model*", "mcp_plan_rollout", 3), ("mcp_plan_batch_update", 11, "const mcp_mppi*", "mcp_mppi_update_ext", 2),
           ("mcp_cem_batch_update", 12, "const mcp_mppi*", "mcp_cem_update", 2))


def test_struct_layout_against_the_header(tmp_path):
    from mc_pilco_amd import hipabi

    names = [n for n, _ in hipabi.PlanBatch._fields_]
    assert names == FIELDS
    src = tmp_path / "pb.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpilco_hip.h"\nint main(void){printf("%zu", sizeof(mcp_plan_batch));'
                   + "".join('printf(" %%zu %%zu", offsetof(mcp_plan_batch, %s), sizeof(((mcp_plan_batch*)0)->%s));' % (n, n) for n in names)
                   + 'printf(" %zu %zu %d %d", sizeof(mcp_mppi), sizeof(mcp_plan_ext), MCP_PLAN_MAX_B, MCP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "pb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(hipabi.PlanBatch) == 2 * 4 + 3 * 8  # two int32, three int64, no padding
    for i, n in enumerate(names):
        f = getattr(hipabi.PlanBatch, n)
        assert out[1 + 2 * i:3 + 2 * i] == [f.offset, f.size], n
    # what the batched form leaves alone: the plan, its extension, the version
    assert out[-4:] == [C.sizeof(hipabi.MPPI), C.sizeof(hipabi.PlanExt), hipabi.PLAN_MAX_B, hipabi.ABI_VERSION] == [200, 104, 4096, 7]


def test_the_entries_are_declared_bound_and_exported():
    from mc_pilco_amd import hipabi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hipabi.lib()
    for name, n_args, first, single, at in ENTRIES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, txt).group(1)
        types_ = [re.sub(r"\s*\w+$", "", a.strip()) for a in decl.split(",")]
        assert len(types_) == n_args and types_[0] == first and types_[-1] == "void*" and types_[-2] == "uint32_t*"
        res, sig = hipabi._SIGS[name]
        assert res is C.c_int and len(sig) == n_args
        for t, s in zip(types_, sig):
            assert s is (C.POINTER(getattr(hipabi, PTRS[t])) if t in PTRS else CTYPE[t]), (name, t)
        assert name in hipabi.EXPORTED and name in declared_symbols() and hasattr(lib, name)
        # the batch descriptor sits behind the extension; the other arguments are the single-problem entry's
        assert sig[at] is C.POINTER(hipabi.PlanBatch) and sig[:at] + sig[at + 1:] == hipabi._SIGS[single][1]
    assert set(hipabi.EXPORTED) == set(declared_symbols())
    assert lib.mcp_abi_version() == hipabi.ABI_VERSION == 7 and re.search(r"#define MCP_ABI_VERSION 7\b", open(HEADER).read())
    assert int(re.search(r"#define MCP_PLAN_MAX_B (\d+)", open(HEADER).read()).group(1)) == hipabi.PLAN_MAX_B == 4096


# ---- the refusals of the C entries ---------------------------------------------------------------------------------------------------------
SIGS = {
    "plan_batch_rollout": ("model", "mppi", "ext", "batch", "cost", "cin", "noise", "particle_pred", "x0", "traj_cost", "states", "inputs", "status"),
    "plan_batch_update": ("mppi", "ext", "batch", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status"),
    "cem_batch_update": ("mppi", "ext", "batch", "noise", "traj_cost", "a_new", "sigma_new", "cand_cost", "elite", "stats", "status"),
}
REQUIRED = {"plan_batch_rollout": ("model", "mppi", "batch", "cost", "noise", "x0", "traj_cost", "status"),
            "plan_batch_update": ("mppi", "batch", "noise", "traj_cost", "a_new", "cand_cost", "weights", "stats", "status"),
            "cem_batch_update": ("mppi", "ext", "batch", "noise", "traj_cost", "a_new", "sigma_new", "cand_cost", "elite", "stats", "status")}
OPTIONAL = ("cin", "states", "inputs")
ALL = tuple(SIGS)


def batch(**edit):
    """A valid descriptor: 3 problems, Philox ids 1000 apart, one xi / eps buffer for all."""
    b = abi().PlanBatch()
    b.B, b.particle_stride = 3, 1000
    for k, v in edit.items():
        setattr(b, k, v)
    return b


def call(entry, **over):
    U = over.pop("U", 1)
    args = dict(model=model(U), mppi=mppi(U), ext=ext(), batch=batch(), cost=cost(), noise=abi().Noise(), particle_pred=1, sigma_new=OUT2)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL else PTR)
    return getattr(abi().lib(), "mcp_" + entry)(*vals, None)


def codes(**over):
    return {e: call(e, **dict(over)) for e in ALL}


def every(code):
    return {e: code for e in ALL}


@pytest.mark.parametrize("entry", ALL)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    assert call(entry, mppi=mppi(a=None)) == -1
    if entry != "cem_batch_update":  # a default extension, and none
        assert call(entry, batch=None, ext=None) == -1 and call(entry, batch=None, ext=abi().PlanExt()) == -1


def test_the_number_of_problems():
    for bad in (0, -1, -(2 ** 31)):
        assert codes(batch=batch(B=bad)) == every(-1), bad
    assert codes(batch=batch(B=abi().PLAN_MAX_B + 1)) == every(-2)
    assert codes(batch=batch(B=2 ** 31 - 1)) == every(-2)
    # B K P over the limit: K P alone passes (2^29), three problems of it do not
    big = dict(mppi=mppi(K=1 << 14, P=1 << 15), ext=ext(n_elite=1))
    assert codes(batch=batch(B=3), **big) == every(-2)
    assert codes(batch=batch(B=abi().PLAN_MAX_B), mppi=mppi(K=1 << 10, P=1 << 9), ext=ext(n_elite=1)) == every(-2)  # 2^31: past an int32 too


def test_the_strides():
    for bad in (-1, -(2 ** 62)):
        assert codes(batch=batch(particle_stride=bad)) == every(-1), bad
    # mppi(): H 6, K 8, U 1 -> an xi buffer of 48 doubles; model(): G 2, P 2 -> an eps buffer of 5 * 2 * 2 = 20
    for bad in (1, 47, -48):
        assert codes(batch=batch(xi_stride=bad)) == every(-1), bad
    for bad in (1, 19, -20):
        assert call("plan_batch_rollout", batch=batch(eps_stride=bad)) == -1, bad
    # the updates read no eps: its stride is the rollout's alone, and every entry is then refused for something else alone
    for e in ("plan_batch_update", "cem_batch_update"):
        assert call(e, batch=batch(eps_stride=1), a_new=A_PTR) == -1
    assert call("plan_batch_rollout", batch=batch(xi_stride=48, eps_stride=20), cost=cost(kind=7)) == -1


def test_every_refusal_of_the_single_problem_entries():
    for edit in (dict(K=0), dict(P=0), dict(H=1), dict(U=0), dict(t0=-1)):
        assert codes(mppi=mppi(**edit)) == every(-1), edit
    assert codes(mppi=mppi(U=abi().MAX_INPUT + 1)) == every(-2)
    assert codes(mppi=mppi(K=abi().MPPI_MAX_K + 1)) == every(-2)
    assert codes(mppi=mppi(H=20481)) == every(-2)
    for edit in (dict(lam=0.0), dict(sigma=(0, -0.5)), dict(u_max=(0, 0.0)), dict(kappa=0.5, P=1), dict(kappa=float("nan"))):
        assert codes(mppi=mppi(**edit)) == every(-1), edit
    for bad in (-0.5, 1.0, float("nan")):
        assert codes(ext=ext(beta=bad)) == every(-1), bad
    for edit in (dict(S=17), dict(G=9), dict(gp_N=abi().MAX_TRAIN + 1)):
        assert call("plan_batch_rollout", model=model(**edit)) == -2, edit
    assert call("plan_batch_rollout", model=model(2)) == -1 and call("plan_batch_rollout", cost=cost(kind=7)) == -1
    assert call("cem_batch_update", ext=ext(n_elite=0)) == -1 and call("cem_batch_update", ext=ext(n_elite=9)) == -2
    assert call("cem_batch_update", ext=ext(alpha=1.0)) == -1 and call("cem_batch_update", ext=ext(sigma_min=(0, -1.0))) == -1
    assert call("plan_batch_update", a_new=A_PTR) == -1 and call("plan_batch_update", a_new=S_PTR, ext=ext(sigma_rows=S_PTR)) == -1
    for over in (dict(a_new=A_PTR), dict(sigma_new=A_PTR), dict(a_new=OUT2), dict(sigma_new=S_PTR, ext=ext(sigma_rows=S_PTR))):
        assert call("cem_batch_update", **over) == -1, over
    assert call("plan_batch_rollout", mppi=mppi(H=10241)) == -2  # the std's rows count in the LDS fit, as in mcp_plan_rollout


def test_precedence():
    assert codes(batch=batch(B=0), mppi=mppi(K=abi().MPPI_MAX_K + 1)) == every(-1)  # B < 1 is a size: before every limit
    assert codes(batch=batch(B=abi().PLAN_MAX_B + 1), mppi=mppi(K=0)) == every(-1)  # the plan's sizes before the batch's limit
    assert codes(batch=batch(B=abi().PLAN_MAX_B + 1, particle_stride=-1)) == every(-2)  # a limit before a value
    assert codes(batch=batch(B=abi().PLAN_MAX_B + 1), mppi=mppi(lam=0.0)) == every(-2)
    assert codes(batch=batch(B=abi().PLAN_MAX_B + 1), ext=ext(beta=2.0)) == every(-2)
    assert codes(batch=batch(xi_stride=1), mppi=mppi(K=abi().MPPI_MAX_K + 1)) == every(-2)  # the plan's limits before the strides
    assert call("plan_batch_rollout", model=model(S=17), batch=batch(particle_stride=-1)) == -2  # the model's limits before the strides
    assert call("plan_batch_rollout", mppi=mppi(H=10241), batch=batch(particle_stride=-1)) == -1  # the strides before the fit
    assert call("cem_batch_update", batch=batch(B=0), ext=ext(n_elite=9)) == -1 and call("cem_batch_update", batch=batch(xi_stride=1), ext=ext(n_elite=9)) == -2


# ---- this side of the ABI -------------------------------------------------------------------------------------------------------------------
def test_packed_plan_batch_refuses_bad_host_values():
    from mc_pilco_amd import ops

    b = ops.PackedPlanBatch(3, 2)
    assert (b.B, b.P, b.x0_per_particle, b.particle_stride) == (3, 2, False, 0)
    c = ops.PackedPlanBatch(5, 3, True, 1000).to_c(48, 20)
    assert (c.B, c.x0_per_particle, c.particle_stride, c.xi_stride, c.eps_stride) == (5, 1, 1000, 48, 20)
    for args in ((0, 1), (-1, 1), (ops.abi.PLAN_MAX_B + 1, 1), (3, 0), (4096, 1 << 20), (3, 2, False, -1), (3, 2, False, 0.5), (3, 2, False, 2 ** 40)):
        with pytest.raises(ValueError):
            ops.PackedPlanBatch(*args)


def _stub(device):
    return types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device(device), c=None)


def test_ops_refuse_wrong_operands():
    from mc_pilco_amd import ops

    mp = ops.PackedMPPI(K=8, P=2, H=6, U=2, sigma=0.3, lam=1.0)
    e = ops.PackedPlanExt(6, 2, beta=0.5, n_elite=4)
    bt = ops.PackedPlanBatch(3, 2)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    pc = types.SimpleNamespace(kind="target", c=None)
    gpu = _stub("cuda:0")
    with pytest.raises(ValueError, match="PackedPlanBatch"):
        ops.plan_batch_rollout(gpu, mp, None, None, pc, z(3, 4), z(3, 6, 2))
    with pytest.raises(ValueError, match="made for P"):
        ops.plan_batch_rollout(gpu, mp, None, ops.PackedPlanBatch(3, 1), pc, z(3, 4), z(3, 6, 2))
    with pytest.raises(ValueError, match="a must have the shape"):
        ops.plan_batch_rollout(gpu, mp, None, bt, pc, z(3, 4), z(6, 2))
    with pytest.raises(ValueError, match="x0 must have the shape"):
        ops.plan_batch_rollout(gpu, mp, None, ops.PackedPlanBatch(3, 2, True), pc, z(3, 4), z(3, 6, 2))
    with pytest.raises(ValueError, match="xi must have the shape"):
        ops.plan_batch_rollout(gpu, mp, None, bt, pc, z(3, 4), z(3, 6, 2), xi=z(2, 6, 8, 2))
    with pytest.raises(ValueError, match="float64"):
        ops.plan_batch_rollout(gpu, mp, None, bt, pc, z(3, 4), z(3, 6, 2).float())
    with pytest.raises(ValueError, match="sigma_rows must have the shape"):
        ops.plan_batch_rollout(gpu, mp, e, bt, pc, z(3, 4), z(3, 6, 2), sigma_rows=z(6, 2))
    with pytest.raises(ValueError, match="u_prev must have the shape"):
        ops.plan_batch_rollout(gpu, mp, e, bt, pc, z(3, 4), z(3, 6, 2), u_prev=z(2))
    with pytest.raises(ValueError, match="device"):
        ops.plan_batch_rollout(gpu, mp, None, bt, pc, z(3, 4), z(3, 6, 2))
    with pytest.raises(ValueError, match="device"):
        ops.plan_batch_update(mp, e, bt, z(3, 16), z(3, 6, 2))
    with pytest.raises(ValueError, match="shape"):
        ops.plan_batch_update(mp, e, bt, z(16), z(3, 6, 2))
    with pytest.raises(ValueError, match="traj_cost"):
        ops.plan_batch_update(mp, e, bt, [0.0] * 48, z(3, 6, 2))
    with pytest.raises(ValueError, match="elites of"):
        ops.cem_batch_update(mp, ops.PackedPlanExt(6, 2, n_elite=9), bt, z(3, 16), z(3, 6, 2))
    with pytest.raises(ValueError, match="PackedPlanExt"):
        ops.cem_batch_update(mp, None, bt, z(3, 16), z(3, 6, 2))
    with pytest.raises(ValueError, match="device"):
        ops.cem_batch_update(mp, e, bt, z(3, 16), z(3, 6, 2))


def _cost():
    from mc_pilco_amd.policy_learning import Cost_function as cf

    return cf.Expected_saturated_distance([0.0, 0.0], [1.0, 1.0], [0, 1])


def test_plan_batch_refuses_bad_arguments():
    import mc_pilco_amd.policy_learning.mppi as mod

    pm = types.SimpleNamespace(S=4, U=2, G=2, D=8, device=torch.device("cpu"))  # (every refusal comes before the model is looked at)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    keep = mod._packed_model
    mod._packed_model = lambda m: m
    try:
        for x0, a, kw, msg in ((z(4), z(6, 2), {}, "x0"), (z(3, 5), z(6, 2), {}, "x0"), (z(3, 2, 4), z(6, 2), dict(P=3), "x0"),
                               (z(3, 4), z(6, 3), {}, "a_init"), (z(3, 4), z(2, 6, 2), {}, "a_init"), (z(3, 4), z(1, 2), {}, "a_init"),
                               (z(3, 4), z(6, 2), dict(iterations=0), "iteration"), (z(3, 4), z(6, 2), dict(method="softmax"), "method"),
                               (z(3, 4), z(6, 2), dict(beta=1.0), "beta"), (z(3, 4), z(6, 2), dict(method="cem", n_elite=9), "elites"),
                               (z(3, 4), z(6, 2), dict(particle_stride=-1), "particle_stride"),
                               (z(3, 4), z(6, 2), dict(sigma_rows=[[0.1, -0.1]] * 6), "sigma_rows"),
                               (z(3, 4), z(6, 2), dict(sigma_rows=[[[0.1, 0.1]] * 6] * 2), "sigma_rows"),
                               (z(3, 4), z(6, 2), dict(sigma_rows=[[[0.1, float("nan")]] * 6] * 3), "sigma_rows"),
                               (z(3, 4), z(6, 2), dict(u_prev=z(3)), "u_prev")):
            with pytest.raises(ValueError, match=msg):
                mod.plan_batch(pm, x0, a, _cost(), K=8, **kw)
    finally:
        mod._packed_model = keep


def test_the_controller_refuses_a_skipped_step_and_a_changed_m():
    """forward holds a warm start per particle under PID_controller.forward's contract: t == 0 resets, every other call follows the previous
    t by one with the same M.  The plan itself is stubbed: the refusals come before it and need no device."""
    import mc_pilco_amd.policy_learning.mppi as mod
    from mc_pilco_amd.policy_learning import Policy

    keep, calls = mod.plan_batch, []

    def fake(model, x0, a_init, cost, **kw):
        calls.append((int(x0.shape[0]), kw["t0"], kw["noise"].call, kw.get("u_prev") is not None, kw["particle_stride"]))
        return a_init.clone() + 0.25, dict(status=None)

    mod.plan_batch = fake
    try:
        ctrl = Policy.MPPI_controller(4, 2, None, _cost(), horizon=6, iterations=2, device=torch.device("cpu"), K=8, charge_first_rate=True,
                                      particle_stride=7)
        x = torch.zeros(5, 4, dtype=torch.float64)
        with pytest.raises(ValueError, match="t == 0"):
            ctrl.forward(x, t=1)  # nothing to continue
        with pytest.raises(ValueError, match="step index"):
            ctrl.forward(x)
        u = ctrl.forward(x, t=0)
        assert tuple(u.shape) == (5, 2) and not u.requires_grad and torch.equal(u, torch.tanh(torch.full((5, 2), 0.25, dtype=torch.float64)))
        ctrl.forward(x, t=1)
        with pytest.raises(ValueError, match="after t = 1"):
            ctrl.forward(x, t=3)  # a skipped step
        with pytest.raises(ValueError, match="after t = 1"):
            ctrl.forward(x, t=1)  # a repeated one
        with pytest.raises(ValueError, match="5 particles"):
            ctrl.forward(x[:4], t=2)  # another M
        ctrl.forward(x, t=2)
        ctrl.forward(x[:4], t=0)  # t == 0 starts over, with any M
        # step, call = noise.call + t * iterations, u_prev from the second step on, the stride handed through; the cost tracks nothing: t0 = 0
        assert calls == [(5, 0, 0, False, 7), (5, 0, 2, True, 7), (5, 0, 4, True, 7), (4, 0, 0, False, 7)]
        assert ctrl.step == 0 and ctrl.u_last is None  # forward_np's episode is its own
    finally:
        mod.plan_batch = keep
