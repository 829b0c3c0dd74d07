"""GPU: the entry points that share the generic step and the generic sweep -- mcp_rollout_open / _rec / _bwd, mcp_model_step / _bwd, the PD,
measured-PD, PID and TVL closed loops with their sweeps, the tanh-MLP loop, mcp_linearize and mcp_lqr_pass -- on the irregular model
layouts of tests/layout_models.py (what each layout pins is written there), against each family's own truth on the "mixed" integrator
(tests/test_layout_models_cpu.py pins the truth, its sensitivity and the conditions every case relies on), driven through
tests/closed_loop_family.py.

Bounds: the constants of each family's own GPU module, imported and not restated -- TOLS of tests/test_gpu_pd_rollout.py,
test_gpu_pid_rollout.py, test_gpu_tvl_rollout.py and test_gpu_mlp_rollout.py (states 1e-9 absolute, inputs 2e-9 absolute, gradients 1e-9
relative), STATE_TOL / GRAD_TOL of tests/test_gpu_open_rollout_grad.py, TOL of tests/test_gpu_model_step.py (next state, means, variances,
gradients), GRAD_TOL / STEP_TOL / bound() of tests/test_gpu_lqr.py.  All cases stay at N = 37 and T <= 12, the sizes those bounds were
set at.

Worst measured per form on an MI355X, over the cases of the form (every one inside its bound by two orders or more; no case of the
matrix exposed a defect in a kernel):
  open loop      states 5.9e-12  g_x0 1.6e-12  g_u 1.1e-12  mean 1.1e-12  var 3.2e-12
  model step     x_next 1.8e-13  mean 2.2e-15  var 1.8e-14  g_x 7.3e-14  g_u 4.1e-13
  PD             states 9.4e-13  measured 4.9e-13  inputs 9.7e-14  g_sqrt_kp 5.4e-13  g_sqrt_kd 2.9e-13  g_x0 8.4e-13
  PID            states 6.2e-12  measured 6.2e-12  inputs 5.2e-13  integral 4.7e-14  g_sqrt_kp 1.2e-12  g_sqrt_kd 3.8e-12  g_sqrt_ki 2.2e-11
                 g_x0 9.5e-13
  TVL            states 1.3e-11  measured 3.8e-13  inputs 2.0e-12  g_gain 1.3e-12  g_ff 2.8e-12  g_x0 2.3e-12
  MLP            states 1.8e-12  inputs 2.3e-13  parameter gradients 9.4e-13  g_x0 3.5e-13
  linearisation  A 5.4e-13  B 9.9e-13  B scaled 8.8e-13;  against model_step's backward g^T A 3.4e-16  g^T B 2.4e-16
  pass           kernel against the float64 recursion 9.1e-16 at d_ref <= 8.1e-16 (bound 1e-12), cond(Quu) <= 5.6

What a wrong kernel would fail here, argued from the code (rollout_open.hip, lqr.hip; a local build with the first and the third
together failed 58 tests of this module, none on limits, and none of the parity cases of the families' own modules):
  - stage B' of the sweep taking ``k < (U & ~1)`` for ``k < U``: the last input of an odd U gets no abar -- its gain gradients stay 0 and
    its pull is read from an unwritten slot.  Every test_pd / test_pid / test_tvl case on cart, all_angle, g1_plain (U = 1), mixed5,
    d16_angles (U = 3) and d15_plain (U = 5) fails, e.g. test_pd[pd-sampled-mixed5-0-37-12-17]; the cases on limits (U = 8) and the
    families' own modules (U = 2, 6) do not notice.
  - stage C without the ``kvel`` pull: g_x0 and the gains' gradients of every test_pd / test_pid case with T >= 2; on mixed5 component 2
    takes the kpos pull of input 2 AND the kvel pull of input 0, so a form that applied one of the two only (an ``else``) fails
    test_pd[pd-sampled-mixed5-0-37-12-17] and passes everywhere else.
  - ``ogt[r] < 0`` giving the identity row in lqr_a_elem: A[0][0] = 1 on g1_plain, A[6][6] = 1 on d16_angles -- test_linearisation on
    those two layouts (against autograd and the exact zero rows) and test_pass (the zero rows, then the recursion) fail.
  - reduce_row stopping at ``16 * (U (S + 1) / 16)``: the tail entries of the partial are never written -- g_gain / g_ff of
    test_tvl on mixed5 (18 = 16 + 2), d16_angles (24), d15_plain (55), limits (136) and, with 10 < 16, every case with U (S + 1) < 16.
"""
import pytest
import torch

import closed_loop_family as clf
import layout_models as lay
import test_gpu_lqr as t_lqr
import test_gpu_mlp_rollout as t_mlp
import test_gpu_model_step as t_step
import test_gpu_open_rollout_grad as t_open
import test_gpu_pd_rollout as t_pd
import test_gpu_pid_rollout as t_pid
import test_gpu_tvl_rollout as t_tvl
from closed_loop_family import Family, controller, policy
from closed_loop_family import meas_spec as spec
from gpu_helpers import DT, G, dev, relmax

pytestmark = pytest.mark.gpu

# the families of the four modules over this table's pairs
PD, PID, TVL, MLP = (Family(f.op_name, f.params, f.grad_text, lay, lay.pair_seed) for f in (clf.PD, t_pid.PID, t_tvl.TVL, clf.MLP))


def pair(layout, N, deg):
    """(record, oracle model, PackedModel), with the sampling time a measurement model needs on the delta-state layout too."""
    return PD.pair(layout, N, deg, None, measured=True)


def noise(case, eps):
    return clf.noise_buffer(eps) if case.mode == "sampled" else None


def cases(form):
    return pytest.mark.parametrize("case", lay.of_form(form), ids=lay.case_id)


def unintegrated(c):
    """The components no GP writes."""
    return [s for s in range(c["S"]) if s not in c["vel"] and s not in c["not_vel"]]


# ---- open loop ------------------------------------------------------------------------------------------------------------------------------
@cases("open")
def test_open_loop(case):
    """States, g_x0 and g_u of rollout_open_diff, and the moments of rollout_open on the same arguments: a GP whose thread did not report
    would leave its mu / var rows unwritten."""
    from mc_pilco_amd import ops

    r = lay.case_truth(case)
    ins, (ost, ogx, ogu, vmin), sample = r["ins"], r["truth"], case.mode == "sampled"
    c, m, pm = pair(case.layout, case.N, case.deg)
    st, gx, gu, status = t_open.gpu_grads(pm, ins["x0"], ins["u"], ins["eps"], ins["w"], sample, lengths=ins["lengths"])
    sp, mu, var, status_p = ops.rollout_open(pm, G(ins["x0"]), G(ins["u"]), lengths=ins["lengths"], noise=noise(case, ins["eps"]), particle_pred=sample,
                                             moments=True)
    es, ex, eu = float((st.cpu() - ost).abs().max()), relmax(gx, ogx), relmax(gu, ogu)
    em, ev = float((mu.cpu() - r["mu"]).abs().max()), float((var.cpu() - r["var"]).abs().max())
    print("%s: states %.3e g_x0 %.3e g_u %.3e mean %.3e var %.3e (min var %.3e)" % (lay.case_id(case), es, ex, eu, em, ev, vmin))
    assert status == 0 and int(status_p.item()) == 0 and torch.equal(sp, st)
    assert es < t_open.STATE_TOL and ex < t_open.GRAD_TOL and eu < t_open.GRAD_TOL
    assert em < t_step.TOL and ev < t_step.TOL
    assert float(r["var"].max()) > 0.0 and tuple(mu.shape) == (case.T - 1, case.M, c["G"])
    if ins["lengths"] is not None:
        for p, ln in enumerate(ins["lengths"]):
            assert bool((gu[ln - 1:, p, :] == 0).all()) and bool((st[ln:, p] == 0).all())
            assert bool((mu[ln - 1:, p] == 0).all()) and bool((var[ln - 1:, p] == 0).all())
    for s in unintegrated(c):
        assert float(st[1:, :, s].abs().max()) == 0.0


# ---- model step -----------------------------------------------------------------------------------------------------------------------------
@cases("step")
def test_model_step(case):
    from mc_pilco_amd import ops

    r = lay.case_truth(case)
    ins, (onx, omu, ovar, ogx, ogu), sample = r["ins"], r["truth"], case.mode == "sampled"
    c, m, pm = pair(case.layout, case.N, case.deg)
    xg, ug = G(ins["x"]).requires_grad_(True), G(ins["u"]).requires_grad_(True)
    nx, mu, var, status = ops.model_step(pm, xg, ug, 0, noise=ops.NoiseSpec(eps=G(ins["eps"])) if sample else None, particle_pred=sample, moments=True)
    (G(ins["w"]) * nx).sum().backward()
    ex, em, ev = (float((a.detach().cpu() - b).abs().max()) for a, b in ((nx, onx), (mu, omu), (var, ovar)))
    egx, egu = relmax(xg.grad, ogx), relmax(ug.grad, ogu)
    print("%s: x_next %.3e mean %.3e var %.3e g_x %.3e g_u %.3e" % (lay.case_id(case), ex, em, ev, egx, egu))
    assert int(status.item()) == 0
    assert max(ex, em, ev, egx, egu) < t_step.TOL
    for s in unintegrated(c):
        assert float(nx.detach()[:, s].abs().max()) == 0.0


# ---- the closed loops -------------------------------------------------------------------------------------------------------------------------
@cases("pd")
def test_pd(case):
    r = lay.case_truth(case)
    i, truth = r["ins"], clf.pd_truth_of(r["truth"])
    c, m, pm = pair(case.layout, case.N, case.deg)
    pol = controller(c, i["kp"], i["kd"], i["target"])
    got = PD.run(pm, pol, i["x0"], case.T, noise(case, i["eps"]), i["w"], i["wu"], case.mode == "sampled", meas=spec(i["ms"], i["pn"]))
    clf.check_against(PD, lay.case_id(case), truth, got, t_pd.TOLS)


@cases("pid")
def test_pid(case):
    r = lay.case_truth(case)
    i, truth = r["ins"], r["truth"]
    c, m, pm = pair(case.layout, case.N, case.deg)
    pol = t_pid.pid_controller(c, i["kp"], i["kd"], i["ki"], i["target"], i_max=i["i_max"])
    got = PID.run(pm, pol, i["x0"], case.T, noise(case, i["eps"]), i["w"], i["wu"], case.mode == "sampled", meas=spec(i["ms"], i["pn"]))
    ei = t_pid.integ_error(pol, truth)
    print("integ %.3e" % ei)
    clf.check_against(PID, lay.case_id(case), t_pid.truth_of(truth), got, t_pid.TOLS)
    assert ei < t_pid.STATE_TOL


@cases("tvl")
def test_tvl(case):
    r = lay.case_truth(case)
    i, truth = r["ins"], r["truth"]
    c, m, pm = pair(case.layout, case.N, case.deg)
    pol = t_tvl.tv_controller(c, i["gain"], i["ff"], i["target"])
    got = TVL.run(pm, pol, i["x0"], case.T, noise(case, i["eps"]), i["w"], i["wu"], case.mode == "sampled", meas=spec(i["ms"], i["pn"]))
    clf.check_against(TVL, lay.case_id(case), t_tvl.truth_of(truth), got, t_tvl.TOLS)
    assert all(tuple(g.shape) == tuple(q.shape) for g, q in zip(got.grads, TVL.params(pol)))


@cases("mlp")
def test_mlp(case):
    r = lay.case_truth(case)
    i, truth = r["ins"], clf.mlp_truth_of(r["truth"])
    c, m, pm = pair(case.layout, case.N, case.deg)
    pol = policy(c, i["params"], case.opt["hidden"], i["angle"], i["non_angle"])
    got = MLP.run(pm, pol, i["x0"], case.T, noise(case, i["eps"]), i["w"], i["wu"], case.mode == "sampled")
    clf.check_against(MLP, lay.case_id(case), truth, got, t_mlp.TOLS)


# ---- linearisation and pass -------------------------------------------------------------------------------------------------------------------
def _record(case, pm, sample):
    from mc_pilco_amd import ops

    x0, a, u, du, eps, target = lay.case_truth(case)["ins"]
    states, jac, status = ops.rollout_open_record(pm, G(x0), G(u[:case.T - 1]), noise=ops.NoiseSpec(eps=G(eps)) if sample else None, particle_pred=sample)
    assert int(status.item()) == 0
    return states, jac


def _zero_rows(c, *tensors):
    """The rows of A / B that belong to a component no GP integrates are exactly 0.0 (the rollouts write that component as 0)."""
    for s in unintegrated(c):
        for t in tensors:
            assert float(t[:, :, s, :].abs().max()) == 0.0


@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
@cases("lin")
def test_linearisation(case, sample):
    from mc_pilco_amd import ops

    r = lay.case_truth(case)
    (x0, a, u, du, eps, target), (st_o, At, Bt) = r["ins"], r[sample]
    c, m, pm = pair(case.layout, case.N, case.deg)
    T, M = case.T, case.M
    states, jac = _record(case, pm, sample)
    assert float((states.cpu() - st_o).abs().max()) < 1e-9
    A, B = ops.linearize(pm, states, jac)
    As, Bs = ops.linearize(pm, states, jac, du_da=G(du))
    ea, eb, ebs = relmax(A, At), relmax(B, Bt), relmax(Bs, Bt * du[:T - 1].unsqueeze(2))
    print("%s %s: A %.3e B %.3e B scaled %.3e" % (lay.case_id(case), "sampled" if sample else "mean", ea, eb, ebs))
    assert tuple(A.shape) == (T - 1, M, c["S"], c["S"]) and tuple(B.shape) == (T - 1, M, c["S"], c["U"])
    assert max(ea, eb, ebs) < t_lqr.GRAD_TOL and torch.equal(As, A)
    _zero_rows(c, A, B, Bs)
    gen = torch.Generator().manual_seed(5)
    g = G(torch.randn(M, c["S"], dtype=DT, generator=gen))
    for t in sorted({0, T - 2}):
        xg, ug = states[t].clone().requires_grad_(True), G(u[t]).requires_grad_(True)
        nxt, status = ops.model_step(pm, xg, ug, t, noise=ops.NoiseSpec(eps=G(eps[t])) if sample else None, particle_pred=sample)
        (g * nxt).sum().backward()
        ga, gb = torch.einsum("mr,mrc->mc", g, A[t]), torch.einsum("mr,mrk->mk", g, B[t])
        ex, eu = relmax(ga, xg.grad), relmax(gb, ug.grad)
        print("   row %d against model_step's backward: g^T A %.3e g^T B %.3e" % (t, ex, eu))
        assert int(status.item()) == 0 and torch.equal(nxt.detach(), states[t + 1]) and max(ex, eu) < t_lqr.STEP_TOL


@cases("pass")
def test_pass(case):
    """ops.lqr_pass against riccati_truth / riccati_truth_ld on the kernel's own A, B, as tests/test_gpu_lqr.py::test_pass_against_the_recursion."""
    from mc_pilco_amd import ops

    x0, a, u, du, eps, target = lay.case_truth(case)["ins"]
    c, m, pm = pair(case.layout, case.N, case.deg)
    T, M, reg = case.T, case.M, case.opt["reg"]
    states, jac = _record(case, pm, False)
    J, lx, lu, hxx, huu, s = t_lqr.cost_rows(c, T, states, a, target)
    assert float((s.cpu() - du).abs().max()) < 1e-15
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    got = ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=reg, du_da=s, status=status)
    assert int(status.item()) == 0 and tuple(got[0].shape) == (M, T, c["U"], c["S"]) and tuple(got[1].shape) == (M, T, c["U"]) and tuple(got[2].shape) == (M, 2)
    assert float(got[0][:, T - 1].abs().max()) == 0.0
    A, B = ops.linearize(pm, states, jac, du_da=s)
    _zero_rows(c, A, B)
    f64, ld, cond = t_lqr.truth_of_the_pass(A, B, (lx, lu, hxx, huu), reg)
    t_lqr.check_pass(lay.case_id(case), got, f64, ld, cond)
    assert bool((got[2][:, 0] < 0).all()) and bool((got[2][:, 1] > 0).all())


# ---- bits -------------------------------------------------------------------------------------------------------------------------------------
def _laws(layout, M, T, seed):
    import tvl_models as tm

    c, m, pm = pair(layout, 37, 1)
    x0, kp, kd, target, eps, w, wu, gain, ff = tm.tvl_inputs(c, M, T, seed)
    return pm, x0, eps, w, wu, ((PD, lambda: controller(c, kp, kd, target)), (TVL, lambda: t_tvl.tv_controller(c, gain, ff, target)))


@pytest.mark.parametrize("layout", list(lay.LAYOUTS))
def test_closed_loop_open_loop_and_recording_launch_carry_the_same_bits(layout):
    pm, x0, eps, w, wu, laws = _laws(layout, 17, 6, 21)
    for fam, make in laws:
        clf.three_way_bit_identity(fam, pm, make(), x0, eps, 6, "eps", sweep=(w, wu))


@pytest.mark.parametrize("layout", list(lay.LAYOUTS))
def test_the_bits_of_a_trajectory_do_not_depend_on_M(layout):
    """A launch at M = 33 (three tiles, the last ragged) against launches of its slices [0:16], [16:32], [32:33]: states, inputs and g_x0."""
    M, T = 33, 3
    pm, x0, eps, w, wu, laws = _laws(layout, M, T, 23)
    for fam, make in laws:
        pol = make()
        run = lambda sl: fam.run(pm, pol, x0[sl], T, clf.noise_buffer(eps[:, sl]), w[:, sl], wu[:, sl], True)
        whole = run(slice(0, M))
        assert whole.status == 0 and bool(torch.isfinite(whole.g_x0).all()) and float(whole.g_x0.abs().max()) > 0.0
        for sl in (slice(0, 16), slice(16, 32), slice(32, 33)):
            part = run(sl)
            assert part.status == 0
            assert torch.equal(part.states, whole.states[:, sl]) and torch.equal(part.inputs, whole.inputs[:, sl])
            assert torch.equal(part.g_x0, whole.g_x0[sl])
