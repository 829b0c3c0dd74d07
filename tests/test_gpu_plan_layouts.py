"""GPU: the sampling planner's rollout entries -- mcp_mppi_rollout and mcp_plan_rollout (csrc/mppi.hip) -- on the irregular layouts of
tests/layout_models.py, at the tile shapes, horizons and options of tests/plan_models.py (what each row pins is written there;
tests/test_plan_models_cpu.py holds the truth's conditions without a GPU); the status word of both entries; the update kernels at the
widths and counts tests/test_gpu_mppi.py and tests/test_gpu_plan_ext.py did not reach; one driver case.

Bounds, imported and not restated: torch.equal for the bit identities; INPUT_LAW_TOL (1e-14) and ORACLE_TOL (1e-9) of
tests/test_gpu_mppi.py; its bound(d_ref) for the updates; its ULP_BOUND where Philox values are compared.

  1. state bits     states == ops.rollout_open on the launch's own inputs with the eps buffer repeated per candidate; candidate 0 == the
                    open loop on the nominal alone; traj_cost unchanged by the optional outputs; unintegrated components exactly 0 from row
                    1 on; the long rows: the first rows of the two neighbouring horizons carry the same bits (16- against 4-rung).
  2. input law      squash(a + sigma xi) -- under the extension squash(a[t] + s(t) xi_t), xi_t cem_truth.colour's -- per input with its own
                    u_max and sigma; the input with sigma == 0 carries the nominal's bits for every candidate; every particle alike.
  3. cost bits      traj_cost == the ascending sum over t of the cost kernels' costs on those states and inputs, under every descriptor of
                    plan_models.cost_specs, with and without time weights, target rows t0 .. t0 + H - 1; with u_prev on a record with
                    u_prev prepended.
  4. oracle         states and costs of every row with H <= 6 against mppi_truth.oracle_states / plan_models.traj_costs.
  5. Philox         per layout: common random numbers by particle id against rollout_open under the same NoiseSpec; the perturbations
                    against the 64-bit-significand truth.
  6. status         var_scale = 0, Kinv scaled past the sign change, a NaN in xi, a NaN in x0: the word the oracle's record gives.
  7. updates        U in {1, 8}, K in {1, 2, 255, 256, 257}, H = 2, P = 2 with kappa != 0, costs of mixed sign, a floor per input.
  8. driver         mppi.plan(method="cem" / "mppi") on mixed5 == the launches chained by hand; MPPI_controller's first input.

What a wrong kernel would fail here, argued from mppi.hip.  None of these was built and run: every one is ARGUED only.
  - the slot of an angle in ``z`` taken from the component's rank among the angles (what a kernel that assumed a sorted list would do)
    instead of ``zi_ang``, its index in ``md.angle``: identical on every sorted list, so on arm2, arm2_delta, ur5 and on all layouts here
    but mixed5 (angle = [4, 0]), where sin / cos of components 0 and 4 change places.  The four mixed5 rows of
    test_state_bits_and_the_input_law (against rollout_open), test_against_the_oracle and test_cost_bits fail, nothing else.  (``zi_ang``
    found by the first match in place of the last is no defect: a valid list names no component twice.)
  - ``zi_plain`` and ``zi_ang`` made exclusive (an ``else``): component 0 of mixed5 is plain AND an angle and would lose one feature; the
    same four rows; tests/test_layout_models_cpu.py's sensitivity argument, which tests/test_plan_models_cpu.py repeats for the planner.
  - a component no GP writes carried over (``nx = xc[os]`` for ``og < 0``) instead of zeroed: g1_plain (component 0) and d16_angles
    (component 6, a GP input) -- the exact zeros of test_state_bits_and_the_input_law, the oracle, and the cost under "wide", whose
    active dimensions include that component.  No regular model has such a component.
  - the three thread sets sized from S, ``isu = ut < PT * (S / 2)``: right on arm2 / ur5 and on all_angle (U = 1 = S / 2), wrong on cart,
    g1_plain, mixed5 and d16_angles -- wherever U != S / 2 (d15_plain has U = S / 2 and passes): inputs of the missing threads stay
    0, or cost threads double as input threads.  ``PT (S + U + 1) <= 512`` holds with 112 threads to spare at the limits row only.
  - the cost thread reading the inputs with ``up`` (0 outside the input threads) in place of ``ct``: every trajectory of a tile is
    charged trajectory 0's input terms.  The old tests see it under "target_add" (every input charged, every sigma > 0).  Under "wide"
    and "traj_rate" (input U - 1 alone) with sigma[U // 2] = 0 the same defect restricted to ONE column -- ``ur[k]`` read at the wrong
    ``k`` -- shows only where the charged input and the unperturbed one differ: every row with U >= 2 of test_cost_bits.
  - ``ub``'s slot of row -1: u_prev staged in the slot of the even rows.  Row 0 overwrites it before its own cost is formed, the rate
    term of row 0 is taken against u_0 itself (0): test_cost_bits under every descriptor with a rate term on the rows with u_prev, and
    the ``with / without u_prev`` comparison at its end; at H = 3 (cart, g1_plain, mixed5, d16_angles, limits) row 2 then reads the slot
    row 0 wrote, which a buffer of three slots would hide at H = 2.
  - the status of a GP reported by its POSITION thread (``og == g_pos``) in place of the velocity thread: GP 1 of mixed5 has no position
    and would never report.  Constructions A-first / A-last / B pick GPs 0 and 2, which have one; ``A-mid`` (g* = 1) is here for this:
    test_the_status_word_of_the_rollout_entries[*mixed5*-A-mid] would read word 0 for NONPOS_VAR.
  - ``nom`` / ``srow`` sized or staged with S for U (``it < T * S``, ``srow = ub + 2 * PT * S``): inside the region wherever it has room
    to spare; at H = 1866 (mppi) and H = 933 (plan) the region ends exactly at the 160 KiB limit, and the rows past the nominal are the
    std's: test_state_bits_and_the_input_law (the law per row) and test_cost_bits on the two rows at the last fitting horizon.

A defect this module did find (fixed in mppi.hip, ``mppi_sincos``): sincos_fast sends a whole wave through the library's sincos when one
lane holds a NaN, and the two differ in the last bit now and then; a candidate lost to a NaN in xi moved states of healthy trajectories
sharing its wave (mixed5: trajectories 0 and 4 from row 3 on, by one ulp).  test_the_status_word_of_the_rollout_entries[*-X-first] failed on
it before the fix.

Worst measured on an MI355X over the cases of each form (every one inside its bound by two orders or more):
  input law        |inputs - law| 4.4e-16 over the 26 rows, the long ones included (INPUT_LAW_TOL 1e-14)
  oracle, mppi     states 2.2e-12  inputs 4.4e-16  traj_cost 1.6e-12 (ORACLE_TOL 1e-9)
  oracle, plan     states 4.9e-13  inputs 3.3e-16  traj_cost 1.4e-13
  Philox           the perturbations within 1.75 ulp of the 64-bit-significand truth (ULP_BOUND 8)
  status           finite states 8.0e-15, finite costs 2.5e-16 against the oracle over the 44 constructions
  updates          a_new, cand_cost, weights, sigma_new within 2.1e-16 of the float64 truth at d_ref <= 4.5e-16 (bound 1e-12)
  bit identities   torch.equal throughout (rollout_open, the cost kernels, the neighbouring horizons, Philox == buffer, the driver)
The longest test is the H = 1866 row of test_state_bits_and_the_input_law, 1.9 s; the module runs in 12 s.
"""
import numpy as np
import pytest
import torch

import cem_truth as ct
import closed_loop_family as clf
import layout_models as lay
import mppi_truth as mt
import noise_truth as nt
import pd_models
import plan_models as pl
import status_models as sm
from gpu_helpers import DT, G, dev, spec_from
from test_gpu_mppi import INPUT_LAW_TOL, ORACLE_TOL, ULP_BOUND, bound, check_update, cost_object
from test_gpu_plan_ext import check_cem

pytestmark = pytest.mark.gpu
n_ = lambda v: v.detach().cpu().numpy()  # noqa: E731


def cases(which):
    return pytest.mark.parametrize("case", which, ids=pl.case_id)


def pair(layout, N, deg):
    """(record, oracle model, PackedModel): the pairs of tests/test_gpu_layouts.py (one build per process, whoever asks)."""
    return clf.pair(lay.build_pair, layout, N, deg, lay.pair_seed(N, deg), None, pd_models.family(layout) == "delta", True)


def packed_costs(spec, S, U, rows=None):
    """(PackedCost, PackedCostInputs or None); ``rows``: the target rows of a trajectory cost, as the cost kernels (which read row t at
    step t) are to see them."""
    from mc_pilco_amd import ops

    if spec["kind"] == "traj":
        pc = ops.PackedCost("traj", S, dev(), target_traj=spec["target"] if rows is None else rows, lengthscales=spec["ls"], used=spec["idx"])
    else:
        pc = ops.PackedCost("target", S, dev(), target_state=spec["target"], lengthscales=spec["ls"], active_dims=spec["idx"],
                            saturate=spec["kind"] == "target")
    cin = None
    if spec.get("u_idx") is not None:
        cin = ops.PackedCostInputs(U, dev(), spec["u_idx"], spec.get("u_ls"), spec.get("u_rate"), spec.get("u_target"), bool(spec.get("joint")))
    return pc, cin


def descriptors(case, op, lam=1.0, kappa=0.0, **ext_kw):
    from mc_pilco_amd import ops

    U = lay.LAYOUTS[case.layout]["U"]
    mp = ops.PackedMPPI(case.K, case.P, case.H, U, op["sigma"], lam, kappa, u_max=op["u_max"], squash=op["squash"])
    ext = ops.PackedPlanExt(case.H, U, beta=op["beta"], sigma_rows=op["rows"], **ext_kw) if pl.is_ext(case) else None
    return mp, ext


def launch(case, pm, spec=None, w=None, t0=None, xi="own", x0=None, noise="own", want_states=True, want_inputs=True, a=None, mp=None, sample=None):
    """One rollout-cost launch of the case's entry on its operands; returns (J, states, inputs, status word)."""
    from mc_pilco_amd import ops

    cfg, op = lay.LAYOUTS[case.layout], pl.operands(case)
    sample = (case.mode == "sampled") if sample is None else sample
    mp0, ext = descriptors(case, op)
    mp = mp0 if mp is None else mp
    spec = pl.cost_specs(case.layout)[case.opt["cost"]] if spec is None else spec
    pc, cin = packed_costs(spec, cfg["S"], cfg["U"])
    if isinstance(noise, str):
        noise = ops.NoiseSpec(eps=G(op["eps"])) if sample else None
    kw = dict(cost_inputs=cin, noise=noise, particle_pred=sample, xi=G(op["xi"]) if isinstance(xi, str) else xi, w=None if w is None else G(w),
              t0=op["t0"] if t0 is None else t0, want_states=want_states, want_inputs=want_inputs)
    x0 = G(op["x0"] if x0 is None else x0)
    a = G(op["a"]) if a is None else a
    if pl.is_ext(case):
        J, st, inp, status = ops.plan_rollout(pm, mp, ext, pc, x0, a, u_prev=None if op["u_prev"] is None else G(op["u_prev"]), **kw)
    else:
        J, st, inp, status = ops.mppi_rollout(pm, mp, pc, x0, a, **kw)
    return J, st, inp, int(status.item())


# ---- 1, 2. state bits and the input law -------------------------------------------------------------------------------------------------------
@cases(pl.CASES)
def test_state_bits_and_the_input_law(case):
    from mc_pilco_amd import ops

    cfg, op = lay.LAYOUTS[case.layout], pl.operands(case)
    c, m, pm = pair(case.layout, case.N, case.deg)
    H, K, P, S, U, M, sample = case.H, case.K, case.P, cfg["S"], cfg["U"], case.K * case.P, case.mode == "sampled"
    J, st, inp, status = launch(case, pm)
    assert status == 0 and tuple(st.shape) == (H, M, S) and tuple(inp.shape) == (H, M, U) and tuple(J.shape) == (M,) and bool(torch.isfinite(J).all())
    x0m, eps = G(op["x0"]).reshape(1, -1).repeat(M, 1).contiguous(), G(op["eps"])
    full = ops.NoiseSpec(eps=eps.repeat(1, K, 1).contiguous()) if sample else None  # trajectory k P + p meets particle p's draws
    ref, s2 = ops.rollout_open(pm, x0m, inp[:H - 1].contiguous(), noise=full, particle_pred=sample)
    assert int(s2.item()) == 0 and torch.equal(st, ref)
    nom, s2 = ops.rollout_open(pm, x0m[:P].contiguous(), inp[:H - 1, :P].contiguous(), noise=ops.NoiseSpec(eps=eps) if sample else None, particle_pred=sample)
    assert int(s2.item()) == 0 and torch.equal(st[:, :P], nom)
    for ws, wi in ((False, False), (True, False), (False, True)):
        J2, st2, inp2, status = launch(case, pm, want_states=ws, want_inputs=wi)
        assert status == 0 and torch.equal(J2, J) and (st2 is None) == (not ws) and (inp2 is None) == (not wi)
        assert (st2 is None or torch.equal(st2, st)) and (inp2 is None or torch.equal(inp2, inp))
    # the law, per input; every particle of a candidate alike; candidate 0 the nominal whatever xi holds for it
    got = inp.reshape(H, K, P, U)
    assert torch.equal(got, got[:, :, :1].expand(H, K, P, U))
    want = pl.candidate_inputs(case, op)
    err = float(np.abs(n_(got[:, :, 0]) - want).max())
    print("%s: |inputs - law| %.3e (asserted %.0e)" % (pl.case_id(case), err, INPUT_LAW_TOL))
    assert err < INPUT_LAW_TOL
    z = pl.zero_input(U)
    if z is not None:  # sigma == 0: the nominal's bits for every candidate
        assert torch.equal(got[..., z], got[:, :1, :1, z].expand(H, K, P))
    if K > 1:
        assert float((got[:, 1:, 0] - got[:, :1, 0]).abs().max()) > 1e-3
    # components no GP writes
    for s in pl.unintegrated(cfg):
        assert float(st[1:, :, s].abs().max()) == 0.0 and bool((st[0, :, s] == float(op["x0"][s])).all())


@pytest.mark.parametrize("entry", ["mppi", "plan"])
def test_the_bits_of_a_trajectory_do_not_depend_on_the_rung(entry):
    """The last horizon of the 16-trajectory rung and the first of the 4-rung (plan_models.LONG): the shorter plan is the prefix of the
    longer one's operands, so its states and inputs are the first rows of the longer one's."""
    fit, beyond = (c for c in pl.LONG_CASES if c.entry == entry and c.mode == "sampled")
    assert fit.H + 1 == beyond.H and pl.rung("limits", 37, fit.H, True, pl.is_ext(fit))[0] == 16 and pl.rung("limits", 37, beyond.H, True, pl.is_ext(fit))[0] == 4
    c, m, pm = pair(fit.layout, fit.N, fit.deg)
    _, st1, in1, s1 = launch(fit, pm)
    _, st2, in2, s2 = launch(beyond, pm)
    assert s1 == 0 and s2 == 0 and torch.equal(st1, st2[:fit.H]) and torch.equal(in1, in2[:fit.H])
    assert bool(torch.isfinite(st2).all()) and float((st2[-1] - st2[0]).abs().max()) > 1e-3


# ---- 3. cost bits ---------------------------------------------------------------------------------------------------------------------------
def kernel_costs(case, op, spec, t0, st, inp, w):
    """The ascending sum over t of the cost kernels' costs on the launch's states and inputs at target rows t0 .. t0 + H - 1; with u_prev
    and input terms: on a record with a dummy state and u_prev prepended (tests/test_gpu_plan_ext.py's idiom), rows 1 .. H."""
    from mc_pilco_amd import ops

    cfg, H, M = lay.LAYOUTS[case.layout], case.H, case.K * case.P
    rows = np.asarray(spec["target"])[t0:t0 + H] if spec["kind"] == "traj" else None
    pre = op["u_prev"] is not None and spec.get("u_idx") is not None
    if pre:
        rows = None if rows is None else np.concatenate([rows[:1], rows])
        st = torch.cat([st[:1], st]).contiguous()
        inp = torch.cat([G(op["u_prev"]).reshape(1, 1, -1).expand(1, M, -1), inp]).contiguous()
    pc, cin = packed_costs(spec, cfg["S"], cfg["U"], rows)
    status = torch.zeros(1, dtype=torch.int32, device=dev())  # (a word of this call's own: without one the flags go to a shared sink)
    _, costs, status = ops.cost_moments(pc, st, status=status, inputs=None if cin is None else inp, cost_inputs=cin)
    assert int(status.item()) == 0
    acc = torch.zeros(M, dtype=DT, device=dev())
    for t in range(H):  # ascending, one rounding per product and per sum
        ct_ = costs[t + 1] if pre else costs[t]
        acc = acc + (ct_ if w is None else float(w[t]) * ct_)
    return acc


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@cases(pl.CASES)
def test_cost_bits_against_the_cost_kernels(case, weighted):
    op = pl.operands(case)
    c, m, pm = pair(case.layout, case.N, case.deg)
    specs = pl.cost_specs(case.layout)
    names = sorted(specs) if case.H <= pl.H_SHORT else [case.opt["cost"]]
    t0 = op["t0"] or 1
    w = op["w"] if weighted else None
    for name in names:
        J, st, inp, status = launch(case, pm, spec=specs[name], w=w, t0=t0)
        acc = kernel_costs(case, op, specs[name], t0, st, inp, w)
        assert status == 0 and bool(torch.isfinite(J).all()) and float(J.abs().min()) > 0, name
        assert torch.equal(J, acc), (name, float((J - acc).abs().max()))
        if specs[name]["kind"] == "traj":  # the offset matters
            assert not torch.equal(launch(case, pm, spec=specs[name], w=w, t0=0)[0], J)
    if op["u_prev"] is not None:  # u_prev reaches row 0's rate term, and nothing without one
        from mc_pilco_amd import ops

        mp, ext = descriptors(case, op)
        for name, moves in (("wide", True), ("effort", False)):
            pc, cin = packed_costs(specs[name], c["S"], c["U"])
            kw = dict(cost_inputs=cin, noise=ops.NoiseSpec(eps=G(op["eps"])) if case.mode == "sampled" else None, particle_pred=case.mode == "sampled",
                      xi=G(op["xi"]), t0=t0)
            with_ = ops.plan_rollout(pm, mp, ext, pc, G(op["x0"]), G(op["a"]), u_prev=G(op["u_prev"]), **kw)[0]
            without = ops.plan_rollout(pm, mp, ext, pc, G(op["x0"]), G(op["a"]), **kw)[0]
            assert torch.equal(with_, without) != moves, name


# ---- 4. the oracle ----------------------------------------------------------------------------------------------------------------------------
@cases(pl.SHORT)
def test_against_the_oracle(case):
    r = pl.case_truth(case)
    c, m, pm = pair(case.layout, case.N, case.deg)
    J, st, inp, status = launch(case, pm)
    es, eu, ej = float(np.abs(n_(st) - r["x"]).max()), float(np.abs(n_(inp) - r["u"]).max()), float(np.abs(n_(J) - r["J"]).max() / np.abs(r["J"]).max())
    print("%s %s: states %.3e inputs %.3e traj_cost %.3e (asserted %.0e)" % (case.entry, pl.case_id(case), es, eu, ej, ORACLE_TOL))
    assert status == 0 and es < ORACLE_TOL and ej < ORACLE_TOL and eu < INPUT_LAW_TOL


# ---- 5. Philox --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(lay.LAYOUTS))
def test_philox_common_random_numbers_by_particle_id(layout):
    """The layout's sampled mppi row without buffers: every candidate's P trajectories are rollout_open's with M = P under the same
    NoiseSpec (particle ids 0 .. P - 1); the perturbations (a = 0, sigma = 1, no squashing) against the 64-bit-significand truth."""
    from mc_pilco_amd import ops

    case = next(c for c in pl.SHORT if c.layout == layout and c.entry == "mppi" and c.mode == "sampled")
    cfg, op = lay.LAYOUTS[layout], pl.operands(case)
    c, m, pm = pair(layout, case.N, case.deg)
    H, K, P, U = case.H, case.K, case.P, cfg["U"]
    nz = ops.NoiseSpec(seed=11, call=3)
    J, st, inp, status = launch(case, pm, xi=None, noise=nz)
    assert status == 0 and bool(torch.isfinite(J).all())
    x0p = G(op["x0"]).reshape(1, -1).repeat(P, 1).contiguous()
    for k in sorted({0, K // 2, K - 1}):
        ref, s2 = ops.rollout_open(pm, x0p, inp[:H - 1, k * P:(k + 1) * P].contiguous(), noise=nz, particle_pred=True)
        assert int(s2.item()) == 0 and torch.equal(st[:, k * P:(k + 1) * P], ref), k
    if K > 1:
        raw = ops.PackedMPPI(K, P, H, U, 1.0, 1.0, squash=False)
        got = launch(case, pm, xi=None, noise=nz, a=torch.zeros(H, U, dtype=DT, device=dev()), mp=raw)[2].reshape(H, K, P, U)
        assert not bool(got[:, 0].any()) and torch.equal(got, got[:, :, :1].expand(H, K, P, U))
        g = n_(got[:, 1:, 0])
        if nt.have_longdouble():
            ulp = float(nt.ulps(g, mt.xi_table(11, 3, H, K, U, 0, hp=True)[:, 1:]).max())
            print("%s: %d draws within %.3f ulp of the truth (asserted %.0f)" % (layout, g.size, ulp, ULP_BOUND))
            assert ulp <= ULP_BOUND
        else:  # numpy's double evaluation is itself within 4 ulp of that truth (tests/test_noise_truth_cpu.py)
            t64 = mt.xi_table(11, 3, H, K, U, 0)[:, 1:]
            assert float((np.abs(g - t64) / np.spacing(np.abs(t64))).max()) <= ULP_BOUND + 4.0
        Jb, stb, inb, status = launch(case, pm, xi=got[:, :, 0].contiguous(), noise=nz)  # Philox == the buffer fed those draws
        assert status == 0 and torch.equal(Jb, J) and torch.equal(stb, st) and torch.equal(inb, inp)


# ---- 6. the status word -------------------------------------------------------------------------------------------------------------------------
def status_model(case, so):
    """The PackedModel on the construction's Kinv and var_scale (the operands status_models-style: what the oracle is given)."""
    from mc_pilco_amd import ops

    if so["factor"] is None and so["var_scale"] is None:
        return pair(case.layout, case.N, case.deg)[2]
    c, m, specs = lay.oracle_pair(case.layout, case.N, case.deg)
    gps = [ops.PackedGP(spec_from(*specs[g]), G(m.cache[g].X), G(m.cache[g].alpha),
                        G(m.cache[g].Kinv * so["factor"] if so["factor"] is not None and g == so["gstar"] else m.cache[g].Kinv)) for g in range(c["G"])]
    return ops.PackedModel(gps, c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"], var_scale=so["var_scale"])


def same_where_finite(got, want, tol, rel=False):
    got, fin = n_(got), np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    if not fin.any():
        return 0.0
    e = float(np.abs(got[fin] - want[fin]).max() / (np.abs(want[fin]).max() if rel else 1.0))
    assert e < tol, e
    return e


@pytest.mark.parametrize("con", pl.CONS, ids=lambda c: c.id)
@cases(pl.STATUS_BASE)
def test_the_status_word_of_the_rollout_entries(case, con):
    from mc_pilco_amd import ops

    cfg, op, so, tr = lay.LAYOUTS[case.layout], pl.operands(case), pl.status_operands(case, con), pl.status_truth(case, con)
    pm = status_model(case, so)
    K, P, H, U, M = case.K, case.P, case.H, cfg["U"], case.K * case.P
    xi = G(so["xi"])
    J, st, inp, word = launch(case, pm, xi=xi, x0=so["x0"], noise=ops.NoiseSpec(eps=G(op["eps"])) if so["sample"] else None, sample=so["sample"])
    assert word == tr["word"] == pl.expected_word(con) and not word & ~(sm.STATUS_NAN | sm.STATUS_NONPOS_VAR)
    es, ej = same_where_finite(st, tr["x"], ORACLE_TOL), same_where_finite(J, tr["J"], ORACLE_TOL, rel=True)
    same_where_finite(inp, tr["u"], INPUT_LAW_TOL)
    print("%s %s %s: word %d, finite states %.3e finite costs %.3e" % (case.entry, pl.case_id(case), con.id, word, es, ej))
    mp, ext = descriptors(case, op, lam=0.7, kappa=0.5)
    cem = ops.PackedPlanExt(H, U, beta=op["beta"], sigma_rows=op["rows"], n_elite=3, alpha=0.2, sigma_min=0.05)
    a = G(op["a"])
    if con.kind in ("A",) or con.mean:
        assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(st).all())
    if con.kind in ("B", "C") and not con.mean:  # no finite candidate: the nominal and the std stay
        assert bool(torch.isnan(J).all())
        a_new, cand, wts, stats, status = ops.mppi_update(mp, J, a, xi=xi)
        assert int(status.item()) == sm.STATUS_NAN and torch.equal(a_new, a) and not bool(wts.any())
        assert float(stats[1]) == -1.0 and float(stats[2]) == 0.0 and bool(torch.isnan(stats[0])) and bool(torch.isnan(stats[3]))
        a_new, s_new, cand, elite, stats, status = ops.cem_update(mp, cem, J, a, xi=xi)
        s_in = G(pl.std_rows(op, H, U))
        assert int(status.item()) == sm.STATUS_NAN and torch.equal(a_new, a) and torch.equal(s_new, s_in) and elite.cpu().tolist() == [-1] * 3
    if con.kind == "X":  # candidate K_STAR alone is lost; every other trajectory carries the bits of the clean run
        Jc, stc, inc, wc = launch(case, pm)
        bad = list(range(pl.K_STAR * P, (pl.K_STAR + 1) * P))
        keep = [i for i in range(M) if i not in bad]
        assert wc == 0 and bool(torch.isnan(J[bad]).all())
        assert torch.equal(J[keep], Jc[keep]) and torch.equal(st[:, keep], stc[:, keep]) and torch.equal(inp[:, keep], inc[:, keep])
        a_new, cand, wts, stats, status = ops.mppi_update(mp, J, a, xi=xi)
        assert int(status.item()) == sm.STATUS_NAN and float(wts[pl.K_STAR]) == 0.0 and bool(torch.isnan(cand[pl.K_STAR])) and bool(torch.isfinite(a_new).all())
        assert abs(float(wts.sum()) - 1.0) < 1e-12
        big = ops.PackedPlanExt(H, U, beta=op["beta"], sigma_rows=op["rows"], n_elite=K, alpha=0.2, sigma_min=0.05)
        a_new, s_new, cand, elite, stats, status = ops.cem_update(mp, big, J, a, xi=xi)
        el = elite.cpu().tolist()
        assert int(status.item()) == sm.STATUS_NAN and sorted(el[:K - 1]) == [k for k in range(K) if k != pl.K_STAR] and el[K - 1] == -1
        assert bool(torch.isfinite(a_new).all()) and bool(torch.isfinite(s_new).all())


# ---- 7. the update kernels at the widths and counts they had not seen ----------------------------------------------------------------------------
UPD_H, UPD_P = 2, 2


def kernel_draws(U, K, nz):
    """[H, K, U]: the kernels' own white normals of (seed, call) for a plan of width U -- the inputs of a sigma = 1, a = 0 launch without
    squashing on the layout with that many inputs (the update itself runs on synthetic costs)."""
    from mc_pilco_amd import ops

    layout = {1: "cart", 8: "limits"}[U]
    c, m, pm = pair(layout, 37, 0)
    pc, cin = packed_costs(pl.cost_specs(layout)["effort"], c["S"], U)
    raw = ops.PackedMPPI(K, 1, UPD_H, U, 1.0, 1.0, squash=False)
    z = lambda *s: torch.zeros(*s, dtype=DT, device=dev())  # noqa: E731
    return ops.mppi_rollout(pm, raw, pc, z(c["S"]), z(UPD_H, U), cost_inputs=cin, noise=nz, want_inputs=True)[2].reshape(UPD_H, K, U).contiguous()


def synthetic_costs(K, seed):
    """J [K, 2] of mixed sign; two candidates (3 and K - 1, where there are that many) with both particles at one negative value each, the
    two values neighbours in the last bit: S_k is that value exactly (the mean of two equals, a zero spread)."""
    gen = np.random.default_rng(seed)
    J = gen.standard_normal((K, UPD_P))
    lo = -1.25
    hi = np.nextafter(lo, 0.0)
    if K >= 2:
        J[K - 1], J[min(3, K - 2)] = lo, hi
    return J.reshape(-1), (lo, hi)


@pytest.mark.parametrize("K", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("U", [1, 8])
def test_the_updates_at_the_widths_and_counts_around_a_block(U, K):
    from mc_pilco_amd import ops

    H, P, lam, kappa, beta = UPD_H, UPD_P, 0.8, 0.5, 0.5
    nz = ops.NoiseSpec(seed=17, call=5)
    white = kernel_draws(U, K, nz)
    assert not bool(white[:, 0].any()) and (K == 1 or float(white[:, 1:].abs().min()) > 0)
    Jh, (lo, hi) = synthetic_costs(K, 100 * U + K)
    J = G(Jh)
    gen = np.random.default_rng(K + U)
    a = G(2 * gen.random((H, U)) - 1)
    sigma = pl.sigma_of(U) if U > 1 else np.array([0.3])
    what = "U %d K %d" % (U, K)
    # the MPPI update, Philox == the buffer, two runs alike
    mp = ops.PackedMPPI(K, P, H, U, sigma, lam, kappa)
    got = ops.mppi_update(mp, J, a, noise=nz)
    assert int(got[4].item()) == 0
    for other in (ops.mppi_update(mp, J, a, noise=nz), ops.mppi_update(mp, J, a, xi=white)):
        assert all(torch.equal(p, q) for p, q in zip(other[:4], got[:4]))
    f64 = check_update(what, got[:4], J, a, sigma, white, K, P, lam, kappa)
    if K == 1:
        assert float(got[2][0]) == 1.0 and torch.equal(got[0], a)
    else:
        assert float(got[1][K - 1]) == lo and float(got[1][min(3, K - 2)]) == hi
    # ... under the extension: a std per row, coloured
    s = 0.2 + 0.5 * gen.random((H, U))
    s[:, U - 1] = 0.01  # (so small that the floor below is active on the last input whatever the elites' spread)
    ext = ops.PackedPlanExt(H, U, beta=beta, sigma_rows=s)
    by_philox, by_buffer = ops.mppi_update_ext(mp, ext, J, a, noise=nz), ops.mppi_update_ext(mp, ext, J, a, xi=white)
    assert int(by_philox[4].item()) == 0 and all(torch.equal(p, q) for p, q in zip(by_philox[:4], by_buffer[:4]))
    args = (Jh, n_(a), s, n_(white), K, P, lam, kappa, beta)
    t64, tld = ct.update_ext(*args), ct.update_ext(*args, dt=np.longdouble)
    d = mt.d_ref(t64, tld)
    errs = [float(np.abs(n_(g) - t).max() / np.abs(t).max()) for g, t in zip(by_philox[:3], t64)]
    print("%s ext: a_new / cand_cost / weights: d_ref %.2e %.2e %.2e, kernel vs float64 truth %.2e %.2e %.2e" % ((what,) + tuple(d) + tuple(errs)))
    for e, dr in zip(errs, d):
        assert e <= bound(dr)
    # the CEM update: mixed signs, the two neighbours, a floor per input active on the last one alone
    E = max(1, K // 2)
    smin = np.zeros(U)
    smin[U - 1] = 0.3
    cem = ops.PackedPlanExt(H, U, beta=beta, sigma_rows=s, n_elite=E, alpha=0.3, sigma_min=smin)
    got = ops.cem_update(mp, cem, J, a, noise=nz)
    assert int(got[5].item()) == 0
    for other in (ops.cem_update(mp, cem, J, a, noise=nz), ops.cem_update(mp, cem, J, a, xi=white)):
        assert all(torch.equal(p, q) for p, q in zip(other[:5], got[:5]))
    f64 = check_cem(what, got, J, a, s, white, K, P, E, 0.3, smin, beta, kappa)
    assert bool((got[1][:, U - 1] == 0.3).all()) and bool((f64[1][:, U - 1] == 0.3).all())
    if U > 1:
        assert bool((got[1][:, :U - 1] > 0).all()) and float(np.abs(n_(got[1][:, :U - 1]) - 0.3).min()) > 0
    el = got[3].cpu().tolist()
    if K >= 4:  # the neighbours in the last bit: both elites, the lower first (cem_key's complement branch orders the negative costs)
        assert K - 1 in el and 3 in el and el.index(K - 1) + 1 == el.index(3)
    if K >= 255:  # costs of both signs among the elites
        Sk = n_(got[2])[el]
        assert bool((Sk < 0).any()) and bool((Sk > 0).any())


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------------
def test_plan_on_mixed5_equals_the_launches_chained_by_hand():
    from mc_pilco_amd import ops
    from mc_pilco_amd.policy_learning import Policy, mppi

    case = pl.BY_ID["plan-sampled-mixed5-2-37-3-7-3"]
    cfg, op = lay.LAYOUTS["mixed5"], pl.operands(case)
    c, m, pm = pair(case.layout, case.N, case.deg)
    K, P, H, U = case.K, case.P, case.H, cfg["U"]
    spec = pl.cost_specs("mixed5")["wide"]
    x0, a, eps = G(op["x0"]), G(op["a"]), G(op["eps"])
    noise = ops.NoiseSpec(eps=eps, seed=21, call=40)
    sigma = [0.4, 0.3, 0.2]
    par = dict(K=K, P=P, iterations=3, sigma=sigma, kappa=0.5, u_max=op["u_max"], particle_pred=True, noise=noise, method="cem", n_elite=3, alpha=0.2,
               sigma_min=0.05, beta=0.5, u_prev=op["u_prev"])
    got, info = mppi.plan(pm, x0, a, cost_object(spec), **par)
    again, info2 = mppi.plan(pm, x0, a, cost_object(spec), **par)
    sg, sg2 = info.pop("sigma"), info2.pop("sigma")
    assert torch.equal(got, again) and torch.equal(sg, sg2) and info == info2 and info["status"] == 0 and info["iterations"] == 3
    pc, cin = packed_costs(spec, c["S"], U)
    mp = ops.PackedMPPI(K, P, H, U, sigma, 1.0, 0.5, op["u_max"], True)
    ext = ops.PackedPlanExt(H, U, beta=0.5, n_elite=3, alpha=0.2, sigma_min=0.05)
    cur, s, nominal, elites = a, G(np.tile(np.array(sigma), (H, 1))), [], []
    for i in range(3):
        nz = ops.NoiseSpec(eps=eps, seed=21, call=40 + i)
        J = ops.plan_rollout(pm, mp, ext, pc, x0, cur, sigma_rows=s, u_prev=G(op["u_prev"]), cost_inputs=cin, noise=nz, particle_pred=True)[0]
        cur, s, cand, elite, stats, _ = ops.cem_update(mp, ext, J, cur, sigma_rows=s, noise=nz)
        nominal.append(float(cand[0])), elites.append(elite.cpu().tolist())
    assert torch.equal(got, cur) and torch.equal(sg, s) and info["nominal_cost"] == nominal and info["elite"] == elites
    assert not torch.equal(got, a) and float((sg - s.new_tensor(sigma)).abs().max()) > 1e-3
    # the MPPI update under the same extension, chained the same way
    got, info = mppi.plan(pm, x0, a, cost_object(spec), **dict(par, method="mppi", lam=0.1))
    mp = ops.PackedMPPI(K, P, H, U, sigma, 0.1, 0.5, op["u_max"], True)
    cur = a
    for i in range(3):
        nz = ops.NoiseSpec(eps=eps, seed=21, call=40 + i)
        J = ops.plan_rollout(pm, mp, ext, pc, x0, cur, u_prev=G(op["u_prev"]), cost_inputs=cin, noise=nz, particle_pred=True)[0]
        cur = ops.mppi_update_ext(mp, ext, J, cur, noise=nz)[0]
    assert torch.equal(got, cur) and info["status"] == 0 and info["iterations"] == 3 and not torch.equal(got, a)
    # the controller on that layout returns the first row of the plan it made
    um = [float(v) for v in op["u_max"]]
    kw = dict(K=19, P=1, sigma=0.4, lam=0.05)
    ctrl = Policy.MPPI_controller(c["S"], U, pm, cost_object(spec), horizon=H, iterations=2, noise=ops.NoiseSpec(seed=3, call=100), flg_squash=True, u_max=um,
                                  device=dev(), **kw)
    first = ctrl.forward_np(op["x0"], 0.0)
    plan_a, info = mppi.plan(pm, x0, torch.zeros(H, U, dtype=DT, device=dev()), cost_object(spec), iterations=2, u_max=um, flg_squash=True,
                             noise=ops.NoiseSpec(seed=3, call=100), t0=0, **kw)
    umt = torch.as_tensor(um, dtype=DT)
    assert first.shape == (1, U) and np.array_equal(first, (umt * torch.tanh(plan_a[0].cpu() / umt)).numpy().reshape(1, -1)) and np.abs(first).max() > 0
    assert torch.equal(ctrl.a, mppi.shift_warm_start(plan_a)) and ctrl.info["status"] == 0
