"""CPU: the table of tests/plan_models.py and the truth tests/test_gpu_plan_layouts.py compares the planner's rollout entries against.

  - the table covers what it says it covers (every layout under both entries sampled, the mean forms, the degrees, the tile shapes, the
    horizons, the options), and mppi_truth.cost_specs is generic in S and U (S = 2, S = 3);
  - the mirror of the LDS arithmetic gives the long horizons of the table, the rung on either side of them, the staging of the mean form,
    and agrees with the two refusals tests/test_plan_refusals_cpu.py::test_the_std_rows_count_in_the_lds_fit pins in the library;
  - on the truth alone, over the whole table: finite states and costs, no saturated point cost, K distinct candidate costs, every sampled
    variance status_models.MARGIN of k_zz away from zero (the long rows: finite states of the mean rollout);
  - the truth is sensitive to what the layouts pin: two entries of ``vel`` exchanged, the angle role of a component dropped (where the
    layout has neither: the unintegrated component carried over) move the costs by more than 1e-6 relative;
  - the status constructions give the word they are built for, with the margins the GPU test relies on."""
import dataclasses

import numpy as np
import pytest
import torch

import layout_models as lay
import mppi_truth as mt
import plan_models as pl
import status_models as sm

SAT = 1e-6  # a point cost's 1 - exp(-d) stays this far below 1
MOVED = 1e-6  # what a wrong variant moves the costs by, relative, at the least


def cases(which):
    return pytest.mark.parametrize("case", which, ids=pl.case_id)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_says():
    C = pl.CASES
    for name in lay.LAYOUTS:
        for entry in ("mppi", "plan"):
            assert any(c.layout == name and c.entry == entry and c.mode == "sampled" for c in C), (name, entry)
    for name in ("mixed5", "d16_angles", "limits"):
        assert any(c.layout == name and c.mode == "mean" and c.H <= pl.H_SHORT for c in C), name
    assert {c.deg for c in pl.SHORT} == {0, 1, 2} and all(c.N == 37 for c in C)
    assert any(c.layout == "limits" and c.mode == "sampled" and c.deg == 2 for c in C)
    sampled = {(c.K, c.P) for c in C if c.mode == "sampled"}
    assert {(7, 3), (3, 16), (2, 17), (33, 1), (1, 5)} <= sampled
    assert {c.H for c in pl.SHORT} == {2, 3, 6}
    assert any(c.entry == "plan" and c.H == 3 and c.opt.get("u_prev") for c in C)
    assert sum(1 for c in C if c.opt.get("squash") is False) == 1
    plan = [c for c in C if c.entry == "plan"]
    assert {c.opt["beta"] for c in plan} == {0.0, 0.5} and any(c.opt.get("rows") for c in plan)
    assert any(c.opt.get("t0", 0) > 0 and pl.cost_specs(c.layout)[c.opt["cost"]]["kind"] == "traj" for c in plan)
    assert all(c.opt.get("beta", 0.0) != 0.0 or c.opt.get("rows") or c.opt.get("u_prev") for c in plan)  # (a non-default extension)
    assert {c.opt["cost"] for c in pl.SHORT} == {"target_add", "traj_plain", "quad_joint", "wide", "traj_rate"}
    for entry in ("mppi", "plan"):
        long = [c for c in pl.LONG_CASES if c.entry == entry]
        assert sorted((c.mode, c.H) for c in long) == [("mean", pl.LONG[entry][1]), ("sampled", pl.LONG[entry][0]), ("sampled", pl.LONG[entry][1])]
        assert all(c.layout == "limits" and c.deg == 0 for c in long)
    for name, cfg in lay.LAYOUTS.items():  # sigma and u_max distinct per input, one sigma 0
        s, um = pl.sigma_of(cfg["U"]), pl.u_max_of(cfg["U"])
        assert len(set(s)) == cfg["U"] and len(set(um)) == cfg["U"] and bool((um > 0).all())
        assert (cfg["U"] == 1 and s[0] > 0) or (list(s).count(0.0) == 1 and s[pl.zero_input(cfg["U"])] == 0.0)
    for c in pl.STATUS_BASE:  # the NaN's candidate lies inside the first tile, its row moves a state that the cost reads
        assert 0 < pl.K_STAR * c.P and (pl.K_STAR + 1) * c.P < 16 and pl.T_STAR + 1 < c.H and pl.sigma_of(lay.LAYOUTS[c.layout]["U"])[0] > 0


@pytest.mark.parametrize("layout", list(lay.LAYOUTS))
def test_the_cost_descriptors_are_generic_in_S_and_U(layout):
    """S = 2 (all_angle) and S = 3 (g1_plain) among them: every index inside the state / the inputs, one lengthscale per index, and the
    truth's formula evaluates on a record of the layout's shape."""
    cfg = lay.LAYOUTS[layout]
    S, U = cfg["S"], cfg["U"]
    gen = np.random.default_rng(1)
    x, u = gen.standard_normal((4, 3, S)), gen.standard_normal((4, 3, U))
    specs = pl.cost_specs(layout)
    assert set(specs) == {"target_add", "traj_plain", "quad_joint", "effort", "wide", "traj_rate"}
    for name, sp in specs.items():
        assert all(0 <= i < S for i in sp["idx"]) and len(set(sp["idx"])) == len(sp["idx"]) == len(sp["ls"]) >= 1, name
        if sp.get("u_idx") is not None:
            assert all(0 <= k < U for k in sp["u_idx"])
        c = pl.point_costs(sp, x, u, 1, u[0, 0])
        assert c.shape == (4, 3) and np.isfinite(c).all(), name
    wide = specs["wide"]
    assert set(pl.unintegrated(cfg)) | {S - 1} <= set(wide["idx"]) and wide["u_idx"] == [U - 1] and specs["traj_rate"]["u_idx"] == [U - 1]
    assert pl.unintegrated(lay.LAYOUTS["g1_plain"]) == [0] and pl.unintegrated(lay.LAYOUTS["d16_angles"]) == [6]


def test_u_prev_enters_row_zero_alone():
    sp = pl.cost_specs("mixed5")["traj_rate"]
    gen = np.random.default_rng(2)
    x, u, up = gen.standard_normal((3, 2, 5)), gen.standard_normal((3, 2, 3)), gen.standard_normal(3)
    with_, without = pl.point_costs(sp, x, u, 2, up), pl.point_costs(sp, x, u, 2)
    assert np.array_equal(with_[1:], without[1:]) and np.abs(with_[0] - without[0]).min() > 0
    q = (u[0, :, 2] - up[2]) / sp["u_rate"][0]
    assert np.allclose(with_[0] - without[0], q * q, rtol=0, atol=1e-14)


# ---- the LDS arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_the_long_horizons_are_the_rung_change():
    for entry, ext in (("mppi", False), ("plan", True)):
        fit, beyond = pl.LONG[entry]
        assert pl.largest_h("limits", 37, 16, True, ext) == fit and beyond == fit + 1
        assert pl.rung("limits", 37, fit, True, ext) == (16, False) and pl.rung("limits", 37, beyond, True, ext) == (4, False)
        assert pl.largest_h("limits", 37, 4, True, ext) > beyond  # (and not refused)
        assert pl.rung("limits", 37, beyond, False, ext) == (1, False)  # the mean form there: unstaged ...
    for c in pl.SHORT:  # ... and staged on every short row; the short sampled rows all run 16 trajectories per workgroup
        assert pl.rung(c.layout, c.N, c.H, c.mode == "sampled", pl.is_ext(c)) == ((16, False) if c.mode == "sampled" else (1, True)), pl.case_id(c)
    assert 16 * (16 + 8 + 1) == 400 <= 512  # the three thread sets at the limits


def test_the_mirror_against_the_refusals_the_library_pins():
    """tests/test_plan_refusals_cpu.py's small model (S 4, U 1, G 2, D 6, Npad 32): H U = 10241 doubles of nominal fit beside it, with the
    std's rows nothing does; 20480 rows of nominal alone do not fit either.  The library's answers to the same calls stand beside."""
    from test_plan_refusals_cpu import S_PTR, call, ext, mppi

    def fits(H, e):
        return [pl.open_layout(PT, nv, 4, 6, 2, 32, pl.mppi_extra(PT, H, 1, e))[0] <= pl.LDS_DOUBLES for PT, nv in ((16, True), (4, True), (1, False))]

    assert fits(10241, False) == [True, True, True] and fits(10241, True) == [False, False, False] and fits(20480, False) == [False, False, False]
    for pp in (1, 0):
        assert call("plan_rollout", mppi=mppi(H=10241), ext=ext(beta=0.0, sigma_rows=S_PTR), particle_pred=pp) == -2
        assert call("plan_rollout", mppi=mppi(H=20480), particle_pred=pp) == -2


# ---- the truth over the table ---------------------------------------------------------------------------------------------------------------
@cases(pl.CASES)
def test_conditions_of_the_gpu_cases(case):
    r, op = pl.case_truth(case), pl.operands(case)
    assert np.isfinite(r["x"]).all() and np.isfinite(r["u"]).all()
    if case.H > pl.H_SHORT:
        assert r["x"].shape[0] == case.H and float(np.abs(r["x"]).max()) < 1e3
        return
    assert np.isfinite(r["J"]).all() and float(np.abs(r["x"]).max()) < 50.0
    spec = pl.cost_specs(case.layout)[case.opt["cost"]]
    d = pl.exponents(spec, r["x"], r["u"], op["t0"], op["u_prev"])
    if d is not None:
        assert float(np.exp(-d).min()) >= SAT, float(d.max())
    S = np.sort(r["S"])
    assert S.size == case.K and (case.K == 1 or float(np.diff(S).min()) > 1e-9 * float(np.abs(S).max()))
    if case.mode == "sampled":
        assert float((r["var"] / r["kzz"]).min()) >= sm.MARGIN
    for s in pl.unintegrated(lay.LAYOUTS[case.layout]):
        assert float(np.abs(r["x"][1:, :, s]).max()) == 0.0 and float(np.abs(r["x"][0, :, s]).min()) > 0.0
    z = pl.zero_input(lay.LAYOUTS[case.layout]["U"])
    if z is not None:  # the input without a perturbation is the nominal's for every candidate
        assert float(np.abs(r["u"][:, :, z] - r["u"][:, :1, z]).max()) == 0.0
    if case.K > 1:
        assert float(np.abs(r["u"] - r["u"][:, :1]).max()) > 1e-3


def test_the_variant_step_without_a_defect_is_the_oracles():
    for case in (pl.BY_ID["mppi-sampled-mixed5-1-37-6-7-3"], pl.BY_ID["plan-sampled-g1_plain-1-37-3-3-16"]):
        op = pl.operands(case)
        _, m, _ = lay.oracle_pair(case.layout, case.N, case.deg)
        x = pl.rollout(case, op, m, pl.candidate_inputs(case, op), step=pl.variant_step())[0]
        assert float(np.abs(x - pl.case_truth(case)["x"]).max()) < 1e-13


def variants(case):
    """(name, model, step) of every wrong variant the layout admits."""
    cfg = lay.LAYOUTS[case.layout]
    _, m, _ = lay.oracle_pair(case.layout, case.N, case.deg)
    out = []
    if cfg["G"] >= 2:
        vel = list(cfg["vel"])
        vel[0], vel[1] = vel[1], vel[0]
        out.append(("vel exchanged", dataclasses.replace(m, vel=vel), pl.variant_step()))  # (the written-out step: the delta-state oracle does not read vel)
    if cfg["angle"]:
        nna, na, i = len(cfg["not_angle"]), len(cfg["angle"]), len(cfg["angle"]) - 1
        out.append(("angle role dropped", m, pl.variant_step(zero_cols=(nna + i, nna + na + i))))
    if not out:
        out.append(("unintegrated component carried", m, pl.variant_step(carry=tuple(pl.unintegrated(cfg)))))
    return out


@cases(pl.SHORT)
def test_the_truth_is_sensitive_to_what_the_layout_pins(case):
    r, op = pl.case_truth(case), pl.operands(case)
    spec = pl.cost_specs(case.layout)[case.opt["cost"]]
    u = pl.candidate_inputs(case, op)
    torch.set_num_threads(1)
    for name, m, step in variants(case):
        x, ut = pl.rollout(case, op, m, u, step=step)
        J = pl.traj_costs(spec, x, ut, None, op["t0"], op["u_prev"])
        moved = float(np.abs(J - r["J"]).max() / np.abs(r["J"]).max())
        assert moved > MOVED, (name, moved)


# ---- the status constructions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("con", pl.CONS, ids=lambda c: c.id)
@cases(pl.STATUS_BASE)
def test_the_status_constructions(case, con):
    cfg, so, tr = lay.LAYOUTS[case.layout], pl.status_operands(case, con), pl.status_truth(case, con)
    g, M = so["gstar"], case.K * case.P
    assert tr["word"] == pl.expected_word(con) and not tr["word"] & ~(sm.STATUS_NAN | sm.STATUS_NONPOS_VAR)
    others = [i for i in range(cfg["G"]) if i != g]
    fin = np.isfinite(tr["var"])
    rel = np.where(fin, tr["var"], 1.0) / np.where(fin, tr["kzz"], 1.0)
    if con.kind == "A":
        assert bool((tr["var"][:, :, g] == 0.0).all()) and bool((rel[:, :, others] > sm.MARGIN).all())
        assert np.isfinite(tr["x"]).all() and np.isfinite(tr["u"]).all() and np.isfinite(tr["J"]).all()
        assert float(np.abs(tr["x"] - pl.case_truth(case)["x"]).max()) > 1e-6  # (delta = mu for g*: not the clean run)
    if con.kind == "B":
        r = pl.ratios_step0(case, pl.operands(case), lay.oracle_pair(case.layout, case.N, case.deg)[1], g)
        assert so["factor"] > 1.0 and float((so["factor"] * r - 1.0).min()) >= 100 * sm.MARGIN  # negative for every candidate, margins to spare
        assert bool((rel[0, :, g] <= -100 * sm.MARGIN).all()) and bool((rel[0][:, others] > sm.MARGIN).all())
        if con.mean:
            assert np.isfinite(tr["x"]).all() and np.isfinite(tr["J"]).all()
        else:
            assert np.isnan(tr["x"][1:, :, cfg["vel"][g]]).all() and np.isnan(tr["J"]).all() and np.isfinite(tr["u"]).all()
    if con.kind == "X":
        clean = pl.case_truth(case)
        bad = list(range(pl.K_STAR * case.P, (pl.K_STAR + 1) * case.P))
        keep = [i for i in range(M) if i not in bad]
        assert np.isnan(tr["J"][bad]).all() and np.array_equal(tr["J"][keep], clean["J"][keep]) and np.array_equal(tr["x"][:, keep], clean["x"][:, keep])
        assert np.isnan(tr["S"][pl.K_STAR]) and np.isfinite(np.delete(tr["S"], pl.K_STAR)).all()
        with np.errstate(invalid="ignore"):
            assert not bool((tr["var"] <= 0.0).any())
    if con.kind == "C":
        assert np.isnan(tr["J"]).all() and np.isnan(tr["var"][0]).all()
        with np.errstate(invalid="ignore"):
            assert not bool((tr["var"] <= 0.0).any())


def test_oracle_states_returns_what_it_did_for_the_existing_callers():
    """``fam`` None is pd_models.family(shape), and the layout's family handed over explicitly gives the same bits."""
    import pd_models

    c, m, _ = pd_models.build_pair("arm2", 37, 0, 37)
    gen = np.random.default_rng(3)
    x0, u, eps = 0.3 * gen.standard_normal(4), gen.standard_normal((4, 3, 2)), gen.standard_normal((3, 2, 2))
    a, b = mt.oracle_states("arm2", m, x0, u, 2, eps, True), mt.oracle_states("arm2", m, x0, u, 2, eps, True, fam="speed")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _, ml, _ = lay.oracle_pair("mixed5", 37, 0)
    x0, u, eps = 0.3 * gen.standard_normal(5), gen.standard_normal((3, 2, 3)), gen.standard_normal((2, 2, 3))
    a, b = mt.oracle_states("mixed5", ml, x0, u, 2, eps, True), mt.oracle_states("mixed5", ml, x0, u, 2, eps, True, fam=lay.family("mixed5"))
    assert np.array_equal(a[0], b[0])
