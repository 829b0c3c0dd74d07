"""CPU: the layouts of tests/layout_models.py and the truth the GPU matrix (tests/test_gpu_layouts.py) compares against.

  - the "mixed" branch of open_grad_models.oracle_step is the speed step on arm2 and the delta step on arm2_delta, bit for bit;
  - the truth of a layout is sensitive to what the layout pins (a truth that did not change under the wrong variant would pin nothing);
  - the conditions the GPU cases rely on hold on the truth alone: finite states below 50, positive variances, cond(Quu) <= 1e4 for the
    pass, clamped and unclamped integral entries (and the clamp margin of tests/pid_models.py) for the PID cases;
  - the truth's autograd graph on the two layouts with overlapping pulls / unintegrated components agrees with central differences."""
import dataclasses

import numpy as np
import pytest
import torch

import layout_models as lay
import lqr_models as lm
import pd_models
import pid_models
import tvl_models as tm
from open_grad_models import oracle_step
from oracle import mcpilco_oracle as orc

DT = torch.float64


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_the_kernels_limits_and_tiles_ask_for():
    L = lay.LAYOUTS
    for name, c in L.items():
        assert len(c["vel"]) == len(c["not_vel"]) == c["G"] and c["pins"]
        assert len(set(c["angle"])) == len(c["angle"]) and len(set(c["not_angle"])) == len(c["not_angle"])  # what model_lists_ok accepts
        pos = [q for q in c["not_vel"] if q >= 0]
        assert len(set(c["vel"])) == c["G"] and len(set(pos)) == len(pos) and not set(c["vel"]) & set(pos)
    D = {n: len(c["not_angle"]) + 2 * len(c["angle"]) + c["U"] for n, c in L.items()}
    assert D == dict(cart=6, all_angle=5, g1_plain=4, mixed5=10, d15_plain=15, d16_angles=16, limits=32)
    assert {n: c["U"] * (c["S"] + 1) for n, c in L.items() if n in ("mixed5", "d15_plain", "d16_angles", "limits")} == dict(
        mixed5=18, d15_plain=55, d16_angles=24, limits=136)
    assert L["limits"]["G"] * D["limits"] == 256 and L["limits"]["U"] * L["limits"]["S"] + L["limits"]["U"] + L["limits"]["S"] == 152
    m5 = L["mixed5"]
    assert set(m5["angle"]) & set(m5["not_angle"]) == {0} and 2 not in m5["angle"] + m5["not_angle"] and m5["angle"] != sorted(m5["angle"])
    assert 2 in range(m5["U"]) and 2 in range(m5["S"] // 2, m5["S"] // 2 + m5["U"])  # position of input 2, velocity of input 0
    assert 0 not in L["g1_plain"]["vel"] + L["g1_plain"]["not_vel"] and 6 not in L["d16_angles"]["vel"] + L["d16_angles"]["not_vel"]
    assert [pd_models.family(n) for n in L] == ["mixed", "delta"] + ["mixed"] * 5 and pd_models.family("arm2") == "speed"


def test_every_layout_runs_every_form_sampled():
    forms = {(c.form, "meas" in c.opt) for c in lay.CASES if c.form in ("pd", "pid", "tvl")} | {(c.form, False) for c in lay.CASES}
    for name in lay.LAYOUTS:
        have = {(c.form, "meas" in c.opt and c.form in ("pd", "pid", "tvl")) for c in lay.CASES if c.layout == name and (c.mode == "sampled" or c.form == "pass")}
        assert have == forms, (name, forms - have)
    assert {c.M for c in lay.CASES} == {1, 5, 17, 33} and {c.T for c in lay.CASES} == {2, 3, 12} and {c.deg for c in lay.CASES} == {0, 1, 2}
    assert all(c.N == 37 for c in lay.CASES)


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True], ids=["mean", "sampled"])
@pytest.mark.parametrize("deg", [0, 2])
def test_the_mixed_step_is_the_speed_step_and_the_delta_step(deg, sample):
    gen = torch.Generator().manual_seed(4)
    x, u = 0.6 * (torch.rand(9, 4, dtype=DT, generator=gen) - 0.5), torch.rand(9, 2, dtype=DT, generator=gen) * 2 - 1
    c, m, _ = pd_models.build_pair("arm2", 37, deg, 37 + deg)
    eps = torch.randn(9, 2, dtype=DT, generator=gen)
    nx, _, var = orc.next_state(m, x, u, eps, sample)
    got = oracle_step("mixed", m, x, u, eps, sample)
    assert torch.equal(got[0], nx) and torch.equal(got[1], var)
    vs = [0.49, 2.25]
    want, got = oracle_step("speed", m, x, u, eps, sample, vs), oracle_step("mixed", m, x, u, eps, sample, vs)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and (not sample or not torch.equal(got[0], nx))
    c, md, _ = pd_models.build_pair("arm2_delta", 37, deg, 37 + deg)
    ms = orc.SpeedModel(md.hyp, md.cache, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    eps = torch.randn(9, 4, dtype=DT, generator=gen)
    nx, dmu, var = orc.delta_next_state(md, x, u, eps, sample)
    got = oracle_step("mixed", ms, x, u, eps, sample)
    assert torch.equal(got[0], nx) and torch.equal(got[1], var)
    vs = [0.49, 2.25, 1.0, 0.81]  # (oracle_step has no scaled delta step: the formula of delta_next_state on the scaled variances)
    got = oracle_step("mixed", ms, x, u, eps, sample, vs)
    dvar = var * torch.tensor(vs, dtype=DT)
    assert torch.equal(got[1], dvar) and torch.equal(got[0], x + dmu + torch.sqrt(dvar) * eps if sample else x + dmu)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------
def _pd(layout, m, T=6, M=5, seed=11, **kw):
    c = lay.LAYOUTS[layout]
    x0, kp, kd, target, eps, w, wu = pd_models.inputs_for(c, M, T, seed)
    return pd_models.pd_truth(layout, m, x0, kp, kd, target, eps, w, wu, True, **kw)


def _changed(a, b, least=1e-6):
    """States or a gradient moved by more than ``least`` relative."""
    d = max(rel(a[0], b[0]), rel(a[2], b[2]), rel(a[3], b[3]), rel(a[4], b[4]))
    assert d > least, d
    return d


def written_out(zero_col=None, carry=()):
    """orc.mixed_next_state assembled column by column, as a step for pd_truth; ``zero_col``: that GP input reads 0; ``carry``: components
    nothing integrates that keep their value instead of becoming 0 -- the deliberately wrong variants."""
    def step(shape, mm, x, u, eps, sample, var_scale=None):
        z = orc.gp_features(x, u, mm.angle, mm.not_angle)
        if zero_col is not None:
            z = torch.cat([z[:, :zero_col], torch.zeros_like(z[:, :1]), z[:, zero_col + 1:]], 1)
        out = [orc.gp_estimate_from_alpha(h, cc.X, z, cc.alpha, cc.Kinv) for h, cc in zip(mm.hyp, mm.cache)]
        dmu, dvar = torch.cat([o[0] for o in out], 1), torch.cat([o[1].reshape(-1, 1) for o in out], 1)
        delta = dmu + torch.sqrt(dvar) * eps if sample else dmu
        cols = [x[:, s] if s in carry else torch.zeros_like(x[:, 0]) for s in range(x.shape[1])]
        for g, (v, q) in enumerate(zip(mm.vel, mm.not_vel)):
            cols[v] = x[:, v] + delta[:, g]
            if q >= 0:
                cols[q] = x[:, q] + mm.Ts * x[:, v] + mm.Ts / 2 * delta[:, g]
        return torch.stack(cols, 1), dvar
    return step


def test_mixed5_is_sensitive_to_what_it_pins():
    c, m, _ = lay.oracle_pair("mixed5", 37, 1)
    torch.set_num_threads(1)
    base = _pd("mixed5", m)
    assert rel(_pd("mixed5", m, step=written_out())[0], base[0]) < 1e-13  # (the written-out step is the oracle's: a variant differs by its defect alone)
    # two entries of vel swapped: GP 1 (no position) and GP 2 (position 4) exchange their components
    _changed(_pd("mixed5", dataclasses.replace(m, vel=[3, 2, 1])), base)
    # component 0 dropped from not_angle: its plain feature reads 0 (what a kernel that found it as an angle ONLY would leave)
    _changed(_pd("mixed5", m, step=written_out(zero_col=list(c["not_angle"]).index(0))), base)
    # input 2 reads its position from component 4 instead of component 2 (which then is a velocity only)
    _changed(_pd("mixed5", m, pos=[0, 1, 4]), base)


def test_g1_plain_is_sensitive_to_the_zeroed_component():
    c, m, _ = lay.oracle_pair("g1_plain", 37, 1)
    torch.set_num_threads(1)
    base = _pd("g1_plain", m)
    assert float(base[0][1:, :, 0].abs().max()) == 0.0 and float(base[0][0, :, 0].abs().min()) > 0.0
    assert rel(_pd("g1_plain", m, step=written_out())[0], base[0]) < 1e-13
    _changed(_pd("g1_plain", m, step=written_out(carry=(0,))), base)  # component 0 carried over instead of zeroed


# ---- the conditions the GPU cases rely on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lay.CASES, ids=lay.case_id)
def test_conditions_of_the_gpu_cases(case):
    r = lay.case_truth(case)
    st = r["states"]
    assert bool(torch.isfinite(st).all()) and float(st.abs().max()) < 50.0
    assert r["vmin"] > 0.0
    if case.form == "pid":
        share, margin = pid_models.clamp_figures(r["truth"], r["ins"]["i_max"])
        assert 0.0 < share < 1.0 and margin >= pid_models.MARGIN, (share, margin)
        assert all(np.isfinite(v) for v in r["ins"]["i_max"])
    if case.form == "pass":
        from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

        c = lay.LAYOUTS[case.layout]
        x0, a, u, du, eps, target = r["ins"]
        states, A, B = r[False]
        cost = Quadratic_tracking_cost(target, torch.ones(c["S"], dtype=DT), input_lengthscales=[1.0] * c["U"])
        J, lx, lu, hxx, huu, s = cost.expansion(states, a, 1.0, True)
        n = lambda v: v.numpy()
        Bs = B * s[:case.T - 1].unsqueeze(2)
        for i in range(case.M):
            cond = lm.riccati_truth(n(A[:, i]), n(Bs[:, i]), n(lx[:, i]), n(lu[:, i]), n(hxx[:, i]), n(huu[:, i]), case.opt["reg"])[3]
            assert cond <= 1e4, (i, cond)
    if case.layout == "g1_plain" and case.form not in ("lin", "pass", "step"):
        assert float(st[1:, :, 0].abs().max()) == 0.0


# ---- the autograd graph of the truth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["mixed5", "d16_angles"])
def test_truth_gradients_against_central_differences(layout):
    """Step 1e-6, bound 1e-6 relative with floor 1e-2 (tests/test_tvl_cpu.py), on the first and the last entry of every parameter and of x0:
    the PD law (two pulls on one component on mixed5) and the dense law."""
    c, m, _ = lay.oracle_pair(layout, 37, 2)
    T, M = 6, 3
    torch.set_num_threads(1)
    x0, kp, kd, target, eps, w, wu, gain, ff = tm.tvl_inputs(c, M, T, 9)
    L = lambda st, inp: float((w * st).sum() + (wu * inp).sum())

    def pd(x, p, d):
        t = pd_models.pd_truth(layout, m, x, p, d, target, eps, w, wu, True)
        return L(t[0], t[1]), [t[4], t[2], t[3]]

    def tvl(x, g, f):
        t = tm.tvl_truth(layout, m, x, g, f, target, eps, w, wu, True)
        return L(t.states, t.inputs), [t.g_x0, t.g_gain, t.g_ff]

    for f, args in ((pd, [x0, kp, kd]), (tvl, [x0, gain, ff])):
        _, grads = f(*args)
        for which, q in enumerate(args):
            for e in (0, q.numel() - 1):
                plus, minus = [a.clone() for a in args], [a.clone() for a in args]
                plus[which].reshape(-1)[e] += 1e-6
                minus[which].reshape(-1)[e] -= 1e-6
                fd, g = (f(*plus)[0] - f(*minus)[0]) / 2e-6, float(grads[which].reshape(-1)[e])
                assert abs(fd - g) < 1e-6 * max(abs(g), 1e-2), (f.__name__, which, e, fd, g)
