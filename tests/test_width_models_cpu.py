"""CPU side of the width-class tests: the oracle's generalised step (``mixed_next_state``: not_vel = -1 beside real positions, var_scale) is tied to
what it restates -- the speed-integration and delta-state steps that the reference's fixtures pin -- and the case table of tests/width_models.py is
shown to be SENSITIVE to the three defects it is there to catch, on the oracle alone (nothing is provoked on a device):

  a wrong row-tile count   the Jacobian columns of the GP-input features 16.. dropped (d delta / dz[16:] = 0)
  an accumulator bound 8   the policy-gradient entries of the features 8.. dropped
  a basis loop to 256      the basis functions 256.. dropped from the policy

Each must move a compared quantity of the listed cases by far more than the bound of tests/test_gpu_width_classes.py."""
import numpy as np
import pytest
import torch

import width_models as wm
from helpers import T, oracle_model
from open_grad_models import build_pair, oracle_step
from oracle import mcpilco_oracle as orc


def test_mixed_step_is_the_speed_step(golden):
    fx = golden("step_se")
    m = oracle_model(fx, "se")
    x, u, eps = T(fx["x"]), T(fx["u"]), T(fx["eps"])
    for sample in (True, False):
        a = orc.mixed_next_state(m, x, u, eps, sample)
        b = orc.next_state(m, x, u, eps, sample)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert np.max(np.abs(orc.mixed_next_state(m, x, u, eps)[0].numpy() - fx["next"])) < 1e-12  # (the reference's own step)


def test_mixed_step_is_the_delta_step():
    c, m, _ = build_pair("delta", 37, 1, 5)
    sm = orc.SpeedModel(m.hyp, m.cache, 0.05, c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    g = torch.Generator().manual_seed(1)
    x, u, eps = torch.randn(7, 4, dtype=torch.float64, generator=g), torch.randn(7, 1, dtype=torch.float64, generator=g), torch.randn(7, 4, dtype=torch.float64, generator=g)
    for sample in (True, False):
        a = orc.mixed_next_state(sm, x, u, eps, sample)
        b = orc.delta_next_state(m, x, u, eps, sample)
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert float((a[0] - b[0]).abs().max()) < 1e-14  # (x + (mu + s eps) against (x + mu) + s eps: one rounding apart)


def test_mixed_step_var_scale_and_missing_positions():
    """var_scale has no fixture of the reference's: it is tied by the identity sqrt(s var) eps = sqrt(var) (sqrt(s) eps) to ``next_state``, which the
    step_se fixture pins to the reference, and to the restatement the open-loop tests use.  (The reference class itself is not imported: the tests
    depend on nothing outside the repository.)"""
    c, m, _ = build_pair("speed", 37, 0, 3)
    g = torch.Generator().manual_seed(2)
    x, u, eps = torch.randn(7, 4, dtype=torch.float64, generator=g), torch.randn(7, 1, dtype=torch.float64, generator=g), torch.randn(7, 2, dtype=torch.float64, generator=g)
    vs = [0.49, 2.25]
    nx, mu, var = orc.mixed_next_state(m, x, u, eps, True, vs)
    ref, rvar = oracle_step("speed", m, x, u, eps, True, vs)  # (the restatement the open-loop tests pin)
    assert torch.equal(nx, ref) and torch.equal(var, rvar)
    # sqrt(s var) eps = sqrt(var) (sqrt(s) eps): the unscaled step on scaled noise
    alt, _, v1 = orc.next_state(m, x, u, eps * torch.sqrt(T(vs)), True)
    assert float((nx - alt).abs().max()) < 1e-14 and float((var - v1 * T(vs)).abs().max()) < 1e-15
    # GP 1 without a position: its velocity as before, the other GP's states as before, its former position has no role and is zero
    mm = orc.SpeedModel(m.hyp, m.cache, m.Ts, m.angle, m.not_angle, m.vel, [m.not_vel[0], -1])
    full = orc.next_state(m, x, u, eps, True)[0]
    got = orc.mixed_next_state(mm, x, u, eps, True)[0]
    keep = [m.vel[0], m.vel[1], m.not_vel[0]]
    assert torch.equal(got[:, keep], full[:, keep])
    assert float(got[:, m.not_vel[1]].abs().max()) == 0.0


def test_rollout_loops_take_the_step(golden):
    from helpers import oracle_policy

    fx = golden("rollout_se")
    m, pp = oracle_model(fx, "se"), oracle_policy(fx, "se")
    args = (T(fx["states"][0]), fx["states"].shape[0], float(fx["p_drop"]), T(fx["eps"]), T(fx["masks"]))
    a = orc.apply_policy(m, pp, *args)
    b = orc.apply_policy(m, pp, *args, step=orc.mixed_next_state)
    assert float((a[0] - T(fx["states"])).abs().max()) < 1e-9  # (the reference's own rollout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_case_table_widths():
    """Every case is a descriptor the library takes, and the table reaches what its coverage list says."""
    seen = set()
    for c in wm.CASES:
        k = wm.classes(c)
        assert c.S <= 16 and c.U <= 8 and 1 <= c.G <= 8 and c.D <= 32 and c.P <= 32 and c.B <= 1024 and len(c.N) == c.G and len(c.not_vel) == c.G
        assert not ((c.P > 16 or c.U > 4) and c.B > 512)
        assert all(0 <= i < c.S for i in c.angle + c.not_angle + c.vel + c.pol_angle + c.pol_non_angle + c.used)
        seen.add((k["sweep"], min(k["maxnt"], 512)))
        seen.add(("tile", k["tile"], k["row_tiles"]))
        assert 1 in wm.sweep_widths(c)
    for sw in ((8, 2), (16, 4), (24, 6), (32, 8)):
        assert (sw, 256) in seen and (sw, 512) in seen
    assert {("tile", 0, 1), ("tile", 1, 1), ("tile", 1, 2), ("tile", 2, 2), ("tile", None, 3)} <= seen
    assert {c.D for c in wm.CASES} >= {7, 8, 15, 16, 24, 25, 31, 32}
    assert {c.P for c in wm.CASES} >= {8, 9, 16, 17, 24, 25, 32} and {c.U for c in wm.CASES} >= {2, 3, 4, 5, 6, 7, 8}
    assert {c.G for c in wm.CASES} >= {1, 3, 5, 8}


def _grad_rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["ur5_angles_pms", "d25_s16_g8", "u7_g7_b257", "d31_traj_p32"])
def test_sensitive_to_a_dropped_row_tile(name):
    """Phase J with one row tile of [X^T; 1] where two are needed: the Jacobian columns of the features 16.. are missing.  (At D = 16 the second
    tile holds the ones row alone, which only the polynomial kernels read: the cases with D >= 17 are the ones that see it.)"""
    c = wm.BY_NAME[name]

    def step(m, x, u, e, sample):
        z = orc.gp_features(x, u, m.angle, m.not_angle)
        z = torch.cat([z[:, :16], z[:, 16:].detach()], 1)
        out = [orc.gp_estimate_from_alpha(h, q.X, z, q.alpha, q.Kinv) for h, q in zip(m.hyp, m.cache)]
        delta = torch.cat([o[0] for o in out], 1) + torch.sqrt(torch.stack([o[1] for o in out], 1)) * e
        nxt = torch.zeros_like(x)
        nxt[:, list(m.vel)] = x[:, list(m.vel)] + delta
        gs = [g for g, q in enumerate(m.not_vel) if q >= 0]
        nxt[:, [m.not_vel[g] for g in gs]] = x[:, [m.not_vel[g] for g in gs]] + m.Ts * x[:, [m.vel[g] for g in gs]] + m.Ts / 2 * delta[:, gs]
        return nxt, None, None

    M = 5
    ost, _, oc, og = wm.oracle(c, M)
    pp = wm.oracle_policy(c)
    prm = [pp.log_ls, pp.centers, pp.weight]
    for q in prm:
        q.requires_grad_(True)
    _, eps, masks, pos_noise = wm.noise(c, M)
    x0 = wm.noise(c, M)[0]
    om = wm.model(c)["om"]
    if c.pms is not None:
        st, _ = orc.apply_policy_pms(om, pp, x0, c.T, list(c.pms[0]), list(c.pms[1]), T(wm.policy(c)["std_pos"]), wm.FC, wm.P_DROP, eps, masks, pos_noise, step=step)
    else:
        st, _ = orc.apply_policy(om, pp, x0, c.T, wm.P_DROP, eps, masks, step=step)
    assert float(np.abs(st.detach().numpy() - ost).max()) < 1e-12  # (the trajectories do not change: only the gradients can tell)
    cost, _ = orc.expected_cost(wm.oracle_cost(c, st))
    cost.backward()
    # (already at T = 2, where the one Jacobian reaches the parameters through u_0 alone: the inputs are the LAST U features, beyond 16 in these cases)
    assert max(_grad_rel(q.grad.numpy(), g) for q, g in zip(prm, og)) > 1e-5


@pytest.mark.parametrize("name", ["d15_p10_g3", "d25_s16_g8", "speed_mixed_p9"])
def test_sensitive_to_an_accumulator_bound_of_8(name):
    """The <16,4> sweep with its per-thread feature accumulators cut at 8: dJ/dcenters[:, 8:] and dJ/dlog_ls[8:] are lost."""
    c = wm.BY_NAME[name]
    assert wm.classes(c)["sweep"] == (16, 4) and c.P > 8
    _, _, _, og = wm.oracle(c, 5)
    for g in (og[0], og[1]):
        cut = g.copy()
        cut[..., 8:] = 0.0
        assert _grad_rel(cut, g) > 1e-3


@pytest.mark.parametrize("name", ["narrow_b257", "narrow_b1024", "g1_plain_d16", "d15_p10_g3", "u4_b513", "p17_u2_b257", "u7_g7_b257"])
def test_sensitive_to_a_basis_loop_that_stops_at_256(name):
    c = wm.BY_NAME[name]
    assert c.B > 256
    _, oin, _, og = wm.oracle(c, 5)
    cut = og[2].copy()
    cut[:, 256:] = 0.0
    assert _grad_rel(cut, og[2]) > 1e-3
    pp = wm.oracle_policy(c)
    pp.centers, pp.weight = pp.centers[:256], pp.weight[:, :256]
    x0, _, masks, _ = wm.noise(c, 5)
    u0 = orc.policy_forward(pp, x0, 0, masks[0][:, :256], wm.P_DROP)
    assert float(np.abs(u0.numpy() - oin[0]).max()) > 1e-6
