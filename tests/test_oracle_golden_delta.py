"""Delta-state models (Model_learning_RBF, Model_learning_RBF_angle_state, Model_learning_RBF_MPK_angle_state -- reference
model_learning/Model_learning.py:471-618): the reference's apply_policy + cost + backward (tests/golden/make_golden_delta.py)
against the delta integrator restated here on the oracle's per-GP posterior.  Pins the fixtures the GPU tests use."""
import numpy as np
import pytest
import torch

from helpers import T, hyper
from oracle import mcpilco_oracle as orc

DELTA_FIXTURES = ["rollout_delta", "rollout_delta_mpk", "rollout_delta_rbf"]


def relerr(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def delta_fixture_poly(fx, g):
    ws = [fx["poly_w%d_gp%d" % (k, g)] for k in (1, 2) if "poly_w%d_gp%d" % (k, g) in fx]
    return ws or None


def delta_features(x, u, angle, not_angle):
    """Model_learning.py:450-456 (z = [x, u]) and :564-579 (z = [x_notangle, sin x_angle, cos x_angle, u])."""
    if len(angle) == 0:
        return torch.cat([x, u], 1)
    return orc.gp_features(x, u, angle, not_angle)


def delta_rollout(fx, pp, x0, eps, masks, p):
    """MC_PILCO.apply_policy's T-loop with the delta integrator (Model_learning.py:471-493): x' = x + (mu + sqrt(var) eps)."""
    G = fx["eps"].shape[2]
    hyp = [hyper(fx["lengthscales"], float(fx["sigma_n"]), 1.0, delta_fixture_poly(fx, g)) for g in range(G)]
    X = [T(fx["Xtr%d" % g]) for g in range(G)]
    alpha = [T(fx["alpha%d" % g]) for g in range(G)]
    Kinv = [T(fx["Kinv%d" % g]) for g in range(G)]
    angle, not_angle = [int(i) for i in fx["angle"]], [int(i) for i in fx["not_angle"]]
    xs = [x0]
    us = [orc.policy_forward(pp, x0, 0, masks[0], p)]
    for t in range(1, fx["states"].shape[0]):
        z = delta_features(xs[-1], us[-1], angle, not_angle)
        mus, vrs = [], []
        for g in range(G):
            mu, var = orc.gp_estimate_from_alpha(hyp[g], X[g], z, alpha[g], Kinv[g])
            mus.append(mu)
            vrs.append(var.reshape(-1, 1))
        delta = torch.cat(mus, 1) + torch.sqrt(torch.cat(vrs, 1)) * eps[t - 1]
        xs.append(xs[-1] + delta)
        us.append(orc.policy_forward(pp, xs[-1], t, masks[t], p))
    return torch.stack(xs), torch.stack(us)


@pytest.mark.parametrize("name", DELTA_FIXTURES)
def test_delta_rollout_cost_gradient(golden, name):
    fx = golden(name)
    pp = orc.PolicyPar(torch.log(T(fx["pol_ls"])), T(fx["pol_centers"]), T(fx["pol_weight"]), 10.0, "angles", angle=[2], non_angle=[0, 1, 3])
    x0 = orc.sample_x0(T(fx["x0_mean"]), T(fx["x0_var"]), fx["eps0"].shape[0], T(fx["eps0"]))
    assert np.array_equal(x0.numpy(), fx["states"][0])  # bit-exact x0
    for q in (pp.log_ls, pp.centers, pp.weight):
        q.requires_grad_(True)
    p = float(fx["p_drop"])
    st, inp = delta_rollout(fx, pp, x0, T(fx["eps"]), T(fx["masks"]), p)
    cost, std = orc.expected_cost(orc.cart_pole_cost(st, T([np.pi, 0.0]), T([3.0, 1.0]), 2, 0))
    cost.backward()
    # SE models: 1e-12 / gradients rel 1e-10.  SE + Volterra: the oracle sums the polynomial Gram in its own order (the posterior mean
    # cancels against it), so the bounds of the project's other SE + polynomial rollout fixture apply (test_oracle_golden.py)
    poly = "poly_w1_gp0" in fx
    xt, ct, gt = (1e-9, 1e-11, 1e-8) if poly else (1e-12, 1e-12, 1e-10)
    assert np.max(np.abs(st.detach().numpy() - fx["states"])) < xt
    assert np.max(np.abs(inp.detach().numpy() - fx["inputs"])) < xt
    assert abs(float(cost.detach()) - float(fx["cost"])) < ct * abs(float(fx["cost"]))
    assert abs(float(std) - float(fx["std"])) < ct * max(abs(float(fx["std"])), 1e-3)
    assert relerr(pp.log_ls.grad.numpy(), fx["g_log_ls"]) < gt
    assert relerr(pp.centers.grad.numpy(), fx["g_centers"]) < gt
    assert relerr(pp.weight.grad.numpy(), fx["g_weight"]) < gt


@pytest.mark.parametrize("name", DELTA_FIXTURES)
def test_delta_fixture_shape(golden, name):
    """Every fixture is a full-state model: one GP per state component, the reference's noise widths."""
    fx = golden(name)
    Tn, M, S = fx["states"].shape
    assert fx["eps"].shape == (Tn - 1, M, S)
    assert fx["masks"].shape[:2] == (Tn, M)
    D = len(fx["not_angle"]) + 2 * len(fx["angle"]) + fx["inputs"].shape[2]
    for g in range(S):
        assert fx["Xtr%d" % g].shape[1] == D
