"""CPU: the truth of the trajectory-optimisation tests (tests/lqr_models.py) against statements that do not share its code -- the
Riccati recursion against the finite-horizon LQ problem stacked as ONE linear system, and the iLQR loop on the oracle's step lowering its
cost -- so that tests/test_gpu_lqr.py does not compare the kernel with a restatement of itself."""
import numpy as np
import torch

import lqr_models as lm
import pd_models


def _random_lq(seed, S=2, U=1, T=3):
    rs = np.random.RandomState(seed)
    A = np.eye(S) + 0.3 * rs.randn(T - 1, S, S)
    B = rs.randn(T - 1, S, U)
    lx, lu = rs.randn(T, S), rs.randn(T, U)
    hxx, huu = 0.5 + rs.rand(T, S), 0.5 + rs.rand(T, U)
    return A, B, lx, lu, hxx, huu


def test_the_recursion_solves_the_stacked_lq_problem():
    """S = 2, U = 1, T = 3, random time-varying linear system, reg = 0.  For every start row t0 the tail problem with dx_t0 given is one
    linear system: its first input is kff[t0] for dx_t0 = 0 and kff[t0] - gain[t0] e_i for dx_t0 = e_i (the law is da = kff - gain dx); and
    the whole open-loop solution from dx_0 = 0 is the closed loop of (gain, kff) rolled forward."""
    for seed in (0, 1, 2):
        A, B, lx, lu, hxx, huu = _random_lq(seed)
        gain, kff, dv, cond = lm.riccati_truth(A, B, lx, lu, hxx, huu, 0.0)
        T, S, U = 3, 2, 1
        for t0 in range(T):
            base = lm.lq_stacked(A, B, lx, lu, hxx, huu, t0, np.zeros(S))
            assert np.abs(base[0] - kff[t0]).max() < 1e-12 * max(1.0, np.abs(kff).max())
            for i in range(S):
                got = lm.lq_stacked(A, B, lx, lu, hxx, huu, t0, np.eye(S)[i])[0] - base[0]
                assert np.abs(got + gain[t0][:, i]).max() < 1e-12 * max(1.0, np.abs(gain).max())
        da, dx = lm.lq_stacked(A, B, lx, lu, hxx, huu, 0, np.zeros(S)), np.zeros(S)
        for t in range(T):
            a_t = kff[t] - gain[t] @ dx
            assert np.abs(a_t - da[t]).max() < 1e-12 * max(1.0, np.abs(da).max())
            if t < T - 1:
                dx = A[t] @ dx + B[t] @ a_t
        # the predicted change of the cost at the full step is the optimum's value: dv0 + dv1 / 2 = min of the quadratic model
        x = np.zeros((T, S))
        for t in range(T - 1):
            x[t + 1] = A[t] @ x[t] + B[t] @ da[t]
        val = (lx * x).sum() + 0.5 * (hxx * x * x).sum() + (lu * da).sum() + 0.5 * (huu * da * da).sum()
        assert abs(dv[0] + 0.5 * dv[1] - val) < 1e-12 * max(1.0, abs(val))
        assert dv[0] < 0 < dv[1] and cond >= 1.0


def test_the_long_double_recursion_agrees_and_measures_rounding():
    A, B, lx, lu, hxx, huu = _random_lq(5, S=4, U=2, T=12)
    f64, ld = lm.riccati_truth(A, B, lx, lu, hxx, huu, 1e-3), lm.riccati_truth_ld(A, B, lx, lu, hxx, huu, 1e-3)
    assert ld[0].dtype == np.longdouble
    d = lm.d_ref(f64, ld)
    assert all(0.0 <= v < 1e-11 for v in d)
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert max(d) > 0.0  # extended precision: the float64 recursion's rounding shows


def test_a_pivot_that_is_not_positive_is_refused():
    A, B, lx, lu, hxx, huu = _random_lq(3)
    huu[1] = -50.0
    for f in (lm.riccati_truth, lm.riccati_truth_ld):
        try:
            f(A, B, lx, lu, hxx, huu, 0.0)
            raise AssertionError("accepted")
        except np.linalg.LinAlgError:
            pass


def test_autograd_jacobians_of_the_oracle_step_against_differences():
    """A, B of lqr_models.autograd_AB at one row of arm2 (mean and sampled) against central differences of oracle_step."""
    c, m, _ = pd_models.build_pair("arm2", 37, 0, seed=37)
    x0, a, u, du, eps, target = lm.operands(c, 3, 2, 1)
    for sample in (False, True):
        st = lm.oracle_rollout("arm2", m, x0, u[:2], eps, sample)
        A, B = lm.autograd_AB("arm2", m, st, u, eps, sample, du)
        assert tuple(A.shape) == (2, 2, 4, 4) and tuple(B.shape) == (2, 2, 4, 2)
        h, t, p = 1e-6, 1, 1
        step = lambda x, v: lm.oracle_step(pd_models.family("arm2"), m, x, v, eps[t], sample)[0][p]
        for j in range(4):
            d = torch.zeros(2, 4, dtype=lm.DT)
            d[p, j] = h
            fd = (step(st[t] + d, u[t]) - step(st[t] - d, u[t])) / (2 * h)
            assert float((fd - A[t, p, :, j]).abs().max()) < 1e-7
        for k in range(2):
            d = torch.zeros(2, 2, dtype=lm.DT)
            d[p, k] = h
            fd = (step(st[t], u[t] + d) - step(st[t], u[t] - d)) / (2 * h) * du[t, p, k]
            assert float((fd - B[t, p, :, k]).abs().max()) < 1e-7


def test_ilqr_on_the_oracle_lowers_the_cost():
    """arm2, N = 37, degree 0, T = 12: the cost of the nominal never rises from pass to pass, and falls."""
    from mc_pilco_amd.policy_learning.ilqr import Quadratic_tracking_cost

    torch.set_num_threads(1)
    c, m, _ = pd_models.build_pair("arm2", 37, 0, seed=37)
    T = 12
    x0, _, _, target = pd_models.inputs_for(c, 1, T, 3)[:4]
    cost = Quadratic_tracking_cost(target[:T], torch.ones(4, dtype=lm.DT), input_lengthscales=[2.0, 2.0])
    out = lm.ilqr_truth("arm2", m, x0[0], torch.zeros(T, 2, dtype=lm.DT), cost, iterations=4)
    J = out["cost"]
    print("ilqr_truth cost per pass:", J, "alpha:", out["alpha"])
    assert len(J) >= 2 and all(b <= a for a, b in zip(J, J[1:])) and J[-1] < J[0]
    assert all(b < a for a, b, al in zip(J, J[1:], out["alpha"]) if al > 0)
