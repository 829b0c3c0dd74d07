"""The truth for the trajectory-optimisation entries (mcp_linearize, mcp_lqr_pass, policy_learning/ilqr.py): dense Jacobians of
tests/open_grad_models.oracle_step by torch autograd, the Riccati recursion of include/mcpilco_hip.h written out in numpy -- once in float64
and once in numpy.longdouble, whose difference measures a case's conditioning --, the finite-horizon LQ problem stacked as ONE linear system
(an independent statement of optimality: tests/test_lqr_truth_cpu.py pins the recursion to it), and the iLQR loop on oracle_step.  Models
and inputs are those of tests/pd_models.py.  CPU side only imports torch, numpy, helpers and the oracle."""
import numpy as np
import torch

from open_grad_models import oracle_step
from pd_models import family

DT = torch.float64
MODELS = [("arm2", 0, 37), ("arm2_delta", 2, 37), ("ur5", 1, 48)]  # (shape, degree, N) of pd_models
SIZES = [(12, 5), (3, 17), (2, 1)]  # (T, M)


def squash(a, u_max, on):
    if not on:
        return a
    um = torch.as_tensor(u_max, dtype=DT)
    return um * torch.tanh(a / um)


def operands(c, T, M, seed, u_max=1.0, squashed=True):
    """x0 [M,S] as pd_models.inputs_for draws it, pre-squash inputs a [T,M,U] in [-1, 1], the applied inputs u, du/da, eps [T-1,M,G] and a
    smooth target [T,S] within +-0.3."""
    gen = torch.Generator().manual_seed(7000 + seed)
    x0 = 0.6 * (torch.rand(M, c["S"], dtype=DT, generator=gen) - 0.5)
    a = torch.rand(T, M, c["U"], dtype=DT, generator=gen) * 2 - 1
    u = squash(a, u_max, squashed)
    du = (1.0 - torch.tanh(a / torch.as_tensor(u_max, dtype=DT)) ** 2) if squashed else torch.ones_like(a)
    eps = torch.randn(T - 1, M, c["G"], dtype=DT, generator=gen)
    ph = 6.28 * torch.rand(1, c["S"], dtype=DT, generator=gen)
    target = 0.3 * torch.sin(0.3 * torch.arange(T, dtype=DT).reshape(-1, 1) + ph)
    return x0, a, u, du, eps, target


def autograd_AB(shape, m, states, u, eps, sample, du=None):
    """A [T-1,M,S,S], B [T-1,M,S,U] = d oracle_step / d(x, u) at (states[t], u[t]) by torch.autograd.functional.jacobian, one call per row
    (the trajectories of a row are independent: the Jacobian of the sum over them is the stack of theirs); ``du`` [T,M,U] scales B's
    columns."""
    T1, M = states.shape[0] - 1, states.shape[1]
    A, B = [], []
    for t in range(T1):
        f = lambda x, v: oracle_step(family(shape), m, x, v, eps[t], sample)[0].sum(0)
        Jx, Ju = torch.autograd.functional.jacobian(f, (states[t], u[t]))  # [S, M, S], [S, M, U]
        A.append(Jx.permute(1, 0, 2))
        B.append(Ju.permute(1, 0, 2) if du is None else Ju.permute(1, 0, 2) * du[t].unsqueeze(1))
    return torch.stack(A), torch.stack(B)


def oracle_rollout(shape, m, x0, u, eps, sample):
    """states [T,M,S] of the oracle's step loop on the inputs u [T-1,M,U]."""
    xs = [x0]
    with torch.no_grad():
        for t in range(u.shape[0]):
            xs.append(oracle_step(family(shape), m, xs[-1], u[t], eps[t], sample)[0])
    return torch.stack(xs)


# ---- the recursion ----------------------------------------------------------------------------------------------------------------------
def _cholesky(Q, dt):
    n = Q.shape[0]
    L = np.zeros((n, n), dtype=dt)
    for j in range(n):
        p = Q[j, j] - sum((L[j, k] * L[j, k] for k in range(j)), dt(0))
        if not p > 0:
            raise np.linalg.LinAlgError("pivot %r" % (p,))
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (Q[i, j] - sum((L[i, k] * L[j, k] for k in range(j)), dt(0))) / L[j, j]
    return L


def _chol_solve(L, R, dt):
    n = L.shape[0]
    Y = np.zeros_like(R)
    for k in range(n):
        Y[k] = (R[k] - sum((L[k, j] * Y[j] for j in range(k)), np.zeros_like(R[0]))) / L[k, k]
    X = np.zeros_like(R)
    for k in range(n - 1, -1, -1):
        X[k] = (Y[k] - sum((L[j, k] * X[j] for j in range(k + 1, n)), np.zeros_like(R[0]))) / L[k, k]
    return X


def riccati_truth(A, B, lx, lu, hxx, huu, reg, dt=np.float64):
    """One trajectory: A [T-1,S,S], B [T-1,S,U] (B in the pre-squash variable), lx [T,S], lu [T,U], hxx [T,S], huu [T,U] ->
    (gain [T,U,S], kff [T,U], dv [2], the largest cond(Quu) met).  The recursion as include/mcpilco_hip.h states it, in ``dt``."""
    c = lambda v: np.asarray(v, dtype=dt)
    A, B, lx, lu, hxx, huu, reg = c(A), c(B), c(lx), c(lu), c(hxx), c(huu), dt(reg)
    T, S, U = lx.shape[0], lx.shape[1], lu.shape[1]
    gain, kff, d0, d1 = np.zeros((T, U, S), dtype=dt), np.zeros((T, U), dtype=dt), [dt(0)] * T, [dt(0)] * T
    den = huu[T - 1] + reg
    if not (den > 0).all():
        raise np.linalg.LinAlgError("huu + reg <= 0 in the last row")
    Vx, Vxx = lx[T - 1].copy(), np.diag(hxx[T - 1])
    kff[T - 1] = -lu[T - 1] / den
    d0[T - 1], d1[T - 1] = kff[T - 1] @ lu[T - 1], kff[T - 1] @ (den * kff[T - 1])
    cond = float((den.max() / den.min()))
    for t in range(T - 2, -1, -1):
        Qx, Qu = lx[t] + A[t].T @ Vx, lu[t] + B[t].T @ Vx
        Qxx = np.diag(hxx[t]) + A[t].T @ Vxx @ A[t]
        Qux = B[t].T @ Vxx @ A[t]
        Quu = np.diag(huu[t]) + B[t].T @ Vxx @ B[t] + reg * np.eye(U, dtype=dt)
        cond = max(cond, float(np.linalg.cond(np.asarray(Quu, dtype=np.float64))))
        L = _cholesky(Quu, dt)
        kff[t] = -_chol_solve(L, Qu.reshape(U, 1), dt)[:, 0]
        gain[t] = _chol_solve(L, Qux, dt)
        d0[t], d1[t] = kff[t] @ Qu, kff[t] @ Quu @ kff[t]
        Vx = Qx + Qux.T @ kff[t]
        W = Qxx - Qux.T @ gain[t]
        Vxx = (W + W.T) / dt(2)
    s0, s1 = dt(0), dt(0)
    for t in range(T):  # ascending
        s0, s1 = s0 + d0[t], s1 + d1[t]
    return gain, kff, np.array([s0, s1], dtype=dt), cond


def riccati_truth_ld(A, B, lx, lu, hxx, huu, reg):
    """riccati_truth in numpy.longdouble (its inputs are the float64 operands, exactly)."""
    return riccati_truth(A, B, lx, lu, hxx, huu, reg, dt=np.longdouble)


def d_ref(f64, ld):
    """Per output (gain, kff, dv): the largest difference between the float64 and the long-double recursion, relative to the output's
    largest entry -- the truth's own rounding on this case."""
    out = []
    for a, b in zip(f64[:3], ld[:3]):
        b = np.asarray(b, dtype=np.longdouble)
        out.append(float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max() / np.abs(b).max()))
    return out


def lq_stacked(A, B, lx, lu, hxx, huu, t0, x_t0):
    """The tail problem from row t0 with dx_{t0} = x_t0 given, as ONE linear system: the states are eliminated (dx = F x_t0 + G da, stacked
    over the rows t0 .. T - 1) and the stationarity of the quadratic cost in the stacked inputs is solved with numpy.linalg.solve.  Returns
    the optimal da [T - t0, U]."""
    T, S, U = lx.shape[0], lx.shape[1], lu.shape[1]
    n = T - t0
    F, G = np.zeros((n * S, S)), np.zeros((n * S, n * U))
    F[:S] = np.eye(S)
    for i in range(1, n):
        t = t0 + i - 1  # the transition t -> t + 1 fills block row i
        F[i * S:(i + 1) * S] = A[t] @ F[(i - 1) * S:i * S]
        G[i * S:(i + 1) * S] = A[t] @ G[(i - 1) * S:i * S]
        G[i * S:(i + 1) * S, (i - 1) * U:i * U] += B[t]
    Hx, Hu = np.diag(hxx[t0:].reshape(-1)), np.diag(huu[t0:].reshape(-1))
    gx, gu = lx[t0:].reshape(-1), lu[t0:].reshape(-1)
    da = np.linalg.solve(G.T @ Hx @ G + Hu, -(G.T @ (gx + Hx @ (F @ x_t0)) + gu))
    return da.reshape(n, U)


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def ilqr_truth(shape, m, x0, a_init, cost, iterations, u_max=1.0, squashed=True, reg_init=1e-6, reg_factor=10.0, reg_max=1e6,
               alphas=(1, .5, .25, .125, .0625), armijo=1e-4, tol=1e-9):
    """The loop of policy_learning/ilqr.py on oracle_step (mean form, one trajectory): x0 [S], a_init [T,U], ``cost`` an object with
    ``expansion``.  Returns a dict: "cost" (per pass), "alpha" (per iteration), "passes" (gain, kff, dv of every pass), "operands" (what
    riccati_truth was given in that pass), "states", "a"."""
    a, T = a_init.clone(), a_init.shape[0]
    x0 = x0.reshape(1, -1)
    eps = torch.zeros(T - 1, 1, 1, dtype=DT)
    reg, out, it, done = reg_init, dict(cost=[], alpha=[], passes=[], operands=[]), 0, False
    roll = lambda av: oracle_rollout(shape, m, x0, squash(av, u_max, squashed)[:T - 1].unsqueeze(1), eps, False)
    while True:
        states = roll(a)
        J, lx, lu, hxx, huu, du = cost.expansion(states, a.unsqueeze(1), u_max, squashed)
        A, B = autograd_AB(shape, m, states, squash(a, u_max, squashed).unsqueeze(1), eps, False, du)
        n = lambda v: v[:, 0].numpy()
        while True:
            try:
                gain, kff, dv, _ = riccati_truth(n(A), n(B), n(lx), n(lu), n(hxx), n(huu), reg)
                break
            except np.linalg.LinAlgError:
                if reg * reg_factor > reg_max:
                    raise
                reg = max(reg, reg_init) * reg_factor
        out["cost"].append(float(J[0]))
        out["passes"].append((gain, kff, dv))
        out["operands"].append((n(A), n(B), n(lx), n(lu), n(hxx), n(huu), reg))
        if it >= iterations or done:
            break
        it += 1
        accepted = 0.0
        for alpha in alphas:
            ff, xs, av = a + alpha * torch.as_tensor(kff), [x0], []
            for t in range(T):
                av.append((torch.as_tensor(gain[t]) @ (states[t, 0] - xs[-1][0]) + ff[t]).reshape(1, -1))
                if t < T - 1:
                    with torch.no_grad():
                        xs.append(oracle_step(family(shape), m, xs[-1], squash(av[-1], u_max, squashed), eps[t], False)[0])
            a_new = torch.cat(av)
            J_new = float(cost.expansion(torch.stack(xs), a_new.unsqueeze(1), u_max, squashed)[0][0])
            if out["cost"][-1] - J_new >= armijo * (-(alpha * dv[0] + 0.5 * alpha * alpha * dv[1])):
                accepted, a = float(alpha), a_new
                break
        out["alpha"].append(accepted)
        if accepted:
            reg /= reg_factor
            done = out["cost"][-1] - J_new <= tol * abs(out["cost"][-1])
        elif reg * reg_factor > reg_max:
            done = True
        else:
            reg = max(reg, reg_init) * reg_factor
    out.update(states=states[:, 0], a=a)
    return out
