"""Trajectory optimisation on the learned GP model -- iLQR / TVLQR (this project's own: the reference has no trajectory optimiser).

``ilqr`` computes what ``Policy.TV_linear_controller`` is the controller of: a nominal trajectory of the GP MEAN model, the feedforward
sequence that produces it and a time-varying gain schedule around it.  Every stage of an iteration is one fused launch of ``ops``:

  nominal and record   ops.rollout_open_record on u = squash(a), mean form, one trajectory (mcp_rollout_open_rec)
  backward pass        ops.lqr_pass over the record and the cost's expansion (mcp_lqr_pass: A_t, B_t composed on the chip)
  forward passes       ops.rollout_tvl with target = nominal states, ff = a + alpha kff, the pass's gain (mcp_rollout_tvl)

and the cost's expansion is a handful of torch operations vectorised over the horizon.  The host decides between the launches (line search,
regularisation), so an iteration synchronises a few times; no step of the horizon is a launch of its own.

Sign convention: the controller's law is a = gain (x* - x) + ff.  With x* the nominal the pass's ``gain`` is used as written and the step is
ff <- a + alpha kff.

``Quadratic_tracking_cost`` is the stage cost the pass takes (diagonal Hessians); any object with its ``expansion`` method serves.
Not built: dense cost Hessians, second-order dynamics terms (DDP), box-constrained Quu, wrapped angle errors, iLQR under
the measurement model or on the sampled form, a batched line search."""
import numpy as np
import torch

from mc_pilco_amd import ops


def _squash_bound(u_max, like):
    return torch.as_tensor(np.asarray(u_max, dtype=np.float64), dtype=like.dtype, device=like.device)


class Quadratic_tracking_cost:
    """c_t = 1/2 sum_i ((x[idx_i] - x*_t[idx_i]) / l_i)^2 + 1/2 sum_k ((u_k - u*_k) / r_k)^2 for every row t = 0 .. T - 1 (row T - 1 takes
    part in both terms, as the cost kernels have it).  ``target_traj`` [rows, S] (rows >= T); ``state_indices``: the components idx that
    count (None: all); ``lengthscales``: one per state ([S], read at idx) or one per component that counts ([n_used]);
    ``input_lengthscales`` [U] (None: no input term); ``target_input`` [U] (None: zeros).  The input term is on the APPLIED input
    u = u_max tanh(a / u_max) (or u = a)."""

    def __init__(self, target_traj, lengthscales, state_indices=None, input_lengthscales=None, target_input=None):
        t64 = lambda v: torch.as_tensor(v).detach().to(torch.float64)
        self.target_traj = t64(target_traj)
        if self.target_traj.dim() != 2:
            raise ValueError("target_traj must be [rows, S]")
        S = int(self.target_traj.shape[1])
        self.state_indices = list(range(S)) if state_indices is None else [int(i) for i in state_indices]
        if len(set(self.state_indices)) != len(self.state_indices) or any(i < 0 or i >= S for i in self.state_indices):
            raise ValueError("state_indices must be distinct components of the state")
        ls = t64(lengthscales).reshape(-1)
        if ls.numel() == len(self.state_indices):
            self.lengthscales = ls
        elif ls.numel() == S:
            self.lengthscales = ls[self.state_indices]
        else:
            raise ValueError("lengthscales must hold one entry per state or per component in state_indices")
        self.input_lengthscales = None if input_lengthscales is None else t64(input_lengthscales).reshape(-1)
        self.target_input = None if target_input is None else t64(target_input).reshape(-1)
        if self.input_lengthscales is None and self.target_input is not None:
            raise ValueError("target_input needs input_lengthscales")

    def expansion(self, states, a, u_max=1.0, squash=True):
        """states [T,M,S], a [T,M,U] (the pre-squash inputs) -> (J [M], lx [T,M,S], lu [T,M,U], hxx [T,M,S], huu [T,M,U], du_da [T,M,U]):
        the cost of each trajectory, its gradient and its diagonal Gauss-Newton Hessian along it, the input terms in the variable a --
        l_a = s l_u, h_aa = s^2 h_uu with s = du/da = 1 - tanh^2(a / u_max) (ones without squashing).  Vectorised over T and M."""
        T, S = int(states.shape[0]), int(states.shape[2])
        if int(self.target_traj.shape[0]) < T or int(self.target_traj.shape[1]) != S:
            raise ValueError("target_traj must be [rows >= %d, %d]" % (T, S))
        on = lambda v: v.to(device=states.device, dtype=states.dtype)
        idx = torch.as_tensor(self.state_indices, device=states.device)
        ls = on(self.lengthscales)
        e = (states[:, :, idx] - on(self.target_traj)[:T, idx].unsqueeze(1)) / ls
        J = 0.5 * (e * e).sum(dim=(0, 2))
        lx, hxx = torch.zeros_like(states), torch.zeros_like(states)
        lx[:, :, idx] = e / ls
        hxx[:, :, idx] = (1.0 / (ls * ls)).expand_as(e)
        if squash:
            um = _squash_bound(u_max, a)
            th = torch.tanh(a / um)
            u, s = um * th, 1.0 - th * th
        else:
            u, s = a, torch.ones_like(a)
        lu, huu = torch.zeros_like(a), torch.zeros_like(a)
        if self.input_lengthscales is not None:
            r = on(self.input_lengthscales)
            if r.numel() != a.shape[2]:
                raise ValueError("input_lengthscales must hold one entry per input")
            eu = (u - (0.0 if self.target_input is None else on(self.target_input))) / r
            J = J + 0.5 * (eu * eu).sum(dim=(0, 2))
            lu = s * (eu / r)
            huu = (s * s) * (1.0 / (r * r))
        return J, lx.contiguous(), lu.contiguous(), hxx.contiguous(), huu.contiguous(), s.contiguous()


def _packed_model(model):
    if isinstance(model, ops.PackedModel):
        return model
    like = getattr(model, "steps_like_the_packed_model", None)
    if like is None or not like():
        raise NotImplementedError("ilqr needs an ops.PackedModel or a Model_learning whose step is the one its fused layout describes")
    return model.packed()


def _squash(a, u_max, flg_squash):
    if not flg_squash:
        return a
    um = _squash_bound(u_max, a)
    return um * torch.tanh(a / um)


def ilqr(model, x0, a_init, cost, iterations=20, u_max=1.0, flg_squash=True, reg_init=1e-6, reg_factor=10.0, reg_max=1e6,
         alphas=(1, .5, .25, .125, .0625), armijo=1e-4, tol=1e-9, controller_par=None):
    """iLQR on the GP mean model from the state ``x0`` [S] and the pre-squash input sequence ``a_init`` [T,U] (row T - 1 moves nothing but
    enters the cost).  ``model``: an ops.PackedModel or a Model_learning with a fused layout; ``cost``: an object with
    ``Quadratic_tracking_cost.expansion``.  Per iteration: nominal and record, expansion, backward pass at the current ``reg``
    (multiplied by ``reg_factor`` and repeated while the pass reports MCP_STATUS_NOT_SPD), then forward passes under the time-varying law
    with the steps ``alphas`` in order; a step is accepted when J - J_new >= armijo (-(alpha dv0 + alpha^2 dv1 / 2)).  After an accepted
    step reg /= reg_factor; when none is accepted reg *= reg_factor.  The loop ends after ``iterations`` iterations, when an accepted step
    lowers the cost by less than ``tol`` (relative), or when reg would exceed ``reg_max``; then ONE more pass about the final nominal gives
    the returned gains -- ``iterations=0`` is plain TVLQR about the rollout of ``a_init``.

    Returns (controller, info): a ``Policy.TV_linear_controller`` with ``target_traj`` = the nominal states [T,S], ``ff`` = the nominal a
    [T,U], ``gain`` [T,U,S] of the last pass, the given squashing and bound (``controller_par``: further constructor keywords, e.g.
    flg_train_gains); ``info``: "cost" (the nominal's cost per pass), "alpha" and "reg" per iteration (alpha 0.0: no step accepted),
    "status" (the status word of every pass), "states" [T,S], "a" [T,U], "inputs" [T,U] (the applied inputs of the nominal), "kff" [T,U]
    and "dv" [2] of the last pass, "converged"."""
    from mc_pilco_amd.policy_learning import Policy

    pm = _packed_model(model)
    dev = pm.device
    x0 = torch.as_tensor(x0).detach().to(device=dev, dtype=ops.DT).reshape(1, -1).contiguous()
    a = torch.as_tensor(a_init).detach().to(device=dev, dtype=ops.DT).contiguous()
    if x0.shape[1] != pm.S or a.dim() != 2 or a.shape[1] != pm.U or a.shape[0] < 2:
        raise ValueError("ilqr takes x0 [%d] and a_init [T >= 2, %d]" % (pm.S, pm.U))
    T = int(a.shape[0])
    reg, info = float(reg_init), dict(cost=[], alpha=[], reg=[], status=[], converged=False)
    it = 0
    while True:
        # ---- nominal, expansion, backward pass ----
        u = _squash(a, u_max, flg_squash)
        states, jac, st_roll = ops.rollout_open_record(pm, x0, u[:T - 1].reshape(T - 1, 1, pm.U).contiguous(), particle_pred=False)
        J, lx, lu, hxx, huu, du_da = cost.expansion(states, a.reshape(T, 1, pm.U), u_max, flg_squash)
        while True:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            gain, kff, dv = ops.lqr_pass(pm, states, jac, lx, lu, hxx, huu, reg=reg, du_da=du_da if flg_squash else None, status=status)
            word = int(status.item()) | int(st_roll.item())
            info["status"].append(word)
            if not (word & ops.abi.STATUS_NOT_SPD) or reg * reg_factor > reg_max:
                break
            reg = max(reg, reg_init) * reg_factor
        J0 = float(J[0])
        info["cost"].append(J0)
        last = it >= int(iterations) or info["converged"] or word != 0
        if last:
            break
        # ---- forward passes: the candidate steps in order ----
        it += 1
        dv0, dv1 = (float(v) for v in dv[0].tolist())
        accepted = 0.0
        for alpha in alphas:
            alpha = float(alpha)
            law = Policy.TV_linear_controller(pm.S, pm.U, gain[0], a + alpha * kff[0], target_traj=states[:, 0], flg_train_gains=False,
                                              flg_train_feedforward=False, flg_squash=flg_squash, u_max=u_max, dtype=ops.DT, device=dev)
            with torch.no_grad():
                xs, _, st_fwd = ops.rollout_tvl(pm, law.packed(), None, x0, T, particle_pred=False)
            a_new = torch.einsum("tus,ts->tu", law.gain.detach(), states[:, 0] - xs[:, 0]) + law.ff.detach()
            J_new = float(cost.expansion(xs, a_new.reshape(T, 1, pm.U), u_max, flg_squash)[0][0])
            if int(st_fwd.item()) == 0 and J0 - J_new >= armijo * (-(alpha * dv0 + 0.5 * alpha * alpha * dv1)):
                accepted, a = alpha, a_new.contiguous()
                break
        info["alpha"].append(accepted)
        info["reg"].append(reg)
        if accepted:
            reg = reg / reg_factor
            info["converged"] = (J0 - J_new) <= tol * max(abs(J0), 1e-300)
        elif reg * reg_factor > reg_max:
            info["converged"] = True  # (nothing more to try: the final pass follows)
        else:
            reg = max(reg, reg_init) * reg_factor
    par = dict(flg_train_gains=True, flg_train_feedforward=True)
    par.update(controller_par or {})
    controller = Policy.TV_linear_controller(pm.S, pm.U, gain[0], a, target_traj=states[:, 0].contiguous(), flg_time_varying_gains=True,
                                             flg_squash=flg_squash, u_max=u_max, dtype=ops.DT, device=dev, **par)
    info.update(states=states[:, 0].contiguous(), a=a, inputs=u, kff=kff[0], dv=dv[0])
    return controller, info
