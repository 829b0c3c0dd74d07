"""Sampling MPC on the learned GP model -- MPPI / random shooting (this project's own: the reference has no planner).

``plan`` improves a pre-squash input sequence a [H,U] from a state x0 by sampling: K candidate sequences a + sigma xi around the nominal
(candidate 0 IS the nominal), each rolled out through the model -- the mean model, or P particles per candidate under common random
numbers -- and scored by a cost of ``Cost_function``; the next nominal is the softmax-weighted mean of the candidates.  It needs no
gradient and no linearisation, works with the saturated costs whose Hessians iLQR cannot use, and its result is the ``a_init`` that
``Policy.TV_linear_controller.from_lqr`` takes.  One iteration is three fused launches of ``ops``:

  rollout-cost   ops.mppi_rollout   (mcp_mppi_rollout: inputs generated, trajectories rolled out and reduced to one number each on the chip)
  update         ops.mppi_update    (mcp_mppi_update: candidate costs and weights in one workgroup, the weighted perturbation sum per row)

and the iterations of one ``plan`` run back to back on the stream with no host synchronisation between them: two nominal buffers are
swapped, ``noise.call`` advances by one per iteration, the statistics of every iteration stay on the device until the end.

``Policy.MPPI_controller`` is the receding-horizon controller over ``plan``.
Beyond the plain planner (``method``, ``beta``, ``sigma_rows``, ``u_prev`` of ``plan``; mcp_plan_ext): the elite-set / CEM update
(ops.cem_update: the elites selected and ranked on the device, mean and std PER ROW fitted to them, smoothed and floored), AR(1)-coloured
perturbations and a std per row (ops.plan_rollout, ops.mppi_update_ext: the colouring happens in the kernels, still one row ahead of the
step), and the input applied before row 0 for the rate term at t = 0.  With all of them at their defaults the calls are the plain ones.
``plan_batch`` is ``plan`` for B start states in the launches of one plan (ops.plan_batch_rollout, ops.plan_batch_update,
ops.cem_batch_update; mcp_plan_batch): a state, a warm start, std rows and u_prev per problem -- or a start state per model particle, for a
set of samples of an uncertain state --, the model, the cost and t0 shared; problem b's result carries the bits of ``plan`` on its operands,
and its statistics stay on the device.  ``Policy.MPPI_controller.forward`` runs it on a batch of particles.
Not built: elites kept across iterations, a momentum on the mean, coloured noise other than AR(1), a throughput layout
for mean-mode planning, GP-sharded forms, the measured (PMS) form, a t0 or a cost per problem of a batch."""
import numpy as np
import torch

from mc_pilco_amd import ops
from mc_pilco_amd.policy_learning.ilqr import _packed_model


class _Like:
    """What a cost object reads of a tensor [., ., n] when it chooses and packs its descriptor: nothing is allocated."""

    def __init__(self, n, device):
        self.shape, self.device, self.dtype, self.is_cuda = (0, 0, int(n)), torch.device(device), ops.DT, torch.device(device).type == "cuda"

    def dim(self):
        return 3


def kernel_cost(cost, S, U, H, device, trial_index=None):
    """(PackedCost, PackedCostInputs or None, time weights [H] on ``device`` or None) of a ``Cost_function`` object the HIP cost kernels
    evaluate -- ``runs_on_kernels()``: Cart_pole_cost, the trajectory and target costs, an ``Input_penalty`` over one of them, a
    ``Cost_shaping`` with time weights / a discount (counted from the plan's row 0) -- else NotImplementedError.  A ``Cost_shaping`` with
    risk != 0 is refused too: its std is per time step over the swarm, the planner's ``kappa`` is over a candidate's trajectory costs.
    ``trial_index``: for a trajectory cost with per-trial lengthscales."""
    from mc_pilco_amd.policy_learning import Cost_function as cf

    like_x = _Like(S, device)
    if not isinstance(cost, cf._HipExpectedCost) or not cost.runs_on_kernels(like_x):
        raise NotImplementedError("mppi plans under the costs the HIP cost kernels evaluate (Cost_function's classes with runs_on_kernels()), "
                                  "not under %s" % type(cost).__name__)
    w = None
    if isinstance(cost, cf.Cost_shaping):
        if cost.risk != 0.0:
            raise NotImplementedError("mppi: a Cost_shaping with risk != 0 is not a per-trajectory cost (use kappa)")
        if not cost._plain:
            w = ops._t(ops.objective_weights(int(H), cost.time_weights, cost.discount), device)
    cin = cost.inputs_packed_for(_Like(U, device))
    return cost.packed_for(like_x, trial_index), cin, w


def _check_rows(pc, t0, H):
    if pc.kind == "traj" and pc.traj_len < int(t0) + int(H):
        raise ValueError("the cost's target trajectory has %d rows but the plan reads rows %d .. %d" % (pc.traj_len, int(t0), int(t0) + int(H) - 1))


def plan(model, x0, a_init, cost, K, P=1, iterations=1, sigma=0.3, lam=1.0, kappa=0.0, u_max=1.0, flg_squash=True, particle_pred=False,
         noise=None, t0=0, trial_index=None, method="mppi", n_elite=None, alpha=0.1, sigma_min=0.0, beta=0.0, sigma_rows=None, u_prev=None):
    """MPPI on the GP model from the state ``x0`` [S] and the pre-squash input sequence ``a_init`` [H,U] (row H - 1 moves nothing but enters
    the cost).  ``model``: an ops.PackedModel or a Model_learning with a fused layout; ``cost``: see ``kernel_cost``; ``K`` candidates,
    ``P`` model particles each (``particle_pred``: sampled increments under common random numbers, else the mean model); ``sigma`` the
    perturbation's std per input in the pre-squash variable, ``lam`` the temperature, ``kappa`` the weight of the particles' std in a
    candidate's cost; ``noise``: an ops.NoiseSpec -- seed, call (iteration i plans with call + i; an ``eps`` buffer [H-1,P,G] is read by
    every iteration) -- None: seed 0, call 0; ``t0``: the row of the cost's target trajectory that plan row 0 reads (receding horizon);
    ``trial_index``: for a trajectory cost with per-trial lengthscales.
    ``method``: "mppi" (the softmax-weighted mean) or "cem" -- the next nominal and the next std PER ROW are fitted to the ``n_elite``
    cheapest candidates (None: K // 8, at least 1), smoothed by ``alpha`` towards the previous ones, the std floored at ``sigma_min``; the
    temperature is not read.  ``beta`` in [0, 1): AR(1)-coloured perturbations xi_t = beta xi_{t-1} + sqrt(1 - beta^2) n_t (0: white);
    ``sigma_rows`` [H,U]: a std per row and input in place of ``sigma`` (host values; CEM starts from it); ``u_prev`` [U]: the post-squash
    input applied before row 0 -- the rate term of the cost at t = 0 is then taken against it.  With every one of these at its default the
    calls are those of the plain planner (ops.mppi_rollout, ops.mppi_update); otherwise ops.plan_rollout with ops.mppi_update_ext or
    ops.cem_update.  CEM carries (a, std) in two swapped buffer pairs and returns, beside "S_min", "nominal_cost", "status" and
    "iterations": "sigma" [H,U] (the final std, on the device), "elite_cost" (the elites' mean cost) and "n_elite_used" per iteration,
    "elite" (every iteration's ranked candidate indices).

    Runs ``iterations`` x (rollout-cost, update) on the current stream without a host synchronisation in between.  Returns (a, info):
    ``a`` [H,U] the new nominal; ``info``: "S_min", "nominal_cost" (the cost of the nominal each iteration STARTED from, cand_cost[0]),
    "ess" (effective sample size) and "mean_cost" per iteration as lists, "status" (the status words OR-ed), "iterations".
    NotImplementedError for a cost the kernels do not evaluate, ValueError for a trajectory cost with fewer than t0 + H rows."""
    pm = _packed_model(model)
    dev = pm.device
    x0 = torch.as_tensor(x0).detach().to(device=dev, dtype=ops.DT).reshape(-1).contiguous()
    a = torch.as_tensor(a_init).detach().to(device=dev, dtype=ops.DT).contiguous().clone()
    if x0.numel() != pm.S or a.dim() != 2 or a.shape[1] != pm.U or a.shape[0] < 2:
        raise ValueError("mppi.plan takes x0 [%d] and a_init [H >= 2, %d]" % (pm.S, pm.U))
    H, n_it = int(a.shape[0]), int(iterations)
    if n_it < 1:
        raise ValueError("mppi.plan: at least one iteration")
    if method not in ("mppi", "cem"):
        raise ValueError("mppi.plan: method is \"mppi\" or \"cem\" (%r)" % (method,))
    mp = ops.PackedMPPI(K, P, H, pm.U, sigma, lam, kappa, u_max, flg_squash)
    plain = method == "mppi" and float(beta) == 0.0 and sigma_rows is None and u_prev is None
    if not plain:
        ext = ops.PackedPlanExt(H, pm.U, beta, sigma_rows, max(1, int(K) // 8) if n_elite is None else n_elite, alpha, sigma_min)
        if method == "cem" and ext.n_elite > mp.K:
            raise ValueError("mppi.plan: %d elites of %d candidates" % (ext.n_elite, mp.K))
        if u_prev is not None:
            u_prev = ops._t(u_prev, dev).reshape(-1)
    pc, cin, w = kernel_cost(cost, pm.S, pm.U, H, dev, trial_index)
    _check_rows(pc, t0, H)
    noise = ops.NoiseSpec() if noise is None else noise
    new = lambda *s: torch.empty(*s, dtype=ops.DT, device=dev)
    b, traj, cand, wts, stats = new(H, pm.U), new(mp.M), new(n_it, mp.K), new(mp.K), new(n_it, 4)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if method == "cem":
        s = (ext.rows_on(dev) if sigma_rows is not None else ops._t(np.tile(mp.sigma, (H, 1)), dev)).clone()
        s2, elite = new(H, pm.U), torch.empty(n_it, ext.n_elite, dtype=torch.int32, device=dev)
    for i in range(n_it):
        nz = ops.NoiseSpec(eps=noise.eps, seed=noise.seed, call=int(noise.call) + i, particle_offset=noise.particle_offset, call_dev=noise.call_dev)
        if plain:
            ops.mppi_rollout(pm, mp, pc, x0, a, cost_inputs=cin, noise=nz, particle_pred=particle_pred, w=w, t0=t0, traj_cost=traj, status=status)
            ops.mppi_update(mp, traj, a, noise=nz, a_new=b, out=(cand[i], wts, stats[i]), status=status)
        elif method == "mppi":
            ops.plan_rollout(pm, mp, ext, pc, x0, a, u_prev=u_prev, cost_inputs=cin, noise=nz, particle_pred=particle_pred, w=w, t0=t0,
                             traj_cost=traj, status=status)
            ops.mppi_update_ext(mp, ext, traj, a, noise=nz, a_new=b, out=(cand[i], wts, stats[i]), status=status)
        else:
            ops.plan_rollout(pm, mp, ext, pc, x0, a, sigma_rows=s, u_prev=u_prev, cost_inputs=cin, noise=nz, particle_pred=particle_pred, w=w,
                             t0=t0, traj_cost=traj, status=status)
            ops.cem_update(mp, ext, traj, a, sigma_rows=s, noise=nz, a_new=b, sigma_new=s2, out=(cand[i], elite[i], stats[i]), status=status)
            s, s2 = s2, s
        a, b = b, a
    st, nom = stats.cpu(), cand[:, 0].cpu()  # (the one synchronisation)
    if method == "cem":
        return a, dict(S_min=st[:, 0].tolist(), nominal_cost=nom.tolist(), elite_cost=st[:, 3].tolist(), n_elite_used=[int(v) for v in st[:, 2].tolist()],
                       elite=[[k for k in row if k >= 0] for row in elite.cpu().tolist()], sigma=s, status=int(status.item()), iterations=n_it)
    info = dict(S_min=st[:, 0].tolist(), nominal_cost=nom.tolist(), ess=st[:, 2].tolist(), mean_cost=st[:, 3].tolist(),
                status=int(status.item()), iterations=n_it)
    return a, info


def _per_problem(name, v, one, B, dev):
    """``v`` -- host values or a tensor of the shape ``one`` (shared by the problems) or [B] + ``one`` -- as a contiguous float64 tensor
    [B] + ``one`` of its own on ``dev``."""
    t = torch.as_tensor(v).detach().to(device=dev, dtype=ops.DT)
    if tuple(t.shape) == tuple(one):
        return t.unsqueeze(0).repeat(B, *([1] * len(one)))
    if tuple(t.shape) != (B,) + tuple(one):
        raise ValueError("mppi.plan_batch: %s must have the shape %s or %s, not %s" % (name, list(one), [B] + list(one), list(t.shape)))
    return t.contiguous().clone()


def plan_batch(model, x0, a_init, cost, K, P=1, iterations=1, sigma=0.3, lam=1.0, kappa=0.0, u_max=1.0, flg_squash=True, particle_pred=False,
               noise=None, t0=0, trial_index=None, method="mppi", n_elite=None, alpha=0.1, sigma_min=0.0, beta=0.0, sigma_rows=None, u_prev=None,
               particle_stride=None):
    """``plan`` for B start states in the launches of one plan: ``x0`` [B,S], or [B,P,S] for a start state per model particle (a set of
    samples of an uncertain state estimate: trajectory k P + p of problem b starts at x0[b,p]); ``a_init`` [H,U] (one warm start for all) or
    [B,H,U]; ``sigma_rows`` [H,U] or [B,H,U] (host values, or a tensor whose values are then read on the host); ``u_prev`` [U] or [B,U];
    every other keyword as in ``plan`` and shared by the problems (the model, the cost, ``t0``, the plan's scalars).  ``particle_stride``:
    problem b draws its perturbations and its model increments as ``plan`` does with ``noise.particle_offset + b * particle_stride`` --
    None: max(K, P), the problems draw independent numbers; 0: common random numbers across the problems.  An ``eps`` buffer of ``noise`` is
    [H-1,P,G] (read by every problem) or [B,H-1,P,G].

    Problem b's result is, bit for bit, that of ``plan`` on its operands with that particle offset.  One iteration is the launches of ONE
    plan whatever B (ops.plan_batch_rollout, ops.plan_batch_update / ops.cem_batch_update); the iterations run back to back with the buffer
    swapping of ``plan`` and NOTHING is read back: returns (a [B,H,U], info) with info's entries DEVICE tensors -- "S_min" and
    "nominal_cost" [iterations,B]; "ess" and "mean_cost", or under CEM "elite_cost", "n_elite_used" (int32) [iterations,B], "elite" int32
    [iterations,B,n_elite] (-1 behind the elites used) and "sigma" [B,H,U]; "status" int32 [B], one word per problem -- and "iterations".  A
    problem with a non-finite start state keeps its nominal, raises MCP_STATUS_NAN in its own status word and leaves the others' bits alone."""
    pm = _packed_model(model)
    dev = pm.device
    x0 = torch.as_tensor(x0).detach().to(device=dev, dtype=ops.DT).contiguous()
    if x0.dim() not in (2, 3) or x0.shape[0] < 1 or x0.shape[-1] != pm.S or (x0.dim() == 3 and x0.shape[1] != int(P)):
        raise ValueError("mppi.plan_batch takes x0 [B,%d] or [B,P = %d,%d]" % (pm.S, int(P), pm.S))
    B = int(x0.shape[0])
    a = torch.as_tensor(a_init).detach()
    if a.dim() not in (2, 3) or a.shape[-1] != pm.U or a.shape[-2] < 2:
        raise ValueError("mppi.plan_batch takes a_init [H >= 2, %d] or [B, H >= 2, %d]" % (pm.U, pm.U))
    H, n_it = int(a.shape[-2]), int(iterations)
    a = _per_problem("a_init", a, (H, pm.U), B, dev)
    if n_it < 1:
        raise ValueError("mppi.plan_batch: at least one iteration")
    if method not in ("mppi", "cem"):
        raise ValueError("mppi.plan_batch: method is \"mppi\" or \"cem\" (%r)" % (method,))
    mp = ops.PackedMPPI(K, P, H, pm.U, sigma, lam, kappa, u_max, flg_squash)
    bt = ops.PackedPlanBatch(B, mp.P, x0.dim() == 3, max(mp.K, mp.P) if particle_stride is None else particle_stride)
    if B * mp.M > ops.abi.MPPI_MAX_M:
        raise ValueError("mppi.plan_batch: at most %d trajectories over all problems (B K P %d)" % (ops.abi.MPPI_MAX_M, B * mp.M))
    plain = method == "mppi" and float(beta) == 0.0 and sigma_rows is None and u_prev is None
    ext = srows = None
    if not plain:
        rows = None if sigma_rows is None else ops._host(sigma_rows)
        if rows is not None and rows.ndim == 3:  # a std per problem: each problem's rows pass the checks of the descriptor
            if rows.shape[0] != B:
                raise ValueError("mppi.plan_batch: sigma_rows must have the shape %s or %s, not %s" % ([H, pm.U], [B, H, pm.U], list(rows.shape)))
            for r in rows:
                ops.PackedPlanExt(H, pm.U, sigma_rows=r)
        ext = ops.PackedPlanExt(H, pm.U, beta, None if rows is None or rows.ndim == 3 else rows, max(1, int(K) // 8) if n_elite is None else n_elite, alpha,
                                sigma_min)
        if method == "cem" and ext.n_elite > mp.K:
            raise ValueError("mppi.plan_batch: %d elites of %d candidates" % (ext.n_elite, mp.K))
        if rows is not None:
            srows = _per_problem("sigma_rows", rows, (H, pm.U), B, dev)
            ext = ops.PackedPlanExt(H, pm.U, beta, None, ext.n_elite, alpha, sigma_min)  # (the rows travel as the device buffer)
        if u_prev is not None:
            u_prev = _per_problem("u_prev", u_prev, (pm.U,), B, dev)
    pc, cin, w = kernel_cost(cost, pm.S, pm.U, H, dev, trial_index)
    _check_rows(pc, t0, H)
    noise = ops.NoiseSpec() if noise is None else noise
    new = lambda *s: torch.empty(*s, dtype=ops.DT, device=dev)
    b, traj, cand, wts, stats = new(B, H, pm.U), new(B, mp.M), new(n_it, B, mp.K), new(B, mp.K), new(n_it, B, 4)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if method == "cem":
        s = srows if srows is not None else ops._t(np.tile(mp.sigma, (B, H, 1)), dev)
        s2, elite = new(B, H, pm.U), torch.empty(n_it, B, ext.n_elite, dtype=torch.int32, device=dev)
    for i in range(n_it):
        nz = ops.NoiseSpec(eps=noise.eps, seed=noise.seed, call=int(noise.call) + i, particle_offset=noise.particle_offset, call_dev=noise.call_dev)
        if method == "mppi":
            ops.plan_batch_rollout(pm, mp, ext, bt, pc, x0, a, sigma_rows=srows, u_prev=u_prev, cost_inputs=cin, noise=nz, particle_pred=particle_pred,
                                   w=w, t0=t0, traj_cost=traj, status=status)
            ops.plan_batch_update(mp, ext, bt, traj, a, sigma_rows=srows, noise=nz, a_new=b, out=(cand[i], wts, stats[i]), status=status)
        else:
            ops.plan_batch_rollout(pm, mp, ext, bt, pc, x0, a, sigma_rows=s, u_prev=u_prev, cost_inputs=cin, noise=nz, particle_pred=particle_pred,
                                   w=w, t0=t0, traj_cost=traj, status=status)
            ops.cem_batch_update(mp, ext, bt, traj, a, sigma_rows=s, noise=nz, a_new=b, sigma_new=s2, out=(cand[i], elite[i], stats[i]), status=status)
            s, s2 = s2, s
        a, b = b, a
    info = dict(S_min=stats[:, :, 0], nominal_cost=cand[:, :, 0], status=status, iterations=n_it)
    if method == "cem":
        info.update(elite_cost=stats[:, :, 3], n_elite_used=stats[:, :, 2].to(torch.int32), elite=elite, sigma=s)
    else:
        info.update(ess=stats[:, :, 2], mean_cost=stats[:, :, 3])
    return a, info


def shift_warm_start(a):
    """The nominal of the next control step: every row moved up by one, the last row repeated ([H,U], or [B,H,U]: every problem's)."""
    return torch.cat([a[..., 1:, :], a[..., -1:, :]], -2).contiguous()
