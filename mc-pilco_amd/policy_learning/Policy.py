"""Control policies on the HIP path -- drop-in for ``policy_learning/Policy.py``.

  Sum_of_gaussians                         Policy.py:153-265   RBF network + dropout + linear + tanh squashing (:52-60)
  Sum_of_gaussians_with_angles             Policy.py:268-335   features [x_nonangle, cos, sin]
  Sum_of_gaussians_with_target_trajectory  Policy.py:338-403   features [x, x*_t - x]

``forward(states, t=None, p_dropout=0.0)`` evaluates the policy with the fused kernel (T = 1) and is
differentiable with respect to ``log_lengthscales``, ``centers`` and ``f_linear.weight`` (names as in the
reference, so ``state_dict``s interoperate).  ``packed()`` exposes the live parameters to the fused rollout.
Dropout noise: ``noise_mode = "philox"`` (in-kernel counter-based generator, default) or ``"torch_cpu"`` (mask
drawn exactly like ``torch.nn.functional.dropout`` draws it on the CPU -- parity with the reference).
``scale_factor`` (plain ``Sum_of_gaussians`` only, as in the reference) is folded into the operands handed to the kernels.
``flg_bias`` adds ``f_linear.bias`` (not dropped out) to the linear layer inside the kernels; its gradient comes out of the adjoint sweep.
``MLP_policy`` (this project's own: a tanh multilayer perceptron on the same features) runs inside the fused closed loop, mcp_rollout_mlp;
with ``target_traj`` it tracks: the errors target_traj[t] - x behind its features (Policy.py:389-403's map), mcp_rollout_mlp_track.
``Residual_MLP_policy`` keeps a PD law (PD_controller's term, :437-449) and adds the network as its correction ahead of the one squashing,
u = squash(PD(x, t) + net(x, t)), mcp_rollout_mlp_res.
``PID_controller`` (this project's own) is PD_controller with a clamped integral of the position error and a third trainable gain; it runs
inside the fused closed loop like its parent, mcp_rollout_pid.
``MPPI_controller`` (this project's own) is the receding-horizon sampling planner on the learned model: policy_learning/mppi.py once per control
step (mcp_mppi_rollout, mcp_mppi_update; with ``method="cem"``, ``beta``, ``sigma_rows`` or ``charge_first_rate`` the entries of mcp_plan_ext); no trainable parameters, host-side interface (``forward_np``, ``get_np_policy``).
Exploration policies (Random_exploration, Sum_of_sinusoids :94-150, PD_controller :406-449) drive the simulated system once per
trial (61-201 samples): host-side, their ``np.random`` draws in the reference's order so that a seeded launch script collects the
same data.
"""
import numpy as np
import torch

from mc_pilco_amd import ops


class Policy(torch.nn.Module):
    def __init__(self, state_dim, input_dim, flg_squash=False, u_max=1, dtype=torch.float64, device=torch.device("cuda")):
        super().__init__()
        self.state_dim = state_dim
        self.input_dim = input_dim
        self.dtype = dtype
        self.device = torch.device(device)
        self.flg_squash = flg_squash
        self.u_max = u_max

    def forward(self, states, t=None, p_dropout=0.0):
        raise NotImplementedError()

    def forward_np(self, state, t=None):
        with torch.no_grad():
            u = self(states=torch.as_tensor(np.asarray(state), dtype=self.dtype).to(self.device), t=t)
        return u.detach().cpu().numpy()

    def to(self, device):
        super().to(device)
        self.device = torch.device(device)

    def squashing(self, u, u_max):
        """u_max tanh(u / u_max), u_max a scalar or one bound per input (Policy.py:52-60).  The fused kernels apply the same
        squashing inside the rollout; this method is the reference's public helper for user code."""
        if not np.isscalar(u_max):
            u_max = torch.tensor(u_max, dtype=self.dtype, device=self.device)
        return u_max * torch.tanh(u / u_max)

    def f_squash(self, x):
        """The reference's ``self.f_squash`` (Policy.py:28-33): squashing when ``flg_squash``, identity otherwise."""
        return self.squashing(x, self.u_max) if self.flg_squash else x

    def get_np_policy(self):
        return lambda state, t: self.forward_np(state, t)

    def reinit(self, scaling=1):
        raise NotImplementedError()


class Random_exploration(Policy):
    """Uniform random input in (-u_max, u_max); host-side, used only to collect data from the system."""

    def __init__(self, state_dim, input_dim, flg_squash=True, u_max=1.0, dtype=torch.float64, device=torch.device("cpu")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)

    def forward(self, states, t=None, p_dropout=0.0):
        return torch.as_tensor(self.forward_np(states, t), dtype=self.dtype)

    def forward_np(self, state, t=None):
        return (np.asarray(self.u_max) * (2 * np.random.rand(self.input_dim) - 1)).reshape([-1, self.input_dim])


class Sum_of_sinusoids(Policy):
    """Exploration policy: u(t) = squash(sum_i A_i sin(omega_i t + phi_i)) with random amplitudes / frequencies / phases
    (Policy.py:94-150).  The draws are ``np.random``'s, in the reference's order: amplitudes (rand), omega (choice, rand),
    phases (choice, rand) -- a launch script seeded with ``np.random.seed`` gets the reference's exploration signal."""

    def __init__(self, state_dim, input_dim, num_sin, omega_min, omega_max, amplitude_min, amplitude_max, flg_squash=False, u_max=1,
                 dtype=torch.float64, device=torch.device("cpu")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        self.num_sin = num_sin
        amplitude_min, amplitude_max = np.array(amplitude_min), np.array(amplitude_max)
        par = lambda a: torch.nn.Parameter(torch.tensor(a, dtype=self.dtype, device=self.device), requires_grad=False)
        self.amplitudes = par(amplitude_min + (amplitude_max - amplitude_min) * np.random.rand(num_sin, input_dim))
        self.omega = par(np.random.choice([-1, 1], [num_sin, input_dim]) * (omega_min + (omega_max - omega_min) * np.random.rand(num_sin, input_dim)))
        self.phases = par(np.random.choice([-1, 1], [num_sin, input_dim]) * (np.pi * (np.random.rand(num_sin, input_dim) - 0.5)))

    def forward(self, states, t, p_dropout=0.0):
        return self.f_squash(torch.sum(self.amplitudes * torch.sin(self.omega * t + self.phases), dim=0).reshape([-1, self.input_dim]))


class PD_controller(Policy):
    """u = squash(Kp e_q + Kd e_qdot) with e = target_traj[t] - state, gains = sqrt_*_gains^2 (Policy.py:406-449; the UR5 launch
    script's tracking controller, and with ``flg_trainable`` the reference's second trainable policy).  ``forward`` is the reference's
    torch expression: the system simulator calls it once per sample.  As ``MC_PILCO``'s control policy on a GPU model with a fused
    layout it runs inside the fused closed-loop rollout (``packed()``, ``fusable()``; ops.rollout_pd: one launch, and the reverse-time
    sweep for the gradients of the two gain parameters)."""

    def __init__(self, state_dim, input_dim, sqrt_Kp_gains, sqrt_Kd_gains, target_traj=None, flg_squash=True, u_max=1.0, flg_trainable=False,
                 dtype=torch.float64, device=torch.device("cpu")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        self.target_traj = target_traj
        self.sqrt_Kp_gains = torch.nn.Parameter(torch.tensor(sqrt_Kp_gains, dtype=self.dtype, device=self.device), requires_grad=flg_trainable)
        self.sqrt_Kd_gains = torch.nn.Parameter(torch.tensor(sqrt_Kd_gains, dtype=self.dtype, device=self.device), requires_grad=flg_trainable)

    def packed(self) -> "ops.PackedPD":
        """mcp_pd_policy over the LIVE gain parameters (rebuilt if a tensor or the target was replaced)."""
        key = (self.sqrt_Kp_gains.data_ptr(), self.sqrt_Kd_gains.data_ptr(), id(self.target_traj), self.flg_squash, id(self.u_max))
        hit = self.__dict__.get("_packed_pd")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed_pd"] = (key, ops.PackedPD(self))
        return hit[1]

    def fusable(self, model, T):
        """Whether T steps of this controller on ``model`` (an ops.PackedModel, or anything with ``S`` and ``U``) can run as the fused
        closed loop: the reference's index layout needs an even S with one input per position (input_dim == S / 2), each gain holds one
        value per input (or one for all: expanded on the host), the target covers the horizon, and everything is float64 on a GPU."""
        S = int(self.state_dim)
        if S % 2 != 0 or int(self.input_dim) != S // 2 or int(self.input_dim) > ops.abi.MAX_INPUT:
            return False
        if int(getattr(model, "S", -1)) != S or int(getattr(model, "U", -1)) != int(self.input_dim):
            return False
        if any(int(g.numel()) not in (1, int(self.input_dim)) for g in (self.sqrt_Kp_gains, self.sqrt_Kd_gains)):
            return False
        tt = self.target_traj
        if tt is None or np.ndim(tt) != 2 or int(np.shape(tt)[0]) < int(T) or int(np.shape(tt)[1]) != S:
            return False
        if not np.isscalar(self.u_max) and np.asarray(self.u_max).size != int(self.input_dim):
            return False
        if self.dtype != torch.float64 or any(g.dtype != torch.float64 or not g.is_cuda for g in (self.sqrt_Kp_gains, self.sqrt_Kd_gains)):
            return False
        return True

    def forward(self, states, t, p_dropout=0.0):
        states = states.reshape([-1, self.state_dim])
        err = self.target_traj[t, :].reshape(1, -1) - states
        h = int(self.state_dim / 2)
        return self.f_squash(self.sqrt_Kp_gains ** 2 * err[:, 0:h] + self.sqrt_Kd_gains ** 2 * err[:, h:])


class PID_controller(PD_controller):
    """PD_controller with an integral term and anti-windup (this project's own: the reference has none).  Per input k, with e = target_traj[t]
    - state, p = k and v = state_dim / 2 + k (PD_controller's layout):
        I_t[k] = clamp(I_{t-1}[k] + T_sampling e[p], -i_max[k], +i_max[k]),  I_{-1} = 0
        u[k]   = squash(sqrt_Kp^2 e[p] + sqrt_Kd^2 e[v] + sqrt_Ki^2 I_t[k])
    ``i_max``: None (no clamp), a scalar, or one bound per input (inf: that input unclamped).  The clamp passes gradient where I_t lies
    strictly inside its bounds.  ``flg_trainable`` covers the three gains.  ``forward(states, t)`` is the torch formula of the step loop and
    of the system simulator; it HOLDS the integral: t == 0 resets it, every other call must come with the previous t + 1 and the same number
    of particles (ValueError otherwise).  As ``MC_PILCO``'s control policy it runs inside the fused closed loop like its parent
    (``packed()``: an ops.PackedPID, mcp_rollout_pid and its sweep), where the integral is a register of the launch and this object's is not
    touched."""

    def __init__(self, state_dim, input_dim, sqrt_Kp_gains, sqrt_Kd_gains, sqrt_Ki_gains, T_sampling, i_max=None, target_traj=None, flg_squash=True,
                 u_max=1.0, flg_trainable=False, dtype=torch.float64, device=torch.device("cpu")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, sqrt_Kp_gains=sqrt_Kp_gains, sqrt_Kd_gains=sqrt_Kd_gains, target_traj=target_traj,
                         flg_squash=flg_squash, u_max=u_max, flg_trainable=flg_trainable, dtype=dtype, device=device)
        self.sqrt_Ki_gains = torch.nn.Parameter(torch.tensor(sqrt_Ki_gains, dtype=self.dtype, device=self.device), requires_grad=flg_trainable)
        self.T_sampling = float(T_sampling)
        self.i_max = i_max
        self._integral, self._t_prev = None, None

    def _i_max_values(self):
        """One bound per input as floats (inf: no clamp), or None when ``i_max`` does not describe that."""
        U = int(self.input_dim)
        if self.i_max is None or np.isscalar(self.i_max):
            return [float("inf") if self.i_max is None else float(self.i_max)] * U
        v = [float(x) for x in np.asarray(self.i_max, dtype=float).reshape(-1)]
        return v if len(v) == U else None

    def packed(self) -> "ops.PackedPID":
        """mcp_pd_policy and mcp_pid_term over the LIVE gain parameters (rebuilt if a tensor, the target, the step or the bound was replaced)."""
        key = (self.sqrt_Kp_gains.data_ptr(), self.sqrt_Kd_gains.data_ptr(), self.sqrt_Ki_gains.data_ptr(), id(self.target_traj), self.flg_squash,
               id(self.u_max), self.T_sampling, id(self.i_max))
        hit = self.__dict__.get("_packed_pid")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed_pid"] = (key, ops.PackedPID(self))
        return hit[1]

    def fusable(self, model, T):
        """The parent's conditions, and the term's: the third gain holds one value per input (or one for all) in float64 on the GPU,
        T_sampling > 0, every bound > 0."""
        if not super().fusable(model, T):
            return False
        ki = self.sqrt_Ki_gains
        if int(ki.numel()) not in (1, int(self.input_dim)) or ki.dtype != torch.float64 or not ki.is_cuda:
            return False
        im = self._i_max_values()
        return bool(self.T_sampling > 0.0) and im is not None and all(v > 0.0 for v in im)

    def forward(self, states, t, p_dropout=0.0):
        states = states.reshape([-1, self.state_dim])
        t = int(t)
        if t == 0:
            self._integral = torch.zeros(states.shape[0], self.input_dim, dtype=states.dtype, device=states.device)
        elif self._t_prev is None or t != self._t_prev + 1:
            raise ValueError("PID_controller.forward holds the integral: called with t = %d after t = %s (t == 0 resets it)" % (t, self._t_prev))
        elif self._integral.shape[0] != states.shape[0]:
            raise ValueError("PID_controller.forward holds the integral of %d particles, called with %d" % (self._integral.shape[0], states.shape[0]))
        self._t_prev = t
        err = self.target_traj[t, :].reshape(1, -1) - states
        h = int(self.state_dim / 2)
        im = self._i_max_values()
        if im is None:
            raise ValueError("i_max must be None, a scalar or hold one bound per input")
        bound = torch.tensor(im, dtype=states.dtype, device=states.device)
        q = self._integral = torch.clamp(self._integral + self.T_sampling * err[:, 0:h], -bound, bound)
        return self.f_squash(self.sqrt_Kp_gains ** 2 * err[:, 0:h] + self.sqrt_Kd_gains ** 2 * err[:, h:] + self.sqrt_Ki_gains ** 2 * q)


class TV_linear_controller(Policy):
    """Feedforward sequence plus time-varying linear feedback around a reference (this project's own: the reference has none) -- the local
    controller of trajectory optimisation (iLQR / TVLQR, guided policy search).  For row t, with e = target_traj[t] - state:
        a[k] = sum_s gain[t][k][s] e[s] + ff[t][k];    u[k] = squash(a[k])
    ``gain`` is [rows, U, S] (``flg_time_varying_gains=False``: [U, S], one matrix for every row), plain (not squared) and dense over all S
    components -- no index layout applies, S may be odd and U need not be S / 2; ``ff`` is [rows, U] or None (no feedforward);
    ``target_traj`` is [rows, S].  The error is the plain difference, not wrapped on angle components.  ``flg_train_gains`` /
    ``flg_train_feedforward`` choose which of the two is a trainable Parameter.  ``from_pd`` builds a ``PD_controller``'s law as the special
    case; ``from_lqr`` computes nominal, feedforward and gains by iLQR on the GP mean model (policy_learning/ilqr.py).  ``forward(states, t)`` is the torch formula of the step loop and of the system simulator; it is stateless and raises ValueError
    for a row the tensors do not have.  As ``MC_PILCO``'s control policy it runs inside the fused closed loop (``packed()``: an
    ops.PackedTVL, mcp_rollout_tvl and its sweep, whose parameter gradient is per row)."""

    def __init__(self, state_dim, input_dim, gain, ff=None, target_traj=None, flg_time_varying_gains=True, flg_train_gains=True,
                 flg_train_feedforward=True, flg_squash=True, u_max=1.0, dtype=torch.float64, device=torch.device("cpu")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        self.flg_time_varying_gains = bool(flg_time_varying_gains)
        self.target_traj = target_traj
        gain = torch.as_tensor(gain, dtype=self.dtype).detach().clone().to(self.device)
        want = (3 if self.flg_time_varying_gains else 2)
        if gain.dim() != want or tuple(gain.shape[-2:]) != (int(input_dim), int(state_dim)):
            raise ValueError("gain must be [rows, U, S] (flg_time_varying_gains=False: [U, S]), got %s" % (tuple(gain.shape),))
        self.gain = torch.nn.Parameter(gain.contiguous(), requires_grad=bool(flg_train_gains))
        self.ff = None
        if ff is not None:
            ff = torch.as_tensor(ff, dtype=self.dtype).detach().clone().to(self.device)
            if ff.dim() != 2 or int(ff.shape[1]) != int(input_dim):
                raise ValueError("ff must be [rows, U], got %s" % (tuple(ff.shape),))
            self.ff = torch.nn.Parameter(ff.contiguous(), requires_grad=bool(flg_train_feedforward))

    @classmethod
    def from_pd(cls, pd_controller, T, flg_feedforward=True, **kwargs):
        """The law of ``pd_controller`` (a PD_controller: input k reads position k and velocity S / 2 + k) over T rows:
        gain[t][k][k] = sqrt_Kp[k]^2, gain[t][k][S / 2 + k] = sqrt_Kd[k]^2, ff = 0 (``flg_feedforward=False``: none).  Target, squashing,
        bound, dtype and device are the controller's; ``kwargs`` go to the constructor."""
        S, U, T = int(pd_controller.state_dim), int(pd_controller.input_dim), int(T)
        with torch.no_grad():
            kp2 = (pd_controller.sqrt_Kp_gains.detach().reshape(-1) ** 2).expand(U)
            kd2 = (pd_controller.sqrt_Kd_gains.detach().reshape(-1) ** 2).expand(U)
            g = torch.zeros(U, S, dtype=pd_controller.dtype, device=kp2.device)
            idx = torch.arange(U, device=kp2.device)
            g[idx, idx] = kp2
            g[idx, S // 2 + idx] = kd2
            tv = kwargs.pop("flg_time_varying_gains", True)
            gain = g.unsqueeze(0).repeat(T, 1, 1) if tv else g
            ff = torch.zeros(T, U, dtype=pd_controller.dtype, device=kp2.device) if flg_feedforward else None
        args = dict(target_traj=pd_controller.target_traj, flg_squash=pd_controller.flg_squash, u_max=pd_controller.u_max,
                    dtype=pd_controller.dtype, device=pd_controller.device)
        args.update(kwargs)
        return cls(S, U, gain, ff, flg_time_varying_gains=tv, **args)

    @classmethod
    def from_lqr(cls, model, x0, a_init, cost, **kwargs):
        """The controller iLQR computes on the GP mean model of ``model`` (an ops.PackedModel, or a Model_learning with a fused layout) from
        the state ``x0`` [S] and the pre-squash input sequence ``a_init`` [T, U] under ``cost`` (an ilqr.Quadratic_tracking_cost):
        ``target_traj`` = the optimised nominal states, ``ff`` = its pre-squash inputs, ``gain`` = the time-varying LQR gains about it --
        the starting point of guided policy search, which ``MC_PILCO.reinforce_policy`` then trains on the particles.
        ``flg_train_gains`` / ``flg_train_feedforward`` go to the constructor (``flg_time_varying_gains`` must be True: the gains are per
        row); every other keyword is ``policy_learning.ilqr.ilqr``'s (iterations, u_max, flg_squash, reg_init, ...).  ``iterations=0`` is
        plain TVLQR about the rollout of ``a_init``."""
        from mc_pilco_amd.policy_learning.ilqr import ilqr

        if not kwargs.pop("flg_time_varying_gains", True):
            raise ValueError("from_lqr computes one gain matrix per row: flg_time_varying_gains must be True")
        par = {k: kwargs.pop(k) for k in ("flg_train_gains", "flg_train_feedforward") if k in kwargs}
        return ilqr(model, x0, a_init, cost, controller_par=par, **kwargs)[0]

    def _rows(self):
        rows = [int(np.shape(self.target_traj)[0])] if self.target_traj is not None else [0]
        if self.flg_time_varying_gains:
            rows.append(int(self.gain.shape[0]))
        if self.ff is not None:
            rows.append(int(self.ff.shape[0]))
        return min(rows)

    def packed(self) -> "ops.PackedTVL":
        """mcp_tvl_policy over the LIVE tensors (rebuilt if a tensor or the target was replaced)."""
        key = (self.gain.data_ptr(), None if self.ff is None else self.ff.data_ptr(), id(self.target_traj), self.flg_squash, id(self.u_max))
        hit = self.__dict__.get("_packed_tvl")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed_tvl"] = (key, ops.PackedTVL(self))
        return hit[1]

    def fusable(self, model, T):
        """Whether T steps of this controller on ``model`` (an ops.PackedModel, or anything with ``S`` and ``U``) can run as the fused
        closed loop: S and U are the model's and within the compiled limits, gain, ff and the target cover the horizon, and everything is
        float64 on a GPU."""
        S, U = int(self.state_dim), int(self.input_dim)
        if U < 1 or U > ops.abi.MAX_INPUT or S > ops.abi.MAX_STATE:
            return False
        if int(getattr(model, "S", -1)) != S or int(getattr(model, "U", -1)) != U:
            return False
        tt = self.target_traj
        if tt is None or np.ndim(tt) != 2 or int(np.shape(tt)[1]) != S or self._rows() < int(T) or int(T) < 1:
            return False
        if not np.isscalar(self.u_max) and np.asarray(self.u_max).size != U:
            return False
        tensors = [self.gain] + ([self.ff] if self.ff is not None else [])
        return self.dtype == torch.float64 and all(q.dtype == torch.float64 and q.is_cuda for q in tensors)

    def forward(self, states, t, p_dropout=0.0):
        t = int(t)
        if t < 0 or t >= self._rows():
            raise ValueError("TV_linear_controller.forward: row %d is beyond the %d rows of gain / ff / target_traj" % (t, self._rows()))
        states = states.reshape([-1, self.state_dim])
        err = self.target_traj[t, :].reshape(1, -1) - states
        a = err @ (self.gain[t] if self.flg_time_varying_gains else self.gain).T
        if self.ff is not None:
            a = a + self.ff[t].reshape(1, -1)
        return self.f_squash(a)


class MPPI_controller(Policy):
    """Receding-horizon sampling MPC on the learned model (this project's own: the reference has none) -- ``policy_learning.mppi.plan`` once
    per control step.  ``forward_np(state, t)`` plans ``iterations`` MPPI iterations from ``state`` over the horizon of the warm start
    (``a_init`` [H, U], pre-squash; None: zeros over ``horizon`` rows), returns the applied input u_0 = squash(a[0]) and shifts the nominal
    one row for the next step, repeating the last row.  ``t == 0`` starts an episode: the warm start is ``a_init`` again, the step count
    and the noise's call are those of the first step (two episodes plan with the same draws).  The controller counts its own steps -- the
    system simulator hands ``t`` in seconds -- and step k plans with ``t0 = k`` when the cost tracks a trajectory
    (Expected_saturated_distance_from_trajectory, alone or wrapped: it needs k + H rows), else ``t0 = 0``; its call is
    ``noise.call + k * iterations``, so no two iterations of an episode share perturbations.  ``plan_par``: ``plan``'s further keywords
    (K, P, sigma, lam, kappa, particle_pred, and method, n_elite, alpha, sigma_min, beta, sigma_rows); every control step starts from the
    std given here -- CEM's narrowed std is not carried over.  ``charge_first_rate``: each plan after an episode's first is handed the input
    this controller returned last as ``u_prev``, so that a cost with a rate term charges the jump from the input just applied (step 0 of an
    episode passes nothing).  ``info``: the last plan's.  It has no trainable parameters; ``get_np_policy()`` drives
    ``simulation_class.Model.rollout``.
    ``forward(states [M, S], t)`` plans for M states at once -- ``policy_learning.mppi.plan_batch``: one plan per row in the launches of one,
    a warm start per row, nothing read back -- and returns u_0 [M, U] on the device: as ``MC_PILCO``'s control policy the controller runs
    the generic step loop of ``apply_policy`` (one model step per launch), which simulates the MPC on M particles of the model before it is
    put on the system.  Row b plans as ``forward_np`` would under ``noise.particle_offset + b * particle_stride`` (``particle_stride``: a
    keyword of this class, None: max(K, P); 0: common random numbers across the rows).  ``forward`` keeps its own episode state (warm starts,
    last inputs, step) apart from ``forward_np``'s, under the contract of ``PID_controller.forward``: ``t`` is the step index, t == 0 resets,
    every other call follows the previous t by one with the same M.  ``batch_info``: the last batched plan's (device tensors).  Training an
    ``MPPI_controller`` in ``reinforce_policy`` is not built: it has nothing to train."""

    def __init__(self, state_dim, input_dim, model, cost, horizon=None, a_init=None, iterations=5, noise=None, flg_squash=True, u_max=1.0,
                 dtype=torch.float64, device=torch.device("cuda"), charge_first_rate=False, **plan_par):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        if a_init is None:
            if horizon is None or int(horizon) < 2:
                raise ValueError("MPPI_controller needs a_init [H, U] or a horizon of at least 2 rows")
            a_init = torch.zeros(int(horizon), int(input_dim), dtype=torch.float64)
        self.a_init = torch.as_tensor(a_init, dtype=torch.float64).detach().clone()
        if self.a_init.dim() != 2 or int(self.a_init.shape[1]) != int(input_dim) or int(self.a_init.shape[0]) < 2:
            raise ValueError("a_init must be [H >= 2, U], got %s" % (tuple(self.a_init.shape),))
        self.__dict__.update(model=model, cost=cost)  # (kept out of this module's registry: the planner owns no parameters)
        self.iterations, self.plan_par = int(iterations), dict(plan_par)
        self.particle_stride = self.plan_par.pop("particle_stride", None)  # (plan_batch's alone: forward_np plans one problem)
        self.noise = ops.NoiseSpec() if noise is None else noise
        self.a, self.step, self.info = self.a_init, 0, None
        self.charge_first_rate, self.u_last = bool(charge_first_rate), None
        self._batch_a, self._batch_u, self._batch_t, self._batch_um, self.batch_info = None, None, None, None, None  # forward's own episode

    def _tracks(self):
        from mc_pilco_amd.policy_learning import Cost_function as cf

        c = self.cost
        while isinstance(c, (cf.Input_penalty, cf.Cost_shaping)):
            c = c.state_cost if isinstance(c, cf.Input_penalty) else c.cost
        return isinstance(c, cf.Expected_saturated_distance_from_trajectory)

    def forward(self, states, t=None, p_dropout=0.0):
        """One plan per row of ``states`` [M, S] in the launches of one plan (``policy_learning.mppi.plan_batch``): returns u_0 [M, U] on the
        device, without grad and without a host synchronisation.  ``t`` is the STEP INDEX (``int(t)``), as for ``PID_controller``: t == 0
        starts an episode, every other call must come with the previous t + 1 and the same M (ValueError otherwise).  ``p_dropout`` is accepted
        and ignored."""
        from mc_pilco_amd.policy_learning import mppi

        if t is None:
            raise ValueError("MPPI_controller.forward holds a warm start per particle: it needs the step index t (t == 0 resets it)")
        t = int(t)
        with torch.no_grad():
            x = states.detach().reshape(-1, int(self.state_dim)).to(device=self.device, dtype=torch.float64).contiguous()
            M = int(x.shape[0])
            if t == 0:
                self._batch_a, self._batch_u = self.a_init.to(self.device).unsqueeze(0).repeat(M, 1, 1), None
            elif self._batch_t is None or t != self._batch_t + 1:
                raise ValueError("MPPI_controller.forward holds the warm starts: called with t = %d after t = %s (t == 0 resets them)" % (t, self._batch_t))
            elif int(self._batch_a.shape[0]) != M:
                raise ValueError("MPPI_controller.forward holds the warm starts of %d particles, called with %d" % (int(self._batch_a.shape[0]), M))
            nz = ops.NoiseSpec(eps=self.noise.eps, seed=self.noise.seed, call=int(self.noise.call) + t * self.iterations,
                               particle_offset=self.noise.particle_offset, call_dev=self.noise.call_dev)
            par = dict(self.plan_par, u_prev=self._batch_u) if self.charge_first_rate and self._batch_u is not None else self.plan_par
            a, self.batch_info = mppi.plan_batch(self.model, x, self._batch_a, self.cost, iterations=self.iterations, u_max=self.u_max,
                                                 flg_squash=self.flg_squash, noise=nz, t0=t if self._tracks() else 0,
                                                 particle_stride=self.particle_stride, **par)
            u0 = a[:, 0]
            if self.flg_squash:
                if self._batch_um is None or self._batch_um.device != a.device:
                    self._batch_um = torch.as_tensor(np.asarray(self.u_max, dtype=np.float64)).to(a.device)
                u0 = self._batch_um * torch.tanh(u0 / self._batch_um)
            self._batch_a, self._batch_u, self._batch_t = mppi.shift_warm_start(a), u0.contiguous(), t
            return self._batch_u

    def forward_np(self, state, t=None):
        from mc_pilco_amd.policy_learning import mppi

        if t is not None and float(t) == 0.0:
            self.a, self.step, self.u_last = self.a_init, 0, None
        nz = ops.NoiseSpec(eps=self.noise.eps, seed=self.noise.seed, call=int(self.noise.call) + self.step * self.iterations,
                           particle_offset=self.noise.particle_offset, call_dev=self.noise.call_dev)
        a, self.info = mppi.plan(self.model, np.asarray(state, dtype=np.float64).reshape(-1), self.a, self.cost, iterations=self.iterations,
                                 u_max=self.u_max, flg_squash=self.flg_squash, noise=nz, t0=self.step if self._tracks() else 0,
                                 **(dict(self.plan_par, u_prev=self.u_last) if self.charge_first_rate and self.u_last is not None else self.plan_par))
        u0 = a[0].detach().cpu()
        if self.flg_squash:
            um = torch.as_tensor(np.asarray(self.u_max, dtype=np.float64))
            u0 = um * torch.tanh(u0 / um)
        self.a, self.step, self.u_last = mppi.shift_warm_start(a), self.step + 1, u0.numpy().reshape(-1).copy()
        return u0.numpy().reshape(1, -1)


class MLP_policy(Policy):
    """Tanh multilayer perceptron (this project's own policy class; the reference has none).  Features as in
    ``Sum_of_gaussians_with_angles``, in the order f = [x[non_angle], sin x[angle], cos x[angle]] (both lists None: f = x); then
    h1 = tanh(W0 f + b0), optionally h2 = tanh(W1 h1 + b1), a = Wout h + bout and u = u_max tanh(a / u_max) (``flg_squash``) or u = a.
    ``hidden_sizes``: one or two widths, each 1..64.  The parameters are separate contiguous float64 tensors in the order W0, b0, [W1, b1],
    Wout, bout; by default the weights are randn / sqrt(fan_in) and the biases zero (``weight_init``: the tensors' values in that order).
    ``forward`` is the torch formula.  As ``MC_PILCO``'s control policy on a GPU model with a fused layout it runs inside the fused closed
    loop (``packed()``, ``fusable()``; ops.rollout_mlp: one launch, and the reverse-time sweep for the parameters' gradients); with
    ``MC_PILCO.fused_feedback = False`` the same object runs the step loop.
    Dropout (``flg_drop=True``; MC-PILCO's regulariser, which the RBF policies have on their basis functions): inverted dropout on the hidden
    units behind the activation, h_l = keep_l * tanh(.) / (1 - p_dropout) with one row ``keep`` of ``drop_width`` = sum(hidden_sizes)
    decisions per call and particle, layer 0's units first; features, the output layer and the squashing are never dropped.  ``forward``
    draws the row with ONE ``bernoulli_(1 - p)`` call, ``MC_PILCO.reference_draws``' own (on ``draw_device``, set by MC_PILCO in "reference"
    noise mode, else on the policy's device), so the step loop and the fused launch see the same masks from the same seed; the fused
    launch takes them as a buffer or draws them in the kernel (ops.rollout_mlp, ``p_drop``).  ``flg_drop=False`` (the default):
    ``p_dropout`` is accepted and ignored.
    Tracking (``target_traj`` [rows, S]; the feature map of the reference's ``Sum_of_gaussians_with_target_trajectory``,
    policy_learning/Policy.py:389-403, behind this class's own): the evaluation at time step ``t`` appends the errors
    target_traj[t][i] - x[i], i in ``error_indices`` (default: all S components in order; the plain difference, not wrapped on angles),
    so f = [x[non_angle], sin x[angle], cos x[angle], errors], ``feature_dim`` counts them and W0's last columns are theirs.  ``forward`` and
    ``features`` then need ``t``.  The fused loop (mcp_rollout_mlp_track) reads row t of the target in policy evaluation t; the target is a
    constant: it gets no gradient.  ``target_traj=None`` (the default): the class without any of it.
    Memory (``history`` = H, 1 .. 4): the network reads the features of the last H rows it was shown, so that it can learn its own estimator
    from them.  ``MC_PILCO`` runs it fused; ``MC_PILCO4PMS`` does NOT (no measured form of the kernels is built): there the object runs the
    step loop, ``last_feedback_fused`` False, this ``forward`` holding the window.  With r_t the row of evaluation t and phi the map above (width P0),
        f_t = [phi(r_t), phi(r_{t-1}), ..., phi(r_{t-H+1}), errors_t],   r_{t-j} := r_0 for t - j < 0
    the newest block first, the errors (of the current row only) last, rows before 0 REPEATING row 0 (no zero padding: f_0 is H copies of
    phi(r_0), and row 0 collects the gradient of every block clamped onto it); ``feature_dim`` = H P0 + the errors, at most 32 (ValueError
    otherwise).  A residual policy's PD term reads the current row only; dropout acts on the hidden units as before.  ``forward`` and
    ``features`` then need ``t`` and HOLD the window the way ``PID_controller.forward`` holds its integral: t == 0 resets it, every other
    call must come with the previous t + 1 and the same number of particles (ValueError otherwise).  The fused loop (mcp_rollout_mlp_hist)
    keeps the window in the launch's LDS and never touches this object's.  ``t`` is the STEP INDEX (``int(t)``), as for ``PID_controller``:
    a caller that passes time in seconds -- the system simulator behind ``get_data_from_system`` does, t = k dt -- resets the window while
    t < 1 and is refused at the first repeated integer, so a policy with memory cannot be deployed through that loop as it stands.  The held
    window keeps the last rollout's autograd graph alive until the next ``t == 0`` (``reset_window()`` drops it).  ``history=1`` (the
    default): the class without any of it."""

    def __init__(self, state_dim, input_dim, hidden_sizes, angle_indices=None, non_angle_indices=None, u_max=1.0, flg_squash=True, weight_init=None,
                 dtype=torch.float64, device=torch.device("cuda"), flg_drop=False, target_traj=None, error_indices=None, history=1):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        self.history = int(history)
        if not 1 <= self.history <= ops.abi.MAX_HIST:
            raise ValueError("history is 1 .. %d rows" % ops.abi.MAX_HIST)
        self._window, self._t_prev = None, None
        self.flg_drop = bool(flg_drop)
        self.target_traj = None if target_traj is None else torch.as_tensor(target_traj).detach().to(self.device)  # (its own dtype: fusable() asks for float64)
        if target_traj is None and error_indices is not None:
            raise ValueError("error_indices needs a target_traj")
        self.error_indices = [] if target_traj is None else (list(range(int(state_dim))) if error_indices is None else
                                                             [int(i) for i in np.atleast_1d(error_indices)])
        self.hidden_sizes = [int(h) for h in np.atleast_1d(hidden_sizes)]
        if len(self.hidden_sizes) not in (1, 2) or any(h < 1 for h in self.hidden_sizes):
            raise ValueError("hidden_sizes holds one or two positive widths")
        self.angle_indices = [] if angle_indices is None else [int(i) for i in np.atleast_1d(angle_indices)]
        self.non_angle_indices = [] if non_angle_indices is None else [int(i) for i in np.atleast_1d(non_angle_indices)]
        self._lists = bool(self.angle_indices or self.non_angle_indices)
        self.feature_dim = self.history * (len(self.non_angle_indices) + 2 * len(self.angle_indices) if self._lists else int(state_dim)) + len(self.error_indices)
        if self.history > 1 and self.feature_dim > ops.abi.MAX_PFEAT:
            raise ValueError("a policy with memory has at most %d features: history * own features + errors = %d" % (ops.abi.MAX_PFEAT, self.feature_dim))
        self.drop_width = sum(self.hidden_sizes)  # a row of dropout decisions: the hidden units, layer 0's first
        widths = [self.feature_dim] + self.hidden_sizes + [int(input_dim)]
        names = ["0", "1", "out"] if len(self.hidden_sizes) == 2 else ["0", "out"]
        self._names = []
        for l, n in enumerate(names):
            self.register_parameter("W" + n, torch.nn.Parameter(torch.zeros(widths[l + 1], widths[l], dtype=dtype, device=self.device)))
            self.register_parameter("b" + n, torch.nn.Parameter(torch.zeros(widths[l + 1], dtype=dtype, device=self.device)))
            self._names += ["W" + n, "b" + n]
        if weight_init is None:
            self.reinit()
        else:
            if len(weight_init) != len(self._names):
                raise ValueError("weight_init holds %d arrays: %s" % (len(self._names), ", ".join(self._names)))
            for q, v in zip(self.mlp_parameters(), weight_init):
                q.data.copy_(torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=dtype).reshape(q.shape))

    def mlp_parameters(self):
        """The parameter tensors in the order W0, b0, [W1, b1], Wout, bout (the order of mcp_rollout_mlp_bwd's slabs)."""
        return [getattr(self, n) for n in self._names]

    def reinit(self, scaling=1):
        """Weights redrawn as scaling * randn / sqrt(fan_in), biases zero; ``draw_device`` (set by MC_PILCO in "reference" noise mode): where
        the draws are made."""
        ddev = getattr(self, "draw_device", None) or self.device
        for q in self.mlp_parameters():
            if q.dim() == 2:
                q.data.copy_(scaling * torch.randn(q.shape, dtype=self.dtype, device=ddev).to(self.device) / np.sqrt(q.shape[1]))
            else:
                q.data.zero_()

    def reset_window(self):
        """Forgets the held window (and with it the autograd graph of the rollout that filled it); the next call must come with t == 0."""
        self._window, self._t_prev = None, None

    def _window_blocks(self, own, t):
        """[phi(r_t), phi(r_{t-1}), ..., phi(r_{t-H+1})] with ``own`` = phi(r_t); holds the H - 1 newest blocks for the next call."""
        if t is None:
            raise ValueError("an MLP_policy with memory is evaluated at a time step: pass t")
        t = int(t)
        if t == 0:
            self._window = [own] * (self.history - 1)  # (rows before 0 repeat row 0)
        elif self._t_prev is None or t != self._t_prev + 1:
            raise ValueError("MLP_policy.forward holds the window: called with t = %d after t = %s (t == 0 resets it)" % (t, self._t_prev))
        elif self._window[0].shape[0] != own.shape[0]:
            raise ValueError("MLP_policy.forward holds the window of %d particles, called with %d" % (self._window[0].shape[0], own.shape[0]))
        self._t_prev = t
        blocks = [own] + self._window
        self._window = blocks[:self.history - 1]
        return blocks

    def features(self, states, t=None):
        x = states.reshape([-1, self.state_dim])
        if self.history > 1:
            own = torch.cat([x[:, self.non_angle_indices], torch.sin(x[:, self.angle_indices]), torch.cos(x[:, self.angle_indices])], dim=1) if self._lists else x
            blocks = self._window_blocks(own, t)
            if self.target_traj is not None:
                row = torch.as_tensor(self.target_traj).to(x.device)[int(t)].reshape(1, -1)
                blocks = blocks + [row[:, self.error_indices] - x[:, self.error_indices]]
            return torch.cat(blocks, dim=1)
        if self.target_traj is None:
            if not self._lists:
                return x
            return torch.cat([x[:, self.non_angle_indices], torch.sin(x[:, self.angle_indices]), torch.cos(x[:, self.angle_indices])], dim=1)
        if t is None:
            raise ValueError("a tracking MLP_policy is evaluated at a time step: pass t")
        row = torch.as_tensor(self.target_traj).to(x.device)[int(t)].reshape(1, -1)
        err = row[:, self.error_indices] - x[:, self.error_indices]
        own = [x[:, self.non_angle_indices], torch.sin(x[:, self.angle_indices]), torch.cos(x[:, self.angle_indices])] if self._lists else [x]
        return torch.cat(own + [err], dim=1)

    def forward(self, states, t=None, p_dropout=0.0):
        return self.f_squash(self.network(states, t, p_dropout))

    def network(self, states, t=None, p_dropout=0.0):
        """a = Wout h + bout: the network's output ahead of the squashing."""
        h = self.features(states, t)
        ps = self.mlp_parameters()
        p = float(p_dropout) if self.flg_drop else 0.0
        keep = None
        if p > 0.0:
            M, H = h.shape[0], self.drop_width
            ddev = getattr(self, "draw_device", None) or self.device
            keep = torch.empty(M, 1, H, dtype=self.dtype, device=ddev).bernoulli_(1 - p).reshape(M, H).to(self.device)
        off = 0
        for l, width in enumerate(self.hidden_sizes):
            h = torch.tanh(h @ ps[2 * l].t() + ps[2 * l + 1])
            if keep is not None:
                h = keep[:, off:off + width] * h * (1.0 / (1.0 - p))
                off += width
        return h @ ps[-2].t() + ps[-1]

    def _u_max_values(self):
        """The bounds as a tuple of floats (a scalar: one entry), or None where ``u_max`` is nothing of the kind."""
        try:
            u = self.u_max.detach().cpu().numpy() if isinstance(self.u_max, torch.Tensor) else self.u_max
            return tuple(float(v) for v in np.asarray(u, dtype=np.float64).reshape(-1))
        except (TypeError, ValueError):
            return None

    def packed(self) -> "ops.PackedMLP":
        """mcp_mlp_policy over the LIVE parameters (rebuilt if a tensor or the target was replaced or a setting changed)."""
        tt = self.target_traj
        key = tuple(q.data_ptr() for q in self.mlp_parameters()) + (self.flg_squash, self._u_max_values(), id(tt),
                                                                    tt.data_ptr() if isinstance(tt, torch.Tensor) else None, tuple(self.error_indices))
        key += (self.history,) + self._packed_key_extra()
        hit = self.__dict__.get("_packed_mlp")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_packed_mlp"] = (key, ops.PackedMLP(self))
        return hit[1]

    def fusable(self, model, T):
        """Whether T steps of this policy on ``model`` (an ops.PackedModel, or anything with ``S`` and ``U``) can run as the fused closed loop:
        float64 parameters on a GPU, S and U those of the model, the index lists in range and disjoint, every width within the kernels' limits
        (``feature_dim``, the window's blocks and the error features included, at most MAX_PFEAT; ``history`` 1 .. MAX_HIST); with a target: a float64 tensor [rows >= T, S], the error indices in
        range and distinct."""
        S, U = int(self.state_dim), int(self.input_dim)
        if int(getattr(model, "S", -1)) != S or int(getattr(model, "U", -1)) != U or U > ops.abi.MAX_INPUT or S > ops.abi.MAX_STATE or int(T) < 1:
            return False
        if self.dtype != torch.float64 or any(q.dtype != torch.float64 or not q.is_cuda for q in self.mlp_parameters()):
            return False
        idx = self.angle_indices + self.non_angle_indices
        if any(i < 0 or i >= S for i in idx) or len(set(idx)) != len(idx):
            return False
        tt, err = self.target_traj, self.error_indices
        if tt is not None:
            if not isinstance(tt, torch.Tensor) or tt.dtype != torch.float64 or tt.dim() != 2 or int(tt.shape[1]) != S or int(tt.shape[0]) < int(T):
                return False
            if any(i < 0 or i >= S for i in err) or len(set(err)) != len(err):
                return False
        if not 1 <= int(self.history) <= ops.abi.MAX_HIST:
            return False
        if self.feature_dim < 1 or self.feature_dim > ops.abi.MAX_PFEAT or any(h < 1 or h > ops.abi.MAX_HIDDEN for h in self.hidden_sizes):
            return False
        um = self._u_max_values()  # (by value: a list of bounds changed in place gives a new descriptor, a tensor on any device is read)
        if um is None or len(um) not in (1, U) or (len(um) == 1 and not np.isscalar(self.u_max) and U != 1):
            return False
        if self.flg_squash and not all(v > 0 for v in um):
            return False
        return True

    def _packed_key_extra(self):
        return ()


class Residual_MLP_policy(MLP_policy):
    """A PD law with a learned correction, u = squash(PD(x, t) + net(x, t)): ``PD_controller``'s term
        a_pd[k] = sqrt_Kp_gains[k]^2 (pd_target_traj[t][pos[k]] - x[pos[k]]) + sqrt_Kd_gains[k]^2 (pd_target_traj[t][vel[k]] - x[vel[k]])
    added to ``MLP_policy``'s output a = Wout h + bout AHEAD of the one squashing (one actuator bound); errors are plain differences,
    dropout never touches the PD term, and the target is a constant.  ``MLP_policy``'s arguments, and
      sqrt_Kp_gains, sqrt_Kd_gains   the gains' square roots (``torch.nn.Parameter``s): one value per input, or one for all
      flg_train_gains                ``requires_grad`` of the two
      pd_target_traj                 [rows, S]; None: ``target_traj``, which is then required
      pd_pos_indices, pd_vel_indices the state components input k reads; None: the reference's layout 0 .. U-1 and S/2 .. S/2+U-1,
                                     which needs an even S and U == S/2 -- otherwise both lists are required
      zero_output                    Wout and bout start at zero and ``reinit`` leaves them zero: training starts from the PD law itself
    ``error_indices=[]``: the network sees no error features while the PD term still has its target.  ``forward`` is the torch formula;
    inside ``MC_PILCO`` the fused closed loop is mcp_rollout_mlp_res (ops.rollout_mlp), its sweep returning the gains' gradients behind
    the network's."""

    def __init__(self, state_dim, input_dim, hidden_sizes, angle_indices=None, non_angle_indices=None, u_max=1.0, flg_squash=True, weight_init=None,
                 dtype=torch.float64, device=torch.device("cuda"), flg_drop=False, target_traj=None, error_indices=None, history=1, *,
                 sqrt_Kp_gains, sqrt_Kd_gains, flg_train_gains=False, pd_target_traj=None, pd_pos_indices=None, pd_vel_indices=None, zero_output=False):
        super().__init__(state_dim, input_dim, hidden_sizes, angle_indices=angle_indices, non_angle_indices=non_angle_indices, u_max=u_max,
                         flg_squash=flg_squash, weight_init=weight_init, dtype=dtype, device=device, flg_drop=flg_drop, target_traj=target_traj,
                         error_indices=error_indices, history=history)
        S, U = int(state_dim), int(input_dim)
        if pd_target_traj is None and target_traj is None:
            raise ValueError("the PD term needs a target: pd_target_traj or target_traj")
        self.pd_target_traj = self.target_traj if pd_target_traj is None else torch.as_tensor(pd_target_traj).detach().to(self.device)
        if (pd_pos_indices is None) != (pd_vel_indices is None):
            raise ValueError("pd_pos_indices and pd_vel_indices come together")
        if pd_pos_indices is None:
            if S % 2 != 0 or U != S // 2:
                raise ValueError("the default PD layout needs an even state_dim and input_dim == state_dim / 2: pass pd_pos_indices and pd_vel_indices")
            pd_pos_indices, pd_vel_indices = range(U), range(S // 2, S // 2 + U)
        self.pd_pos_indices, self.pd_vel_indices = [int(i) for i in pd_pos_indices], [int(i) for i in pd_vel_indices]
        if len(self.pd_pos_indices) != U or len(self.pd_vel_indices) != U:
            raise ValueError("pd_pos_indices and pd_vel_indices hold one state component per input")
        gain = lambda g: torch.nn.Parameter(torch.as_tensor(np.asarray(g.detach().cpu() if isinstance(g, torch.Tensor) else g), dtype=dtype)
                                            .to(self.device).contiguous(), requires_grad=bool(flg_train_gains))
        self.sqrt_Kp_gains, self.sqrt_Kd_gains = gain(sqrt_Kp_gains), gain(sqrt_Kd_gains)
        if any(int(g.numel()) not in (1, U) for g in (self.sqrt_Kp_gains, self.sqrt_Kd_gains)):
            raise ValueError("a gain holds one value per input, or one for all")
        self.zero_output = bool(zero_output)
        if self.zero_output:
            self._zero_output_layer()

    def _zero_output_layer(self):
        for q in self.mlp_parameters()[-2:]:
            q.data.zero_()

    def reinit(self, scaling=1):
        super().reinit(scaling)
        if getattr(self, "zero_output", False):
            self._zero_output_layer()

    def gains(self):
        """(sqrt_kp, sqrt_kd) as [U] tensors on the parameters' autograd graph: views, or a scalar gain expanded to every input."""
        U = int(self.input_dim)
        return [g.reshape(-1).expand(U) if g.numel() == 1 and U > 1 else g.reshape(-1) for g in (self.sqrt_Kp_gains, self.sqrt_Kd_gains)]

    def pd_term(self, states, t):
        x = states.reshape([-1, self.state_dim])
        kp, kd = self.gains()
        e = torch.as_tensor(self.pd_target_traj).to(x.device)[int(t)].reshape(1, -1) - x
        return kp ** 2 * e[:, self.pd_pos_indices] + kd ** 2 * e[:, self.pd_vel_indices]

    def forward(self, states, t=None, p_dropout=0.0):
        if t is None:
            raise ValueError("a Residual_MLP_policy is evaluated at a time step: pass t")
        return self.f_squash(self.network(states, t, p_dropout) + self.pd_term(states, t))

    def _packed_key_extra(self):
        pt = self.pd_target_traj
        return (self.sqrt_Kp_gains.data_ptr(), self.sqrt_Kd_gains.data_ptr(), id(pt), pt.data_ptr() if isinstance(pt, torch.Tensor) else None,
                tuple(self.pd_pos_indices), tuple(self.pd_vel_indices))

    def fusable(self, model, T):
        """``MLP_policy.fusable``, and: float64 gains on a GPU, the PD target a float64 tensor [rows >= T, S], pos and vel in range and each
        without a repeated entry."""
        if not super().fusable(model, T):
            return False
        S = int(self.state_dim)
        if any(g.dtype != torch.float64 or not g.is_cuda for g in (self.sqrt_Kp_gains, self.sqrt_Kd_gains)):
            return False
        pt = self.pd_target_traj
        if not isinstance(pt, torch.Tensor) or pt.dtype != torch.float64 or pt.dim() != 2 or int(pt.shape[1]) != S or int(pt.shape[0]) < int(T):
            return False
        for lst in (self.pd_pos_indices, self.pd_vel_indices):
            if any(i < 0 or i >= S for i in lst) or len(set(lst)) != len(lst):
                return False
        return True


class Sum_of_gaussians(Policy):
    _kind = "plain"

    def __init__(self, state_dim, input_dim, num_basis, flg_train_lengthscales=True, lengthscales_init=None, flg_train_centers=True,
                 centers_init=None, centers_init_min=-1, centers_init_max=1, weight_init=None, flg_train_weight=True, flg_bias=False,
                 bias_init=None, flg_train_bias=False, flg_squash=False, u_max=1, scale_factor=None, flg_drop=True, dtype=torch.float64,
                 device=torch.device("cuda")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, flg_squash=flg_squash, u_max=u_max, dtype=dtype, device=device)
        self.num_basis = num_basis
        if lengthscales_init is None:
            lengthscales_init = np.ones(state_dim)
        self.log_lengthscales = torch.nn.Parameter(torch.tensor(np.log(lengthscales_init), dtype=dtype, device=self.device).reshape([1, -1]),
                                                   requires_grad=flg_train_lengthscales)
        if centers_init is None:
            centers_init = centers_init_min + (centers_init_max - centers_init_min) * np.random.rand(num_basis, state_dim)
        self.centers = torch.nn.Parameter(torch.tensor(np.asarray(centers_init), dtype=dtype, device=self.device), requires_grad=flg_train_centers)
        self.f_linear = torch.nn.Linear(in_features=num_basis, out_features=input_dim, bias=bool(flg_bias))
        w = np.ones([input_dim, num_basis]) if weight_init is None else np.asarray(weight_init)
        self.f_linear.weight = torch.nn.Parameter(torch.tensor(w, dtype=dtype, device=self.device).contiguous(), requires_grad=flg_train_weight)
        if flg_bias:  # Policy.py:203-212: torch.nn.Linear's own initial bias unless bias_init is given; trained only with flg_train_bias
            b0 = self.f_linear.bias.detach().to(torch.float64).cpu().numpy() if bias_init is None else np.asarray(bias_init, dtype=float).reshape(-1)
            self.f_linear.bias = torch.nn.Parameter(torch.tensor(b0, dtype=dtype, device=self.device).contiguous(), requires_grad=flg_train_bias)
        # states / scale_factor before the RBF layer (Policy.py:220-222, 252): folded into the operands the kernels see --
        # ((s/f - c)/l)^2 = ((s - c f)/(l f))^2, i.e. centres c*f and log-lengthscales log l + log f (see packed())
        sf = np.ones(state_dim) if scale_factor is None else np.asarray(scale_factor, dtype=float).reshape(-1)
        self.scale_factor = torch.tensor(sf, dtype=dtype, device=self.device).reshape([1, -1])
        self._unit_scale = bool(np.all(sf == 1.0))
        self.flg_drop = flg_drop
        self.noise_mode = "philox"
        self.seed = 0
        self._calls = 0
        self._packed = None

    # ---- descriptors ---------------------------------------------------------------------------------------------
    def _system_state_dim(self):
        return self.state_dim

    def _pack_extra(self):
        return {}

    def packed(self) -> ops.PackedPolicy:
        """mcp_policy over the LIVE parameter tensors (optimizer updates are seen; rebuilt if a tensor was replaced)."""
        if not self._unit_scale:
            # derived operands, rebuilt per call (the parameters move every optimizer step); autograd carries the chain rule
            # back to log_lengthscales / centers through the two elementwise ops
            return ops.PackedPolicy(self._kind, self._system_state_dim(), self.log_lengthscales + torch.log(self.scale_factor),
                                    (self.centers * self.scale_factor).contiguous(), self.f_linear.weight, self.u_max, self.flg_squash,
                                    bias=self.f_linear.bias, **self._pack_extra())
        key = (self.log_lengthscales.data_ptr(), self.centers.data_ptr(), self.f_linear.weight.data_ptr(),
               None if self.f_linear.bias is None else self.f_linear.bias.data_ptr())
        if self._packed is None or self._packed[0] != key:
            pk = ops.PackedPolicy(self._kind, self._system_state_dim(), self.log_lengthscales, self.centers, self.f_linear.weight, self.u_max,
                                  self.flg_squash, bias=self.f_linear.bias, **self._pack_extra())
            self._packed = (key, pk)
        return self._packed[1]

    def reinit(self, lenghtscales_par, centers_par, weight_par):
        """Policy.py:229-240: lengthscales reset, centres uniform in +-centers_par, weights uniform in +-weight_par / 2 (two
        ``torch.rand`` draws, in this order).  ``draw_device`` (set by MC_PILCO in "reference" noise mode) = where the draws are made:
        on the CPU generator they are the reference's own numbers for the same seed."""
        dev, dt = self.device, self.dtype
        ddev = getattr(self, "draw_device", None) or dev
        self.log_lengthscales.data = torch.tensor(np.log(lenghtscales_par), dtype=dt, device=dev).reshape([1, -1])
        self.centers.data = torch.tensor(centers_par, dtype=dt, device=dev) * 2 * (torch.rand(self.num_basis, self.state_dim, dtype=dt, device=ddev).to(dev) - 0.5)
        self.f_linear.weight.data = weight_par * (torch.rand(self.input_dim, self.num_basis, dtype=dt, device=ddev).to(dev) - 0.5)
        self._packed = None

    # ---- evaluation -------------------------------------------------------------------------------------------------
    def dropout_noise(self, M, T, p_dropout):
        """NoiseSpec for T policy evaluations of M particles."""
        p = float(p_dropout) if self.flg_drop else 0.0
        self._calls += 1
        if p > 0.0 and self.noise_mode == "torch_cpu":
            masks = torch.stack([torch.empty(M, 1, self.num_basis, dtype=self.dtype).bernoulli_(1 - p).reshape(M, self.num_basis) for _ in range(T)])
            return ops.NoiseSpec(masks=masks.to(torch.uint8).to(self.device).contiguous()), p
        return ops.NoiseSpec(seed=self.seed, call=self._calls), p

    def forward(self, states, t=None, p_dropout=0.0):
        x = states.reshape([-1, self._system_state_dim()]).to(self.device)
        noise, p = self.dropout_noise(x.shape[0], 1, p_dropout)
        pk = self.packed()
        if pk.kind == "traj":
            pk = self._packed_at(int(t))
        _, inputs, _ = ops.rollout(None, pk, noise, x, 1, p)
        return inputs[0]


class Sum_of_gaussians_with_angles(Sum_of_gaussians):
    _kind = "angles"

    def __init__(self, state_dim, input_dim, num_basis, angle_indices, non_angle_indices, flg_train_lengthscales=True, lengthscales_init=None,
                 flg_train_centers=True, centers_init=None, centers_init_min=-1, centers_init_max=1, weight_init=None, flg_train_weight=True,
                 flg_bias=False, bias_init=None, flg_train_bias=False, flg_squash=False, u_max=1, flg_drop=True, dtype=torch.float64,
                 device=torch.device("cuda")):
        self.angle_indices = np.asarray(angle_indices)
        self.non_angle_indices = np.asarray(non_angle_indices)
        self.num_angle_indices = self.angle_indices.size
        self.num_non_angle_indices = self.non_angle_indices.size
        self._sys_dim = state_dim
        super().__init__(state_dim=state_dim + self.num_angle_indices, input_dim=input_dim, num_basis=num_basis,
                         flg_train_lengthscales=flg_train_lengthscales, lengthscales_init=lengthscales_init, flg_train_centers=flg_train_centers,
                         centers_init=centers_init, centers_init_min=centers_init_min, centers_init_max=centers_init_max, weight_init=weight_init,
                         flg_train_weight=flg_train_weight, flg_bias=flg_bias, bias_init=bias_init, flg_train_bias=flg_train_bias,
                         flg_squash=flg_squash, u_max=u_max, flg_drop=flg_drop, dtype=dtype, device=device)

    def _system_state_dim(self):
        return self._sys_dim

    def _pack_extra(self):
        return dict(angle=[int(i) for i in self.angle_indices], non_angle=[int(i) for i in self.non_angle_indices])


class Sum_of_gaussians_with_target_trajectory(Sum_of_gaussians):
    _kind = "traj"

    def __init__(self, state_dim, input_dim, num_basis, target_traj, flg_train_lengthscales=True, lengthscales_init=None, flg_train_centers=True,
                 centers_init=None, centers_init_min=-1, centers_init_max=1, weight_init=None, flg_train_weight=True, flg_bias=False,
                 bias_init=None, flg_train_bias=False, flg_squash=False, u_max=1, flg_drop=True, dtype=torch.float64, device=torch.device("cuda")):
        super().__init__(state_dim=state_dim, input_dim=input_dim, num_basis=num_basis, flg_train_lengthscales=flg_train_lengthscales,
                         lengthscales_init=lengthscales_init, flg_train_centers=flg_train_centers, centers_init=centers_init,
                         centers_init_min=centers_init_min, centers_init_max=centers_init_max, weight_init=weight_init,
                         flg_train_weight=flg_train_weight, flg_bias=flg_bias, bias_init=bias_init, flg_train_bias=flg_train_bias,
                         flg_squash=flg_squash, u_max=u_max, flg_drop=flg_drop, dtype=dtype, device=device)
        self.target_traj = torch.as_tensor(np.asarray(target_traj.detach().cpu() if isinstance(target_traj, torch.Tensor) else target_traj),
                                           dtype=self.dtype).to(self.device)

    def _system_state_dim(self):
        return self.state_dim // 2

    def _pack_extra(self):
        return dict(target_traj=self.target_traj)

    def _packed_at(self, t):
        """Descriptor whose target row 0 is x*_t (single-step evaluation at time t)."""
        return ops.PackedPolicy("traj", self._system_state_dim(), self.log_lengthscales, self.centers, self.f_linear.weight, self.u_max,
                                self.flg_squash, target_traj=self.target_traj[t:t + 1], bias=self.f_linear.bias)
