"""Expected costs on the HIP path -- drop-in for ``policy_learning/Cost_function.py``.

  Expected_cost.forward                          Cost_function.py:25-36    sum_t mean_m c , sum_t std_m c (unbiased, detached)
  Cart_pole_cost / cart_pole_cost                Cost_function.py:150-182
  Expected_saturated_distance_from_trajectory    Cost_function.py:104-147
  Expected_distance / Expected_saturated_distance    Cost_function.py:39-101

The two costs the launch scripts use run in the HIP cost kernels (forward and state gradient), and so do the two
target-state costs whenever they have ONE target row and are handed float64 GPU states (``runs_on_kernels``): three
launches for cost + gradient, eligible for the recorded attempts of ``MC_PILCO.reinforce_policy`` and for the pooled
sums of a sharded step.  With several target rows, on CPU tensors or in another dtype they evaluate their
``cost_function`` (kept as an attribute: user code may call it) as ordinary torch ops, exactly as before.  A generic
``Expected_cost(cost_function)`` with a user-supplied torch function keeps working the same way (it is user code).
``forward(..., group=None)``: with a torch.distributed group the mean / std pool every rank's particles.

The project's own extension (the reference's cost functions receive ``inputs_sequence`` and ignore it): ``Input_penalty`` adds a
control-effort and an input-rate term on the applied inputs (``input_distance``) to one of the four kernel costs and runs in the HIP
cost kernels too (mcp_cost_u_fwd / mcp_cost_u_bwd), which then return the gradient in the inputs the adjoint sweeps take.
``Cost_shaping`` wraps one of these costs into the time-weighted, risk-sensitive objective J = sum_t w_t (mean_t + risk std_t) (a discount, explicit
per-step weights, PILCO's ``cost.expl``), still three launches on the kernels (mcp_cost_rows / mcp_cost_bwd_shaped); the std term IS differentiated.
"""
import numpy as np
import torch

from mc_pilco_amd import ops


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class Expected_cost(torch.nn.modules.loss._Loss):
    """sum over time of the particle mean of ``cost_function(states, inputs, trial_index)`` [T,M]."""

    def __init__(self, cost_function):
        super().__init__()
        self.cost_function = cost_function

    def forward(self, states_sequence, inputs_sequence, trial_index=None, group=None, counts=None):
        costs = self.cost_function(states_sequence, inputs_sequence, trial_index)
        if group is not None:
            import torch.distributed as dist

            # pooled over the ranks' particles; shards may be uneven: the total count is reduced, never assumed
            if counts is None:
                n = torch.tensor([float(costs.shape[1])], dtype=costs.dtype, device=costs.device)
                dist.all_reduce(n, group=group)
                n = float(n.item())
            else:
                n = float(sum(int(c) for c in counts))
            s1 = costs.sum(1)
            s1_all = s1.detach().clone()
            dist.all_reduce(s1_all, group=group)
            mean = s1_all / n
            m2 = ((costs.detach() - mean[:, None]) ** 2).sum(1)
            dist.all_reduce(m2, group=group)
            return torch.sum(s1) / n + (torch.sum(mean) - torch.sum(s1.detach()) / n), torch.sum(torch.sqrt(m2 / (n - 1)))
        return torch.sum(torch.mean(costs, 1)), torch.sum(torch.std(costs.detach(), 1))

    def local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift=None, sums_out=None):
        """This rank's share of a particle-sharded cost in summable form (sharding.StepReducer): (share = sum_t sum_m c / m_total,
        differentiable;  sums [2T] = per time step sum_m (c - shift_t), sum_m (c - shift_t)^2, detached).  ``sums_out``: where to leave the
        sums (the slot of the step's all-reduce message, sharding.StepMessage.sums)."""
        costs = self.cost_function(states_sequence, inputs_sequence, trial_index)
        d = costs.detach() - (0.0 if shift is None else shift.reshape(-1, 1))
        sums = torch.cat([d.sum(1), (d * d).sum(1)])
        if sums_out is not None:
            sums_out.copy_(sums)
            sums = sums_out
        return costs.sum() / float(m_total), sums

    @staticmethod
    def from_sums(sums, n_total, shift=None, mean_out=None):
        """(cost, std) of the pooled swarm from the all-reduced sums."""
        T = sums.numel() // 2
        a, b = sums[:T], sums[T:]
        mean = a / n_total + (0.0 if shift is None else shift)
        if mean_out is not None:
            mean_out.copy_(mean)
        return torch.sum(mean), torch.sum(torch.sqrt(torch.clamp(b - a * a / n_total, min=0.0) / (n_total - 1)))


class _HipExpectedCost(Expected_cost):
    def __init__(self):
        super().__init__(None)
        self._packed = None   # the descriptor of the last evaluation
        self._packs = {}      # every descriptor made so far, by what packed_for keys it with

    def _pack(self, states, trial_index=None):
        raise NotImplementedError()

    def packed_for(self, states, trial_index=None):
        """The kernels' descriptor of this cost for these states: one per (trial, where the cost depends on it; state width; device), packed
        when first needed and kept for the life of the object (nothing is evicted)."""
        key = (int(trial_index) if getattr(self, "flg_var_lengthscales", False) else None, states.shape[2], states.device)
        if key not in self._packs:
            self._packs[key] = self._pack(states, trial_index)
        self._packed = self._packs[key]
        return self._packed

    def runs_on_kernels(self, states=None):
        """Whether this cost (for these states, when given) is evaluated by the HIP cost kernels: what makes an attempt recordable into a
        HIP graph (MC_PILCO.reinforce_policy).  A subclass that keeps a torch path for some instances or inputs answers for them here."""
        return True

    def inputs_packed_for(self, inputs):
        """The kernels' descriptor of the terms of this cost that read the inputs (ops.PackedCostInputs); None: it reads the states only."""
        return None

    def objective_for(self, states):
        """The kernels' descriptor of what is made of the per-particle costs (ops.PackedObjective); None: sum_t mean_m c."""
        return None

    def forward(self, states_sequence, inputs_sequence=None, trial_index=None, group=None, counts=None):
        if not self.runs_on_kernels(states_sequence):
            return Expected_cost.forward(self, states_sequence, inputs_sequence, trial_index, group, counts)
        return ops.expected_cost(self.packed_for(states_sequence, trial_index), states_sequence, group, counts)

    def local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift=None, sums_out=None):
        if not self.runs_on_kernels(states_sequence):
            return Expected_cost.local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift, sums_out)
        return ops.local_cost(self.packed_for(states_sequence, trial_index), states_sequence, m_total, shift, sums_out)

    @staticmethod
    def from_sums(sums, n_total, shift=None, mean_out=None):
        out = ops.cost_from_sums(sums, n_total, shift, mean_out)
        return out[0], out[1]


class Cart_pole_cost(_HipExpectedCost):
    """1 - exp(-((|theta|-theta*)/l_theta)^2 - ((x-x*)/l_x)^2);  target_state=[theta*, x*], lengthscales=[l_theta, l_x]."""

    def __init__(self, target_state, lengthscales, angle_index, pos_index):
        super().__init__()
        self.target_state, self.lengthscales = _np(target_state).reshape(-1), _np(lengthscales).reshape(-1)
        self.angle_index, self.pos_index = int(angle_index), int(pos_index)

    def _pack(self, states, trial_index=None):
        return ops.PackedCost("cartpole", states.shape[2], states.device, target_state=self.target_state, lengthscales=self.lengthscales,
                              angle_index=self.angle_index, pos_index=self.pos_index)


class Expected_saturated_distance_from_trajectory(_HipExpectedCost):
    """1 - exp(-sum_i ((x_i - x*_{t,i}) / l_i)^2) over ``used_indeces``; target_traj must have one row per time step.
    ``flg_var_lengthscales``: ``lengthscales[trial_index]`` is the lengthscale vector of that trial (Cost_function.py:136-141)."""

    def __init__(self, target_traj, lengthscales, flg_var_lengthscales=False, used_indeces=None):
        super().__init__()
        self.flg_var_lengthscales = bool(flg_var_lengthscales)  # (per-trial lengthscales: packed_for keeps one descriptor per trial index)
        self.target_traj = _np(target_traj)
        self.lengthscales = [_np(l).reshape(-1) for l in lengthscales] if self.flg_var_lengthscales else _np(lengthscales).reshape(-1)
        self.used_indeces = None if used_indeces is None else [int(i) for i in used_indeces]

    def _pack(self, states, trial_index=None):
        ls = self.lengthscales[int(trial_index)] if self.flg_var_lengthscales else self.lengthscales
        return ops.PackedCost("traj", states.shape[2], states.device, target_traj=self.target_traj, lengthscales=ls, used=self.used_indeces)


# ---- the two costs as plain functions (Cost_function.py:124-147, 170-182) -----------------------------------------------
# What a user hands to the generic ``Expected_cost(cost_function=...)``: ordinary differentiable torch ops on the GPU (user-code
# path; the classes above run the same formulas in the HIP cost kernels).
def saturated_distance_from_trajectory(states_sequence, inputs_sequence, trial_index, target_traj, lengthscales, flg_var_lengthscales,
                                       used_indeces):
    """1 - exp(-sum_i ((x_i - x*_{t,i}) / l_i)^2) over ``used_indeces`` (None: every state); ``flg_var_lengthscales``:
    ``lengthscales[trial_index]`` is the vector of that trial.  [T,M,S] -> [T,M]."""
    if used_indeces is None:
        used_indeces = list(range(states_sequence.shape[2]))
    tt = torch.as_tensor(target_traj, dtype=states_sequence.dtype, device=states_sequence.device)
    targets = tt.reshape(tt.shape[0], 1, -1).expand(states_sequence.shape)
    ls = lengthscales[trial_index] if flg_var_lengthscales else lengthscales
    ls = torch.as_tensor(ls, dtype=states_sequence.dtype, device=states_sequence.device)
    d = (states_sequence[:, :, used_indeces] - targets[:, :, used_indeces]) / ls
    return 1 - torch.exp(-(d * d).sum(2))


def cart_pole_cost(states_sequence, inputs_sequence, trial_index, target_state, lengthscales, angle_index, pos_index):
    """1 - exp(-((|theta| - theta*)/l_theta)^2 - ((x - x*)/l_x)^2);  target_state = [theta*, x*], lengthscales = [l_theta, l_x]."""
    x = states_sequence[:, :, pos_index]
    theta = states_sequence[:, :, angle_index]
    return 1 - torch.exp(-(((torch.abs(theta) - target_state[0]) / lengthscales[0]) ** 2) - ((x - target_state[1]) / lengthscales[1]) ** 2)


# ---- simple torch-level variants (Cost_function.py:39-101) -------------------------------------------------------------
def distance_from_target(states_sequence, inputs_sequence, trial_index, target_state, lengthscales, active_dims):
    d = (states_sequence[:, :, active_dims] - target_state) / lengthscales
    return (d * d).sum(2)


def saturated_distance_from_target(states_sequence, inputs_sequence, trial_index, target_state, lengthscales, active_dims):
    return 1 - torch.exp(-distance_from_target(states_sequence, inputs_sequence, trial_index, target_state, lengthscales, active_dims))


class _TargetStateCost(_HipExpectedCost):
    """A cost over the scaled distance from ONE target state, d = sum_i ((x[active_dims[i]] - x*_i) / l_i)^2.  On float64 GPU states it
    runs in the HIP cost kernels (ops.PackedCost("target")); everything else the torch formula accepts -- K target rows [K, n] (the
    reference then sums K per-target stds, which the kernels' [T][2] moments do not hold), CPU tensors, another dtype, parameters that
    require grad, more than MCP_MAX_STATE indices -- is evaluated by ``cost_function`` through ``Expected_cost``, call by call."""

    _saturate = True
    _torch_cost = None

    def __init__(self, target_state, lengthscales, active_dims):
        super().__init__()
        f = type(self)._torch_cost
        self.cost_function = lambda x, u, k: f(x, u, k, target_state, lengthscales, active_dims)
        self.target_state, self.lengthscales, self.active_dims = target_state, lengthscales, active_dims
        self._act = self._one_target(target_state, lengthscales, active_dims)
        if self._act is None:
            self.from_sums = Expected_cost.from_sums  # (this instance never leaves the torch path)

    @staticmethod
    def _one_target(target_state, lengthscales, active_dims):
        """The active dims as ints when the descriptor fits the kernels (one target row, one lengthscale per index), else None."""
        try:
            act = [int(i) for i in np.asarray(active_dims).reshape(-1)]
        except (TypeError, ValueError):  # (a slice, a mask: torch indexing takes them, the kernels' index list does not)
            return None
        if np.asarray(active_dims).dtype == bool or not 1 <= len(act) <= ops.abi.MAX_STATE:
            return None
        for v in (target_state, lengthscales):
            if isinstance(v, torch.Tensor) and v.requires_grad:
                return None
        tg = target_state if isinstance(target_state, torch.Tensor) else np.asarray(target_state)
        one_row = tg.ndim == 1 or (tg.ndim == 2 and tg.shape[0] == 1)
        if not one_row or tg.shape[-1] != len(act) or ops._count(lengthscales) != len(act):
            return None
        return act

    def runs_on_kernels(self, states=None):
        if self._act is None:
            return False
        if states is None:
            return True
        S = states.shape[-1]
        return (states.is_cuda and states.dtype == torch.float64 and states.dim() == 3 and S <= ops.abi.MAX_STATE
                and all(-S <= i < S for i in self._act))

    def _pack(self, states, trial_index=None):
        S = states.shape[2]
        return ops.PackedCost("target", S, states.device, target_state=_np(self.target_state), lengthscales=_np(self.lengthscales),
                              active_dims=[i % S for i in self._act], saturate=self._saturate)

    @staticmethod
    def from_sums(sums, n_total, shift=None, mean_out=None):
        # (the sums of either path have one meaning; they are pooled where local_moments left them)
        if sums.is_cuda and sums.dtype == torch.float64:
            return _HipExpectedCost.from_sums(sums, n_total, shift, mean_out)
        return Expected_cost.from_sums(sums, n_total, shift, mean_out)


class Expected_distance(_TargetStateCost):
    """sum_i ((x_i - x*_i) / l_i)^2 over ``active_dims`` (Cost_function.py:39-63)."""

    _saturate = False
    _torch_cost = staticmethod(distance_from_target)


class Expected_saturated_distance(_TargetStateCost):
    """1 - exp(-sum_i ((x_i - x*_i) / l_i)^2) over ``active_dims`` (Cost_function.py:66-101)."""

    _saturate = True
    _torch_cost = staticmethod(saturated_distance_from_target)


# ---- control-effort and input-rate terms (the project's own extension: the reference's cost functions ignore inputs_sequence) -----------
def input_distance(inputs_sequence, lengthscales=None, rate_lengthscales=None, target_input=None, input_indices=None):
    """(d_u, d_r), each [T,M], over the input columns ``input_indices`` (None: every input):
    d_u = sum_i ((u_t,i - u*_i) / l_i)^2 (zeros without ``lengthscales``; ``target_input`` None: u* = 0) and
    d_r = sum_i ((u_t,i - u_t-1,i) / r_i)^2 for t >= 1, 0 at t = 0 (zeros without ``rate_lengthscales``).  Plain differentiable torch ops
    in the difference form, like distance_from_target."""
    u = inputs_sequence if input_indices is None else inputs_sequence[:, :, input_indices]

    def as_t(v):
        return torch.as_tensor(v, dtype=u.dtype, device=u.device).reshape(-1)

    zero = torch.zeros(u.shape[0], u.shape[1], dtype=u.dtype, device=u.device)
    d_u, d_r = zero, zero
    if lengthscales is not None:
        d = (u if target_input is None else u - as_t(target_input)) / as_t(lengthscales)
        d_u = (d * d).sum(2)
    if rate_lengthscales is not None:
        d = (u[1:] - u[:-1]) / as_t(rate_lengthscales)
        d_r = torch.cat([zero[:1], (d * d).sum(2)])
    return d_u, d_r


class Input_penalty(_HipExpectedCost):
    """A state cost of this module with a control-effort term d_u and an input-rate term d_r (``input_distance``) on the inputs the policy
    applied: ``state_cost`` is an instance of Cart_pole_cost, Expected_saturated_distance_from_trajectory, Expected_distance or
    Expected_saturated_distance; with f(d) = 1 - exp(-d) (f(d) = d for Expected_distance) and d_x its scaled state distance,

        joint=False:  c = f(d_x) + d_u + d_r      (the penalty stays active where the state cost saturates)
        joint=True:   c = f(d_x + d_u + d_r)      (one saturated distance over states and inputs)

    ``lengthscales`` l_i switch the effort term on, ``rate_lengthscales`` r_i the rate term (at least one); ``target_input`` u* (None: 0);
    ``input_indices`` (None: every input).  On float64 GPU states and inputs [T,M,U <= MCP_MAX_INPUT] it runs in the HIP cost kernels
    (mcp_cost_u_fwd / _bwd: the three-launch cost, recordable attempts, the sharded step's sums); everything else -- CPU tensors, another
    dtype, trainable scales, a state cost that itself keeps its torch path -- evaluates ``cost_function``, the torch formula of the whole
    cost, through ``Expected_cost``, call by call."""

    def __init__(self, state_cost, lengthscales=None, rate_lengthscales=None, target_input=None, input_indices=None, joint=False):
        super().__init__()
        if not isinstance(state_cost, (Cart_pole_cost, Expected_saturated_distance_from_trajectory, _TargetStateCost)):
            raise TypeError("Input_penalty: state_cost must be one of this module's kernel costs (got %s)" % type(state_cost).__name__)
        if lengthscales is None and rate_lengthscales is None:
            raise ValueError("Input_penalty: lengthscales (effort term) or rate_lengthscales (rate term) must be given")
        self.state_cost, self.joint = state_cost, bool(joint)
        self.lengthscales, self.rate_lengthscales, self.target_input = lengthscales, rate_lengthscales, target_input
        self.input_indices = None if input_indices is None else [int(i) for i in np.asarray(input_indices).reshape(-1)]
        self._trainable = any(isinstance(v, torch.Tensor) and v.requires_grad for v in (lengthscales, rate_lengthscales, target_input))
        self._in_packs = {}  # the inputs descriptor, one per (U, device)
        self.cost_function = self._torch_cost

    def _torch_cost(self, states_sequence, inputs_sequence, trial_index):
        """The whole cost [T,M] as torch ops, composed from the module's plain functions."""
        sc, x, u, k = self.state_cost, states_sequence, inputs_sequence, trial_index
        d_u, d_r = input_distance(u, self.lengthscales, self.rate_lengthscales, self.target_input, self.input_indices)
        if isinstance(sc, _TargetStateCost):
            d_x = distance_from_target(x, u, k, sc.target_state, sc.lengthscales, sc.active_dims)
            if not sc._saturate:
                return d_x + d_u + d_r  # (both modes coincide for the plain distance)
            if self.joint:
                return 1 - torch.exp(-(d_x + d_u + d_r))
            return saturated_distance_from_target(x, u, k, sc.target_state, sc.lengthscales, sc.active_dims) + d_u + d_r
        if isinstance(sc, Cart_pole_cost):
            f_x = cart_pole_cost(x, u, k, sc.target_state, sc.lengthscales, sc.angle_index, sc.pos_index)
        else:
            f_x = saturated_distance_from_trajectory(x, u, k, sc.target_traj, sc.lengthscales, sc.flg_var_lengthscales, sc.used_indeces)
        if self.joint:  # (these two plain functions return 1 - exp(-d_x): 1 - exp(-(d_x + d_u + d_r)) = 1 - (1 - f_x) exp(-(d_u + d_r)))
            return 1 - (1 - f_x) * torch.exp(-(d_u + d_r))
        return f_x + d_u + d_r

    def runs_on_kernels(self, states=None):
        if self._trainable or not self.state_cost.runs_on_kernels(states):
            return False
        return states is None or (states.is_cuda and states.dtype == torch.float64 and states.dim() == 3)

    def _inputs_fit(self, states, inputs):
        if not isinstance(inputs, torch.Tensor) or inputs.dim() != 3:
            return False
        U = inputs.shape[2]
        return (inputs.is_cuda and inputs.dtype == torch.float64 and inputs.device == states.device and inputs.shape[:2] == states.shape[:2]
                and 1 <= U <= ops.abi.MAX_INPUT and (self.input_indices is None or all(-U <= i < U for i in self.input_indices)))

    def packed_for(self, states, trial_index=None):
        self._packed = self.state_cost.packed_for(states, trial_index)  # (the state cost keeps its own per-trial descriptors)
        return self._packed

    def inputs_packed_for(self, inputs):
        U = inputs.shape[2]
        key = (U, inputs.device)
        if key not in self._in_packs:
            idx = None if self.input_indices is None else [i % U for i in self.input_indices]
            self._in_packs[key] = ops.PackedCostInputs(U, inputs.device, idx, self.lengthscales, self.rate_lengthscales, self.target_input, self.joint)
        return self._in_packs[key]

    def forward(self, states_sequence, inputs_sequence=None, trial_index=None, group=None, counts=None):
        if not (self.runs_on_kernels(states_sequence) and self._inputs_fit(states_sequence, inputs_sequence)):
            return Expected_cost.forward(self, states_sequence, inputs_sequence, trial_index, group, counts)
        return ops.expected_cost(self.packed_for(states_sequence, trial_index), states_sequence, group, counts, inputs_sequence,
                                 self.inputs_packed_for(inputs_sequence))

    def local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift=None, sums_out=None):
        if not (self.runs_on_kernels(states_sequence) and self._inputs_fit(states_sequence, inputs_sequence)):
            return Expected_cost.local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift, sums_out)
        return ops.local_cost(self.packed_for(states_sequence, trial_index), states_sequence, m_total, shift, sums_out, inputs_sequence,
                              self.inputs_packed_for(inputs_sequence))

    from_sums = staticmethod(_TargetStateCost.from_sums)  # (the sums of either path have one meaning: pooled where local_moments left them)


# ---- time weights and risk sensitivity (the project's own extension: the reference minimises sum_t mean_m c and prints sum_t std_m c) --------
class Cost_shaping(_HipExpectedCost):
    """One of this module's kernel costs (Cart_pole_cost, Expected_saturated_distance_from_trajectory, Expected_distance,
    Expected_saturated_distance) or an Input_penalty, under a time-weighted, risk-sensitive objective.  With mu_t / sigma_t the mean / unbiased
    std of its per-particle costs c_tm over the n pooled particles at step t:

        J = sum_t w_t (mu_t + risk sigma_t)    first output: what is minimised (risk > 0 cautious, risk < 0 uncertainty-seeking)
        S = sum_t w_t sigma_t                  second output: the monitor, no gradient
        dJ/dc_tm = w_t [1/n + risk (c_tm - mu_t) / ((n - 1) sigma_t)]

    ``time_weights`` (at least T entries, the first T are used; >= 0, finite, not all zero), ``discount`` gamma in (0, 1] (w_t = gamma^t), or
    the product of both; ``risk`` any finite real (risk != 0 needs two particles or more: ValueError).  Unlike the reference's monitor the
    sigma term IS differentiated.  A row whose particles all have the same cost (sigma_t = 0: t = 0 with a zero-variance x0) keeps the factor
    w_t / n -- its sigma term is dropped from the gradient, where autograd through torch.std gives NaN: a stated departure.

    Where the wrapped cost runs on the HIP cost kernels it stays there: three launches (forward, rows + objective, backward), recordable
    attempts, the sharded step's sums.  CPU tensors, another dtype, a wrapped cost that keeps its torch path, a ``time_weights`` tensor that
    requires grad: the same formula as torch ops on the wrapped cost's torch formula.  With no option set it is the wrapped cost, launch for
    launch.  A sharded step with risk != 0 makes one additional small all-reduce (``local_moments(..., reducer=)``: the gradient needs the pooled
    rows of the current step); with risk == 0 the step keeps its single one."""

    def __init__(self, cost, time_weights=None, discount=None, risk=0.0):
        super().__init__()
        if not isinstance(cost, (Cart_pole_cost, Expected_saturated_distance_from_trajectory, _TargetStateCost, Input_penalty)):
            raise TypeError("Cost_shaping: cost must be one of this module's kernel costs or an Input_penalty (got %s)" % type(cost).__name__)
        self.cost, self.time_weights, self.discount, self.risk = cost, time_weights, discount, float(risk)
        if not np.isfinite(self.risk):
            raise ValueError("Cost_shaping: risk must be finite (%r)" % (risk,))
        n_w = 1 if time_weights is None else ops._count(time_weights)
        ops.objective_weights(n_w, time_weights, discount)  # (the values, checked once over every entry given; per T again when packed)
        self._trainable = isinstance(time_weights, torch.Tensor) and time_weights.requires_grad
        self._plain = time_weights is None and discount is None and self.risk == 0.0
        self._objectives = {}  # the objective's descriptor, one per (T, device)
        self.cost_function = self._torch_cost_of(cost)

    needs_pooled_rows = property(lambda self: self.risk != 0.0)  # (a sharded step then hands local_moments its reducer)

    @staticmethod
    def _torch_cost_of(cost):
        """The per-particle costs [T,M] of the wrapped cost as torch ops."""
        if isinstance(cost, Cart_pole_cost):
            return lambda x, u, k: cart_pole_cost(x, u, k, cost.target_state, cost.lengthscales, cost.angle_index, cost.pos_index)
        if isinstance(cost, Expected_saturated_distance_from_trajectory):
            return lambda x, u, k: saturated_distance_from_trajectory(x, u, k, cost.target_traj, cost.lengthscales, cost.flg_var_lengthscales,
                                                                      cost.used_indeces)
        return cost.cost_function

    # -- the kernels ----------------------------------------------------------------------------------------------------------------------
    def runs_on_kernels(self, states=None):
        if self._trainable or not self.cost.runs_on_kernels(states):
            return False
        return states is None or (states.is_cuda and states.dtype == torch.float64 and states.dim() == 3)

    def _on_kernels(self, states, inputs):
        if not self.runs_on_kernels(states):
            return False
        return not isinstance(self.cost, Input_penalty) or self.cost._inputs_fit(states, inputs)

    def packed_for(self, states, trial_index=None):
        self._packed = self.cost.packed_for(states, trial_index)
        return self._packed

    def inputs_packed_for(self, inputs):
        return self.cost.inputs_packed_for(inputs)

    def objective_for(self, states):
        return None if self._plain else self._objective(states.shape[0], states.device)

    def _objective(self, T, device):
        key = (int(T), device)
        if key not in self._objectives:
            self._objectives[key] = ops.PackedObjective(T, device, self.time_weights, self.discount, self.risk)
        return self._objectives[key]

    def _kernel_args(self, states, inputs, trial_index):
        cin = self.inputs_packed_for(inputs) if isinstance(self.cost, Input_penalty) else None
        return self.packed_for(states, trial_index), (None if cin is None else inputs), cin

    def forward(self, states_sequence, inputs_sequence=None, trial_index=None, group=None, counts=None):
        if self._plain:
            return self.cost(states_sequence, inputs_sequence, trial_index, group, counts)
        if not self._on_kernels(states_sequence, inputs_sequence):
            return self._torch_forward(states_sequence, inputs_sequence, trial_index, group, counts)
        pc, inp, cin = self._kernel_args(states_sequence, inputs_sequence, trial_index)
        return ops.expected_cost(pc, states_sequence, group, counts, inp, cin, self.objective_for(states_sequence))

    def local_moments(self, states_sequence, inputs_sequence, trial_index, m_total, shift=None, sums_out=None, reducer=None):
        if self._plain:
            return self.cost.local_moments(states_sequence, inputs_sequence, trial_index, m_total, shift, sums_out)
        if not self._on_kernels(states_sequence, inputs_sequence):
            return self._torch_local_moments(states_sequence, inputs_sequence, trial_index, m_total, shift, sums_out, reducer)
        pc, inp, cin = self._kernel_args(states_sequence, inputs_sequence, trial_index)
        return ops.local_cost(pc, states_sequence, m_total, shift, sums_out, inp, cin, self.objective_for(states_sequence), reducer)

    def from_sums(self, sums, n_total, shift=None, mean_out=None):
        """(J, S) of the pooled swarm from the all-reduced sums (an instance method: the weights are the object's)."""
        if self._plain:
            return self.cost.from_sums(sums, n_total, shift, mean_out)
        T = sums.numel() // 2
        if sums.is_cuda and sums.dtype == torch.float64 and not self._trainable:
            objective = self._objective(T, sums.device)
            objective.check_particles(n_total)
            out = ops.cost_from_sums(sums, n_total, shift, mean_out, objective)
            return out[0], out[1]
        a, b = sums[:T], sums[T:]
        mean = a / n_total + (0.0 if shift is None else shift)
        if mean_out is not None:
            mean_out.copy_(mean)
        self._check_particles(n_total)
        sd = torch.sqrt(torch.clamp(b - a * a / n_total, min=0.0) / (n_total - 1))
        w = self._weights(T, sums)
        j = mean + self.risk * sd if self.risk != 0.0 else mean
        return (torch.sum(j), torch.sum(sd)) if w is None else (torch.sum(w * j), torch.sum(w.detach() * sd))

    # -- the torch path -------------------------------------------------------------------------------------------------------------------
    def _check_particles(self, n):
        if self.risk != 0.0 and n < 2:
            raise ValueError("Cost_shaping: the std term (risk = %g) needs at least two particles (%d given)" % (self.risk, n))

    def _weights(self, T, like):
        """w [T] on the device and in the dtype of ``like`` (None: ones); a trainable ``time_weights`` stays in the graph."""
        if self.time_weights is None and self.discount is None:
            return None
        host = ops.objective_weights(T, self.time_weights, self.discount)  # (the checks)
        if not self._trainable:
            return torch.as_tensor(host, dtype=like.dtype, device=like.device)
        w = self.time_weights.reshape(-1)[:T].to(dtype=like.dtype, device=like.device)
        if self.discount is not None:
            w = w * torch.as_tensor(float(self.discount) ** np.arange(T), dtype=like.dtype, device=like.device)
        return w

    def _shaped(self, costs, mean, m2, n):
        """(J, S) from the per-particle costs and the (detached) pooled mean and centred sum of squares per step: the value is
        sum_t w_t (mean_t + risk sd_t), the gradient that of sum_tm fac_tm c_tm with fac the hand form of the class docstring (rows of zero spread
        without their sigma term).  What a rank of several holds is its part of the gradient; the value is the pooled one."""
        T = costs.shape[0]
        w = self._weights(T, costs)
        sd = torch.sqrt(m2 / (n - 1)) if n > 1 else torch.full_like(m2, float("nan"))
        fac = torch.full_like(costs.detach(), 1.0 / n)
        j = mean
        if self.risk != 0.0:
            spread = sd > 0
            safe = torch.where(spread, sd, torch.ones_like(sd))
            fac = fac + torch.where(spread, self.risk / ((n - 1) * safe), torch.zeros_like(sd))[:, None] * (costs.detach() - mean[:, None])
            j = mean + self.risk * sd
        if w is not None:
            fac, j, s = fac * w[:, None], w * j, w.detach() * sd
        else:
            s = sd
        part = (fac * costs).sum()
        return part, part + (torch.sum(j) - part).detach(), torch.sum(s)

    def _torch_forward(self, states, inputs, trial_index, group, counts):
        costs = self.cost_function(states, inputs, trial_index)
        cd = costs.detach()
        if group is None:
            n = costs.shape[1]
            self._check_particles(n)
            mean = cd.mean(1)
            m2 = ((cd - mean[:, None]) ** 2).sum(1)
            m2 = torch.where(cd.amax(1) > cd.amin(1), m2, torch.zeros_like(m2))  # (identical costs: exactly 0, whatever the mean rounded to)
        else:
            import torch.distributed as dist

            if counts is None:
                nt = torch.tensor([float(costs.shape[1])], dtype=costs.dtype, device=costs.device)
                dist.all_reduce(nt, group=group)
                n = int(nt.item())
            else:
                n = sum(int(c) for c in counts)
            self._check_particles(n)
            s1 = cd.sum(1)
            dist.all_reduce(s1, group=group)
            mean = s1 / n
            m2 = ((cd - mean[:, None]) ** 2).sum(1)
            dist.all_reduce(m2, group=group)
        _, J, S = self._shaped(costs, mean, m2, n)
        return J, S

    def _torch_local_moments(self, states, inputs, trial_index, m_total, shift, sums_out, reducer):
        costs = self.cost_function(states, inputs, trial_index)
        T, n = costs.shape[0], int(m_total)
        self._check_particles(n)
        d = costs.detach() - (0.0 if shift is None else shift.reshape(-1, 1))
        sums = torch.cat([d.sum(1), (d * d).sum(1)])
        if sums_out is not None:
            sums_out.copy_(sums)
            sums = sums_out
        if self.risk == 0.0:  # (the factor w_t / n needs nothing from the other ranks)
            mean, m2 = torch.zeros(T, dtype=costs.dtype, device=costs.device), torch.ones(T, dtype=costs.dtype, device=costs.device)
        else:
            if reducer is None:
                raise ValueError("Cost_shaping: a sharded cost with risk != 0 needs the step's reducer for the pooled rows")
            # one additional small all-reduce: the pooled rows of THIS step.  A NaN on another rank makes them, and this rank's gradient, NaN:
            # harmless -- the pooled cost is then non-finite on every rank and the attempt is discarded, as without the std term
            pooled = reducer.allreduce_(sums.detach().clone())
            a, b = pooled[:T], pooled[T:]
            mean = a / n + (0.0 if shift is None else shift)
            m2 = torch.clamp(b - a * a / n, min=0.0)
        share, _, _ = self._shaped(costs, mean, m2, n)
        return share, sums
