"""MC-PILCO driver on the HIP path -- drop-in for ``policy_learning/MC_PILCO.py`` (class ``MC_PILCO``).

  apply_policy       MC_PILCO.py:615-674   particle rollout  -> ONE fused HIP launch (mcp_rollout_fwd)
  reinforce_policy   MC_PILCO.py:375-613   optimizer loop: rollout, expected cost, backward (fused reverse-time adjoint,
                                           mcp_rollout_bwd), optimizer step, cost monitors, lr / dropout annealing, NaN retries
  reinforce          MC_PILCO.py:89-258    trial loop and ``log.pkl`` bookkeeping (same keys)
  rollout            MC_PILCO.py:347-373   mean-only single-trajectory prediction

Constructor injection is the plug-in mechanism, as in the reference: model / policy / cost classes and their kwargs.
Additions (all optional): ``noise_mode`` -- "philox" (in-kernel generator, default) or "reference" (noise drawn on the
CPU with the reference's torch calls in its order, for seed-for-seed parity); ``shard_particles(group)`` -- split the
particles over the ranks of a torch.distributed group (ONE all-reduce of [gradients | cost sums | flags] per optimizer
step; every rank then applies the identical update).
``MC_PILCO4PMS`` (MC_PILCO.py:755-958, partially measurable systems): the measurement filter between particles and policy is
part of the fused rollout kernels (``mcp_meas``); a step-wise path on the posterior / policy operators remains as fallback.
Out of scope: MC_PILCO_Experiment, MuJoCo environments.
"""
import copy
import pickle as pkl
import time
from functools import partial

import numpy as np
import torch
from torch.distributions.multivariate_normal import MultivariateNormal
from torch.distributions.uniform import Uniform

from mc_pilco_amd import hipabi, ops, sharding
from mc_pilco_amd.policy_learning import Cost_function as _Cost
from mc_pilco_amd.policy_learning import Policy as _Policy
from mc_pilco_amd.policy_learning import opt_loop
from mc_pilco_amd.simulation_class import model as _sim


def _has_fused_layout(ml):
    """The model has a fused-rollout layout (``packed()``): the speed-integration models and the delta-state models with one GP per
    state.  A model object without ``has_fused_layout`` keeps the older test, a speed-integration interface."""
    f = getattr(ml, "has_fused_layout", None)
    return bool(f()) if callable(f) else hasattr(ml, "vel_indeces")


def reference_draws(m_total, T, G, dtype, *, B=0, p_drop=0.0, n_pos=0):
    """The noise of one rollout of the WHOLE swarm, drawn from the CPU generator with the reference's torch calls in the reference's order
    (what seed-for-seed parity rests on): mask_0 if p_drop > 0, then for t = 1..T-1: eps_t, the position noise of a simulated
    measurement if n_pos > 0 (MC_PILCO4PMS), mask_t if p_drop > 0.
    Returns eps [T-1, Mt, G], masks [T, Mt, B] uint8 or None, pos_noise [T-1, Mt, n_pos] or None."""
    Mt, p = int(m_total), float(p_drop)
    mask = lambda: torch.empty(Mt, 1, B, dtype=dtype).bernoulli_(1 - p).reshape(Mt, B)
    masks = [mask()] if p > 0 else None
    eps, pos_noise = [], []
    for _ in range(1, T):
        eps.append(torch.empty(Mt, G, dtype=dtype).normal_())
        if n_pos:
            pos_noise.append(torch.randn(Mt, n_pos, dtype=dtype))
        if p > 0:
            masks.append(mask())
    stack = lambda l, w: torch.stack(l) if l else torch.zeros(0, Mt, w, dtype=dtype)
    return stack(eps, G), None if masks is None else torch.stack(masks).to(torch.uint8), stack(pos_noise, n_pos) if n_pos else None


class MC_PILCO(torch.nn.Module):
    def __init__(self, T_sampling, state_dim, input_dim, f_sim, f_model_learning, model_learning_par, f_rand_exploration_policy,
                 rand_exploration_policy_par, f_control_policy, control_policy_par, f_cost_function, cost_function_par, std_meas_noise=None,
                 log_path=None, dtype=torch.float64, device=torch.device("cuda")):
        super().__init__()
        self.T_sampling = T_sampling
        self.dtype = dtype
        self.device = torch.device(device)
        self.state_dim = state_dim
        self.input_dim = input_dim
        print("\n\nGet the system...")
        self.system = _sim.Model(f_sim)
        self.std_meas_noise = np.zeros(state_dim) if std_meas_noise is None else std_meas_noise
        print("\n\nGet the learning object...")
        self.model_learning = f_model_learning(**model_learning_par)
        print("\n\nGet the exploration policy...")
        self.rand_exploration_policy = f_rand_exploration_policy(**rand_exploration_policy_par)
        print("\n\nGet the control policy...")
        self.control_policy = f_control_policy(**control_policy_par)
        print("\n\nGet the cost function...")
        self.cost_function = f_cost_function(**cost_function_par)
        self.state_samples_history = []
        self.input_samples_history = []
        self.noiseless_states_history = []
        self.num_data_collection = 0
        self.log_path = log_path
        if self.log_path is not None:
            self.log_dict = {}
        # HIP-path options
        self.noise_mode = "philox"
        self.seed = 0
        self._rollout_calls = 0
        self.fused_open_loop = True       # MC_PILCO.rollout's mean chain as one fused launch (False: the step loop on get_next_state)
        self.last_open_loop_fused = False  # what the last rollout() ran
        self.fused_feedback = True        # apply_policy with a PD_controller or an MLP_policy as one fused launch (False: the step loop on get_next_state)
        self.last_feedback_fused = False  # what the last apply_policy() ran for such a policy
        self.fused_step = False           # the generic loop of apply_policy steps the model with ONE launch per step (see _step_fused); False: get_next_state
        self.last_step_fused = False      # what the last apply_policy() ran in its generic loop
        self.dist_group = None
        self.last_status = None
        self.gp_sharding = True    # cleared for good once a GP-sharded launch reports MCP_STATUS_SYNC (co-residency was not there)
        self._reducer = None       # sharding.StepReducer: the one all-reduce of a sharded optimizer step
        self._step_msgs = {}       # sharding.StepMessage by (with gradients?): the persistent flat message of that all-reduce
        self._cost_shift = None    # previous step's pooled per-time-step mean cost (the shift of the summable cost moments)
        self.pipeline_depth = 1    # reinforce_policy reads an attempt's outcome this many attempts late (0: at once); see there
        self.capture_attempts = False  # True: reinforce_policy records an attempt into a HIP graph and replays it (pipelined loop only); see there
        self._call_dev = None      # device int64 [1]: the rollout counter of replayed attempts (mcp_noise.call_dev), None while attempts run eagerly
        self.attempts_replayed = 0  # attempts of the last reinforce_policy that ran as a graph replay (diagnostic)

    # ------------------------------------------------------------------------------------------------------------
    # particle sharding
    # ------------------------------------------------------------------------------------------------------------
    def shard_particles(self, group=None, transport="torch"):
        """Split ``num_particles`` over the ranks of ``group`` (default: the WORLD group).  Per optimizer step the ranks then meet
        in ONE all-reduce (sharding.StepReducer; ``transport`` "torch" = torch.distributed, "abi" = the C ABI's RCCL communicator).
        Every rank must seed torch identically (the launch scripts' ``torch.manual_seed(seed)``): x0 -- and in "reference"
        noise mode eps and the masks -- are drawn for ALL particles on every rank and sliced, so a sharded run simulates
        exactly the particles one GPU would."""
        import torch.distributed as dist

        self.dist_group = dist.group.WORLD if group is None else group
        self._reducer = sharding.StepReducer(self.dist_group, transport)

    def _world(self):
        if self.dist_group is None:
            return 1, 0
        import torch.distributed as dist

        return dist.get_world_size(self.dist_group), dist.get_rank(self.dist_group)

    # ------------------------------------------------------------------------------------------------------------
    # forward simulation of the particles
    # ------------------------------------------------------------------------------------------------------------
    def sample_initial_particles(self, mean, var, flg_uniform, up_bound, low_bound, flg_multi_gauss, num_particles):
        """x_0 ~ uniform / mixture of Gaussians / Gaussian.  In "reference" noise mode the draw is made on the CPU with
        the reference's own distribution calls (bit-exact for a given torch seed)."""
        if self.noise_mode != "reference" and not flg_uniform and not flg_multi_gauss:
            # same distribution as MultivariateNormal(mean, diag(var)) without building M covariance matrices and their Cholesky
            # factors on every optimizer step
            # (two launches per draw -- randn, addcmul -- instead of four: the standard deviations are kept per variance tensor and version)
            mean = mean.to(self.device).reshape(1, -1)
            hit = self.__dict__.get("_x0_std")
            if hit is None or hit[0] is not var or hit[1] != int(var._version):
                hit = self.__dict__["_x0_std"] = (var, int(var._version), torch.sqrt(var.to(self.device).reshape(1, -1)))
            return torch.addcmul(mean, hit[2], torch.randn(num_particles, mean.shape[1], dtype=mean.dtype, device=self.device))
        on = torch.device("cpu") if self.noise_mode == "reference" else self.device
        mean, var = mean.to(on), var.to(on)
        if flg_uniform:
            dist_ = Uniform(low_bound.to(on).repeat(num_particles, 1), up_bound.to(on).repeat(num_particles, 1))
        elif flg_multi_gauss:
            idx = torch.randint(0, mean.shape[0], [num_particles], device=on)
            dist_ = MultivariateNormal(loc=mean[idx, :], covariance_matrix=torch.diag_embed(var[idx, :]))
        else:
            dist_ = MultivariateNormal(loc=mean.repeat(num_particles, 1), covariance_matrix=torch.diag_embed(var.repeat(num_particles, 1)))
        return dist_.rsample().to(self.device)

    def _shard_slice(self, t, dim):
        """This rank's particles of a tensor drawn for the whole swarm (no-op on a single rank)."""
        off, cnt = self._shard
        return t if cnt == t.shape[dim] else t.narrow(dim, off, cnt).contiguous()

    def _rollout_noise(self, T, p_dropout=None, n_pos=0):
        """(NoiseSpec, position noise or None, the dropout probability the policy applies) of the next rollout; the one place that advances
        the rollout counter.  ``p_dropout`` None: a policy without dropout.  "reference" mode: the reference's draws for the WHOLE swarm
        (every rank draws the same numbers from the same seed), sliced to this rank's particles."""
        pol = self.control_policy
        p = float(p_dropout) if p_dropout is not None and getattr(pol, "flg_drop", True) else 0.0
        self._rollout_calls += 1
        if self.noise_mode != "reference":
            return self._philox_noise(), None, p
        B = getattr(pol, "num_basis", None) or getattr(pol, "drop_width", 0)  # a mask row: the basis functions, or an MLP's hidden units
        draws = reference_draws(self._m_total, T, self.model_learning.num_gp, self.dtype, B=B, p_drop=p, n_pos=n_pos)
        eps, masks, pos_noise = (None if t is None else self._shard_slice(t, 1).to(self.device).contiguous() for t in draws)
        return ops.NoiseSpec(eps=eps, masks=masks), pos_noise, p

    def _philox_noise(self):
        """In-kernel noise keyed by (seed, rollout counter, global particle).  While an attempt is being recorded into a graph the counter is the
        device word the graph advances (by-value part 0); the host's ``_rollout_calls`` mirrors it either way."""
        call = self._rollout_calls if self._call_dev is None else 0
        return ops.NoiseSpec(seed=self.seed, call=call, particle_offset=self._shard[0], call_dev=self._call_dev)

    def _begin_rollout(self, particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                       particles_init_low_bound, flg_particles_init_multi_gauss, num_particles, T_control):
        """The set-up every rollout starts with (the arguments of ``apply_policy``): this rank's range of the swarm (``_shard``, ``_m_total``) and
        x0, drawn for the whole swarm and sliced.  Returns (M of this rank, T, x0)."""
        world, rank = self._world()
        self._shard = sharding.shard_range(int(num_particles), world, rank)
        self._m_total = int(num_particles)
        x0 = self.sample_initial_particles(particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                                           particles_init_low_bound, flg_particles_init_multi_gauss, self._m_total)
        return self._shard[1], int(T_control), self._shard_slice(x0, 0)

    def _fused(self, states, inputs, status, feedback=False):
        """Books a fused launch (its status word; whether it ran the PD law) and returns what ``apply_policy`` returns."""
        self.last_status, self.last_feedback_fused = status, feedback
        return states, inputs

    def _fused_rollout(self, x0, T, p_dropout, model_of=None, meas_of=None, n_pos=0):
        """The one place that picks the fused rollout of the control policy: what ``apply_policy`` returns, or None when nothing fuses (then
        nothing was drawn; a feedback policy's ``fusable`` is asked about the packed model, so that may have been packed).  ``model_of()``:
        the packed model to launch on (default: ``packed`` of a model with a fused layout); ``meas_of(pos_noise)``: the MeasSpec of a rollout
        on simulated measurements of ``n_pos`` positions (MC_PILCO4PMS).  ``_rollout_noise`` is called once, on the branch that launches --
        the reference's draw order: (mask_0;) per step eps_t, (position noise,) (mask_t).  Sharded: x0 and the eps buffers are drawn for the
        whole swarm and sliced, Philox counts by global particle; the gradients reach the all-reduce through the parameters' .grad."""
        pol, ml = self.control_policy, self.model_learning
        if not _has_fused_layout(ml):
            return None
        measured = meas_of is not None
        model_of, meas_of = model_of or ml.packed, meas_of or (lambda pos_noise: None)
        if isinstance(pol, _Policy.Sum_of_gaussians):  # (on measurements the kernels carry the filter's states per particle, mcp_meas)
            noise, pos_noise, p = self._rollout_noise(T, p_dropout, n_pos=n_pos)
            return self._fused(*ops.rollout(model_of(), pol.packed(), noise, x0, T, p, meas=meas_of(pos_noise), gp_sharding=self.gp_sharding))
        # the closed loop under the PD law, the time-varying linear law or the tanh MLP: one launch (and one sweep in backward); the eps draws, and for an MLP with
        # dropout (flg_drop) the masks of its hidden units -- the PD law has none
        mlp = isinstance(pol, _Policy.MLP_policy)
        if mlp and measured and int(getattr(pol, "history", 1)) > 1:
            return None  # (an MLP with memory has no fused form on simulated measurements: the step loop, which holds its window)
        op = (ops.rollout_pd if isinstance(pol, _Policy.PD_controller) else ops.rollout_tvl if isinstance(pol, _Policy.TV_linear_controller)
              else ops.rollout_mlp if mlp else None)
        model = model_of() if op is not None and self.fused_feedback else None
        if model is None or not pol.fusable(model, T):
            return None
        noise, pos_noise, p = self._rollout_noise(T, p_dropout if mlp and pol.flg_drop else None, n_pos=n_pos)
        drop = dict(p_drop=p) if p > 0.0 else {}
        return self._fused(*op(model, pol.packed(), noise, x0, T, meas=meas_of(pos_noise), **drop), feedback=True)

    def apply_policy(self, particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                     particles_init_low_bound, flg_particles_init_multi_gauss, num_particles, T_control, p_dropout=0.0):
        """Simulates ``num_particles`` particles for ``T_control`` steps under the control policy.
        Returns states [T,M,S] and inputs [T,M,U] (differentiable w.r.t. the policy parameters)."""
        _, T, x0 = self._begin_rollout(particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                                       particles_init_low_bound, flg_particles_init_multi_gauss, num_particles, T_control)
        pol, ml = self.control_policy, self.model_learning
        self.last_feedback_fused = False  # (reset before every branch: a run under another policy must not leave an earlier True standing)
        self.last_step_fused = False
        out = self._fused_rollout(x0, T, p_dropout)
        if out is not None:
            return out
        # generic (unfused) path: any model / policy object with the reference's step interface
        self.last_status = None  # (no fused launch: the flags of an earlier fused rollout do not describe this one)
        if self._world()[0] > 1:
            # its noise (torch draws inside get_next_state / the policy's dropout) is per LOCAL particle: identically seeded ranks
            # would simulate correlated shards, not the particles one GPU would
            raise NotImplementedError("particle sharding needs the fused rollout (Sum_of_gaussians, PD_controller, TV_linear_controller or MLP_policy policy + a model "
                                      "with a fused layout)")
        step = self._step_fused(T)
        xs = [x0]
        us = [pol(x0, t=0, p_dropout=p_dropout)]
        for t in range(1, T):
            x, _, _ = step(xs[-1], us[-1], t - 1) if step else ml.get_next_state(current_state=xs[-1], current_input=us[-1])
            xs.append(x)
            us.append(pol(x, t=t, p_dropout=p_dropout))
        return torch.stack(xs), torch.stack(us)

    def _step_fused(self, T, n_pos=0):
        """The generic loop's model step as one launch per time step (Model_learning.fused_next_state) when ``fused_step`` is on and the
        model's step is the one its fused layout describes, else None: the loop then calls get_next_state as ever.  The policy is called
        exactly as in the unfused loop.  The noise is the fused rollouts': ``_rollout_noise`` -- Philox by (seed, call, t, particle), or in
        "reference" mode row t of the eps buffer of ``reference_draws`` -- and nothing is drawn from the torch generator for the model.  The
        steps OR their flags into one word, ``last_status``.  Returns step(x, u, t) -> get_next_state's tuple; ``step.pos_noise``: the
        position noise [T-1,M,n_pos] drawn with the eps ("reference" mode with ``n_pos``), else None."""
        f = getattr(self.model_learning, "steps_like_the_packed_model", None)
        if not (self.fused_step and callable(f) and f() and T > 1):
            return None
        noise, pos_noise, _ = self._rollout_noise(T, n_pos=n_pos)
        status = self.last_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last_step_fused = True
        ml, eps = self.model_learning, noise.eps

        def step(x, u, t):
            nz = noise if eps is None else ops.NoiseSpec(eps=eps[t])
            return ml.fused_next_state(current_state=x, current_input=u, t=t, noise=nz, status=status)

        step.pos_noise = pos_noise
        return step

    def _step_flags(self, cost):
        """Device vector [cost is NaN, a GP-sharded launch timed out (MCP_STATUS_SYNC), a predictive variance was <= 0
        (MCP_STATUS_NONPOS_VAR)] of the last fused rollout."""
        st = self.last_status
        if st is None or st.device != cost.device:
            sync = nonpos = torch.zeros((), dtype=torch.bool, device=cost.device)
        else:
            sync = (st.reshape(-1)[0] & hipabi.STATUS_SYNC) != 0
            nonpos = (st.reshape(-1)[0] & hipabi.STATUS_NONPOS_VAR) != 0
        return torch.stack([torch.isnan(cost.detach()).reshape(()), sync.reshape(()), nonpos.reshape(())]).to(self.dtype)

    def _cost_backward(self, states, inputs, trial_index, backward=True, flags_as_vector=True):
        """Expected cost of the rollout and (``backward``) its gradient in the policy parameters' ``.grad``.
        Returns (cost, std, flags): flags is a device vector, > 0 where [the cost is NaN, a hand-off timed out] -- on EVERY rank
        alike, so all ranks take the same retry decision.

        Single process: the reference's two lines, ``cost_function(...)`` and ``cost.backward()`` (MC_PILCO.py:496,522).
        Sharded: each rank forms its share sum_t sum_m c / M_total, runs its own backward sweep (the gradient of the pooled mean
        needs nothing from the other ranks), and then ONE all-reduce sums [gradients | cost sums | flags]."""
        if self.dist_group is None:
            cost, std = self.cost_function(states, inputs, trial_index)
            if backward:
                # queued before anybody looks at the cost; gradients of a NaN rollout are discarded
                cost.backward(retain_graph=False)
            # (flags_as_vector False: the caller hands the rollout's status word and the cost to mcp_policy_step_commit itself)
            return cost, std, (self._step_flags(cost) if flags_as_vector else None)
        T = states.shape[0]
        if self._cost_shift is None or self._cost_shift.numel() != T:
            self._cost_shift = torch.zeros(T, dtype=self.dtype, device=states.device)
        cf = self.cost_function
        params = list(self.control_policy.parameters())
        # the step's message [gradients | cost sums | flags], kept per (policy size, horizon, with / without gradients): the adjoint sweep and
        # the cost kernels write straight into it and the all-reduce runs on it in place (sharding.StepMessage)
        n_grad = sum(q.numel() for q in params if q.requires_grad) if backward else 0
        msg = self._step_msgs.get(bool(backward))
        if msg is None or not msg.fits(n_grad, T, 3, states.device):
            msg = self._step_msgs[bool(backward)] = sharding.StepMessage(n_grad, T, 3, states.device, self.dtype)
        packed = self.control_policy.packed() if (backward and isinstance(self.control_policy, _Policy.Sum_of_gaussians)) else None
        if getattr(cf, "needs_pooled_rows", False):
            # (Cost_shaping with risk != 0: the gradient factor holds the pooled mean / std of THIS step, so the cost makes one additional small
            #  all-reduce of a copy of the 2T sums through the step's reducer before the sweep; the step's message below is unchanged)
            share, sums = cf.local_moments(states, inputs, trial_index, self._m_total, self._cost_shift, sums_out=msg.sums, reducer=self._reducer)
        else:
            share, sums = cf.local_moments(states, inputs, trial_index, self._m_total, self._cost_shift, sums_out=msg.sums)
        if backward:
            if packed is not None and packed.grad_numel() == n_grad:
                packed.grad_flat = msg.grad  # (mcp_rollout_bwd leaves log_ls | centers | weight | bias there: the order of `params`)
            try:
                share.backward(retain_graph=False)
            finally:
                if packed is not None:
                    packed.grad_flat = None
            for q in params:  # a parameter the cost does not reach still takes part in the message (every rank sends the same layout)
                if q.requires_grad and q.grad is None:
                    q.grad = torch.zeros_like(q)
        # one all-reduce; pooled cost / std; a NaN rollout neither poisons the next steps' shift nor goes unnoticed on the other ranks
        # (the message holds the parameters that require grad -- n_grad above --: a frozen tensor, e.g. some of an MLP's six, takes no part even
        # where an earlier step left it a .grad)
        cost, std, flags, self._cost_shift = sharding.finish_step(cf, self._reducer, [q for q in params if q.requires_grad] if backward else [], sums,
                                                                  self._step_flags(share),
                                                                  self._m_total, self._cost_shift, msg=msg)
        return cost, std, flags

    # ------------------------------------------------------------------------------------------------------------
    # policy optimisation
    # ------------------------------------------------------------------------------------------------------------
    def _rollout_failed(self, flags):
        """Reads the step's flags (ONE device->host transfer; warm-up rollout and user code -- the optimizer loop itself reads the
        record of ``mcp_policy_step_commit``).  True when the cost is NaN (data, not an error: MC_PILCO.py:497) or when a GP-sharded
        launch timed out waiting for a partner workgroup; in the second case the GP-sharded launch forms are switched off for this
        object (the device was not giving the grid co-residency -- another process, CU masking), so the repeated step runs on the
        unsharded kernels: never a silently wrong trajectory, never a rank-local raise."""
        nan, sync, nonpos = (float(v) for v in flags.tolist())
        return self._judge_attempt(nan, sync, nonpos)

    def _judge_attempt(self, nan, sync, nonpos):
        if nonpos > 0:
            # The reference samples with Normal(mean, sqrt(var)).rsample() (Model_learning.py:704), whose argument validation raises
            # ValueError on a scale that is not > 0 -- a zero / negative predictive variance is a modelling error there, not a case of
            # the NaN retry, whatever the cost of that rollout turns out to be (sqrt of a negative variance makes it NaN).  The kernels
            # raise this flag for a FINITE variance <= 0 only; a NaN variance (divergence) is MCP_STATUS_NAN, the retry case.  Same on
            # every rank of a sharded run: the flag travels with the step's all-reduce.
            raise ValueError("Expected parameter scale of the particles' sampling distribution to be > 0: a GP's predictive variance was <= 0 "
                             "(MCP_STATUS_NONPOS_VAR)")
        if sync > 0:
            if self.gp_sharding:
                print("\nGP-sharded rollout: a partner workgroup never arrived (MCP_STATUS_SYNC) -- continuing on the unsharded kernels")
            self.gp_sharding = False
            return True
        return nan > 0

    @staticmethod
    def _plain_adam(opt):
        """(lr, beta1, beta2, eps) when ``opt`` is a torch.optim.Adam whose update is the textbook one (what every launch script
        builds: "lambda p, lr : torch.optim.Adam(p, lr)") -- the loop then runs the update itself, guarded on the device
        (mcp_adam_step_guarded), and never has to wait for a step's outcome.  None: any other optimizer; its own ``step()`` is called,
        after the host has seen that the attempt counts."""
        if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
            return None
        g = opt.param_groups[0]
        if (g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False) or g.get("differentiable", False)
                or g.get("decoupled_weight_decay", False) or isinstance(g["lr"], torch.Tensor)):
            return None
        ps = [q for q in g["params"] if q.requires_grad]
        if not ps or len(ps) > 32 or any(q.dtype != torch.float64 or not q.is_cuda or not q.is_contiguous() for q in ps):
            return None
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])

    def reinforce_policy(self, T_control, num_particles, trial_index, particles_initial_state_mean, particles_initial_state_var,
                         flg_particles_init_uniform, particles_init_up_bound, particles_init_low_bound, flg_particles_init_multi_gauss,
                         opt_steps_list, lr_list, f_optimizer, num_step_print=10, policy_reinit_dict=None, p_dropout_list=None,
                         std_cost_filt_order=None, std_cost_filt_cutoff=None, max_std_cost=None, alpha_cost=0.99, alpha_input=0.99,
                         alpha_diff_cost=0.99, lr_reduction_ratio=0.5, lr_min=0.001, p_drop_reduction=0.0, min_diff_cost=0.1,
                         num_min_diff_cost=200, min_step=np.inf):
        """Monte-Carlo policy gradient: at most ``opt_steps_list[trial_index]`` optimizer steps (MC_PILCO.py:375-613).

        One ATTEMPT = rollout + expected cost + adjoint sweep; what the reference then decides on the host from ``torch.isnan(cost)``
        -- does the attempt count, the cost-difference monitors, the lr / exit condition -- is decided on the device by
        ``mcp_policy_step_commit`` (and, for a plain Adam, the update itself by ``mcp_adam_step_guarded``), which leaves a small record
        per attempt.  The host reads that record ``self.pipeline_depth`` attempts late (1: it has already enqueued the next attempt,
        so the GPU never idles while Python catches up; 0: at once -- the mode with host-drawn "reference" noise, with any other
        optimizer and in a particle-sharded run).  A failed attempt needs nothing from the host (the next attempt is the retry);
        where the host must act -- ten failures in a row, the lr / exit condition, the last step -- the device ignores the attempts
        enqueued meanwhile and the host rewinds the noise counters past them: both depths take exactly the same steps."""
        n_steps = opt_steps_list[trial_index]
        sim = dict(particles_initial_state_mean=particles_initial_state_mean, particles_initial_state_var=particles_initial_state_var,
                   flg_particles_init_uniform=flg_particles_init_uniform, flg_particles_init_multi_gauss=flg_particles_init_multi_gauss,
                   particles_init_up_bound=particles_init_up_bound, particles_init_low_bound=particles_init_low_bound,
                   num_particles=num_particles, T_control=int(T_control / self.T_sampling))
        p_drop0 = 0.0 if p_dropout_list is None else p_dropout_list[trial_index]
        if p_dropout_list is not None:
            print("\nDROPOUT ACTIVE:")
            print("p_dropout:", p_drop0)
        make_opt = eval(f_optimizer)  # the reference passes optimizers as strings, e.g. "lambda p, lr : torch.optim.Adam(p, lr)"
        # re-initialisations draw where the rest of the noise is drawn: in "reference" mode on the CPU generator (the reference's stream)
        self.control_policy.draw_device = torch.device("cpu") if self.noise_mode == "reference" else None

        # reference value for the cost-difference monitor (policy re-initialised while the cost is NaN)
        with torch.no_grad():
            for _ in range(10):
                st0, in0 = self.apply_policy(p_dropout=p_drop0, **sim)
                cost0, _, fl0 = self._cost_backward(st0, in0, trial_index, backward=False)
                sharded_before = self.gp_sharding
                if not self._rollout_failed(fl0):
                    break
                if sharded_before and not self.gp_sharding:
                    continue  # a hand-off time-out, not a NaN: same policy, unsharded kernels
                print("\nSE filter initialization: Cost is NaN - reinit the policy")
                self.control_policy.reinit(**policy_reinit_dict)

        sched = opt_loop.HostSchedule(lr_list[trial_index], p_drop0, min_diff_cost, min_step, lr_min, lr_reduction_ratio, p_drop_reduction,
                                      num_min_diff_cost)
        lp = opt_loop.PolicyLoop(self, make_opt, sched, n_steps, cost0, sim, trial_index, alpha_diff_cost)
        self.attempts_replayed = 0
        last, done = self._run_attempts(lp, num_step_print, policy_reinit_dict)
        if lp.graphs.last_flat is not None:  # (the last attempt was a replay: its gradients are where autograd would have left them)
            for q in lp.params:
                g_ = lp.graphs.last_flat.get(id(q))
                q.grad = None if g_ is None else g_.reshape(q.shape)
        lp.graphs.drop()  # (rollouts after this call count by value again; the host's mirror of the counter is current)
        return (lp.state.cost_list[0:done].detach().cpu().numpy(), lp.state.std_list[0:done].detach().cpu().numpy(),
                last.states.detach().cpu().numpy(), last.inputs.detach().cpu().numpy())

    def _run_attempts(self, lp, num_step_print, policy_reinit_dict):
        """Enqueues attempts and reads their records ``lp.depth`` attempts late until the steps are taken or the exit condition holds.
        Returns (the last attempt read, the number of steps taken)."""
        sched = lp.sched
        sched.t_mark = time.time()
        queue, last, done, reinits, leave = [], None, 0, 0, False
        while not leave:
            queue.append(self._enqueue(lp))
            while queue and (len(queue) > lp.depth) and not leave:
                h = queue.pop(0)
                r = opt_loop.read(h)
                k = int(r.step)
                assert r.void == 0.0, "the oldest attempt in flight cannot be void"
                if r.counted == 0.0:
                    self._judge_attempt(r.nan, r.sync, r.nonpos)  # (raises on a non-positive variance; switches GP sharding off after a time-out)
                    print("\nCost is NaN: try sampling again")
                    last = h
                    if r.attempt >= hipabi.OPT_MAX_ATTEMPTS:
                        # ten failed attempts in a row (MC_PILCO.py:573-607): the reference takes the step on the failed cost (its monitors
                        # and messages included) and restarts from a re-initialised policy
                        self._discard(queue)
                        if k % num_step_print == 0:
                            sched.step_print(k, r.cost, float("nan"))
                        if k > sched.min_step:  # (its lr / exit test looks at the window BEFORE this step's ratio: it may still fire; only the
                            win = torch.abs(lp.state.ratio[max(k + 1 - sched.n_win, 0):k + 1])  # messages matter, everything is reset below)
                            if int(torch.sum(win < sched.min_diff)) >= sched.n_win and k + 1 >= sched.n_win:
                                sched.lr_or_exit(k)
                        reinits += 1
                        print("\nCost is NaN: re-initialize control policy [attempt #" + str(reinits) + "]")
                        self.control_policy.reinit(**policy_reinit_dict)
                        lp.state.reset_after_reinit()
                        sched.reset()
                        lp.new_optimizer(same_kind=False)  # (new moments / learning rate / dropout / parameters: what the graphs recorded is gone)
                        done = 0
                    continue
                # the attempt counted: step k was taken
                last, done = h, k + 1
                if lp.adam is None:
                    lp.opt.step()  # (depth 0: the host knows the attempt counted before it updates)
                if k % num_step_print == 0:
                    sched.step_print(k, r.cost, r.abs_ratio)
                if r.pending != 0.0:
                    self._discard(queue)
                    leave = sched.lr_or_exit(k)
                    if not leave:
                        lp.new_optimizer()  # (new moments / learning rate / dropout: what the graphs recorded is gone)
                    lp.state.clear_pending()
                if done >= lp.state.n_steps:
                    self._discard(queue)
                    leave = True
        self._discard(queue)
        return last, done

    def _recordable(self):
        """An attempt of this object can be recorded into a HIP graph (``capture_attempts``; pipelined loop with the guarded Adam only)."""
        pol = self.control_policy
        return (bool(getattr(self, "capture_attempts", False)) and self.device.type == "cuda"
                and type(self).apply_policy is MC_PILCO.apply_policy  # (the measurement-model rollout of MC_PILCO4PMS keeps the eager loop)
                and isinstance(pol, _Policy.Sum_of_gaussians) and getattr(pol, "_unit_scale", False)
                and _has_fused_layout(self.model_learning) and isinstance(self.cost_function, _Cost._HipExpectedCost)
                and self.cost_function.runs_on_kernels())  # (a target-state cost with several target rows keeps its torch path)

    def _attempt(self, lp, rec_row):
        """The reference's lines (MC_PILCO.py:484-525) on the drop-in classes: apply_policy -> cost_function -> cost.backward() -> step."""
        for q in lp.params:
            q.grad = None
        states, inputs = self.apply_policy(p_dropout=lp.sched.p_drop, **lp.sim)
        cost, std, flags = self._cost_backward(states, inputs, lp.trial_index, flags_as_vector=self.dist_group is not None)
        status = None if (flags is not None or self.last_status is None) else self.last_status
        grads = None if lp.adam is None else lp.adam.pointers(None if q.grad is None else q.grad.data_ptr() for q in lp.adam.ps)
        lp.commit(cost, std, flags, status, grads, rec_row)
        return states, inputs, cost, None

    def _attempt_raw(self, lp, rec_row):
        """The same attempt as the operators underneath make it, without the autograd engine (whose stream bookkeeping does not survive a
        stream capture): x0 -> mcp_rollout_fwd -> mcp_cost_fwd / _finalize / _bwd (under a Cost_shaping: / _rows / _bwd_shaped) -> mcp_rollout_bwd -> guarded Adam -> commit.  Identical
        launches with identical arguments, hence identical bits; this is the form that is recorded and replayed."""
        pol = self.control_policy
        self._call_dev.add_(1)
        _, T, x0 = self._begin_rollout(**lp.sim)  # (a recorded attempt runs on one rank: the whole swarm)
        noise, _, p = self._rollout_noise(T, lp.sched.p_drop)
        model, pk = self.model_learning.packed(), pol.packed()
        states, inputs, jac, status = ops.rollout_forward_raw(model, pk, noise, x0, T, p, True, need_jac=True, gp_sharding=self.gp_sharding)
        self.last_status = status
        cf = self.cost_function
        cin = cf.inputs_packed_for(inputs)  # (None: the cost reads the states only -- no inputs gradient, the sweep takes NULL as before)
        cost, std, g_states, g_inputs = ops.expected_cost_raw(cf.packed_for(states, lp.trial_index), states, lp.graphs.one,
                                                              None if cin is None else inputs, cin, want_g_inputs=True,
                                                              objective=cf.objective_for(states))
        g_ls, g_c, g_w, _, g_b = ops.rollout_backward_raw(model, pk, noise, states, inputs, jac, g_states, g_inputs, p)
        by_param = {id(pol.log_lengthscales): g_ls, id(pol.centers): g_c, id(pol.f_linear.weight): g_w}
        if pol.f_linear.bias is not None:
            by_param[id(pol.f_linear.bias)] = g_b
        lp.commit(cost, std, None, status, lp.adam.pointers(by_param[id(q)].data_ptr() for q in lp.adam.ps), rec_row)
        return states, inputs, cost, by_param

    def _enqueue(self, lp):
        """One attempt, start to finish, without a host sync: a graph replay where there is one, else the eager calls."""
        state, graphs = lp.state, lp.graphs
        snap = (self._rollout_calls, torch.cuda.get_rng_state(self.device) if lp.depth > 0 else None)
        slot, gi = state.seq % state.slots, state.seq & 1  # (of the record ring; which of the two graphs)
        state.seq += 1
        ran = graphs.run(gi, lambda row: self._attempt_raw(lp, row), snap)
        if ran is None:
            graphs.eager += 1
            ran = self._attempt(lp, state.rec_dev[slot]), state.rec_dev[slot]
        (states, inputs, cost, graphs.last_flat), rec_src = ran
        state.ring[slot].copy_(rec_src, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return opt_loop.Attempt(states, inputs, cost, state.ring[slot], ev, snap)

    def _discard(self, queue):
        """The attempts enqueued while the device was waiting for the host: the device ignored them; the noise counters go back
        to where the first of them found them, so the run continues exactly as one that never enqueued them."""
        if queue:
            for h in queue:
                r = opt_loop.read(h)
                assert r.void == 1.0 and r.counted == 0.0, "an attempt enqueued past a host decision was not void"
            self._rollout_calls, rng_state = queue[0].snap
            if self._call_dev is not None:
                self._call_dev.fill_(self._rollout_calls)
            if rng_state is not None:
                torch.cuda.set_rng_state(rng_state, self.device)
            queue.clear()

    # ------------------------------------------------------------------------------------------------------------
    # trial loop
    # ------------------------------------------------------------------------------------------------------------
    def _draw_x0(self, initial_state, initial_state_var, random_initial_state, flg_uniform, low, up, flg_multi):
        if not random_initial_state:
            return initial_state
        if flg_uniform:
            return np.random.uniform(low, up)
        if flg_multi:
            k = np.random.randint(initial_state.shape[0])
            return np.random.normal(initial_state[k, :], np.sqrt(initial_state_var[k, :]))
        return np.random.normal(initial_state, np.sqrt(initial_state_var))

    def _save_log(self):
        if self.log_path is not None:
            print("Save log file...")
            pkl.dump(self.log_dict, open(self.log_path + "/log.pkl", "wb"))

    def reinforce(self, initial_state, initial_state_var, T_exploration, T_control, num_trials, model_optimization_opt_list,
                  policy_optimization_dict, num_explorations=1, flg_init_uniform=False, init_up_bound=None, init_low_bound=None,
                  flg_init_multi_gauss=False, random_initial_state=True, loaded_model=False):
        """Alternates model learning, policy optimisation on the learned model, and interaction with the system."""
        x0_args = (initial_state, initial_state_var, random_initial_state, flg_init_uniform, init_low_bound, init_up_bound, flg_init_multi_gauss)
        if not loaded_model:
            print("\n\n\n\n----------------- INITIAL EXPLORATIONS -----------------")
            for k in range(num_explorations):
                print("\nEXPLORATION # " + str(k))
                self.get_data_from_system(initial_state=self._draw_x0(*x0_args), T_exploration=T_exploration, flg_exploration=True, trial_index=k)
            costs, stds, params, pstates, pinputs = [], [], [], [], []
            first = num_explorations - 1
        else:
            costs, stds = self.log_dict["cost_trial_list"], self.log_dict["std_cost_trial_list"]
            params, pstates, pinputs = (self.log_dict["parameters_trial_list"], self.log_dict["particles_states_list"],
                                        self.log_dict["particles_inputs_list"])
            first = len(self.state_samples_history) - 1
        t_dev = lambda a: torch.tensor(a, dtype=self.dtype, device=self.device)
        for trial in range(first, first + num_trials):
            print("\n\n\n\n----------------- TRIAL " + str(trial) + " -----------------")
            print("\n\n----- REINFORCE THE MODEL -----")
            self.model_learning.reinforce_model(optimization_opt_list=model_optimization_opt_list)
            with torch.no_grad():
                if self.log_path is not None:
                    ml = self.model_learning
                    self.log_dict["parameters_gp_" + str(trial)] = [copy.deepcopy(ml.gp_list[k].state_dict()) for k in range(ml.num_gp)]
                    self.log_dict["gp_inputs_" + str(trial)] = ml.gp_inputs
                    self.log_dict["gp_output_list_" + str(trial)] = ml.gp_output_list
                    self.log_dict["state_samples_history"] = self.state_samples_history
                    self.log_dict["input_samples_history"] = self.input_samples_history
                    self.log_dict["noiseless_states_history"] = self.noiseless_states_history
                    self._save_log()
                print("\n\n----- CHECK THE ROLLOUT PERFORMANCE (after model update) -----")
                self.get_rollout_prediction_performance(data_collection_index=trial)
            print("\n\n----- REINFORCE THE POLICY -----")
            self.model_learning.set_eval_mode()
            cost_list, std_list, p_states, p_inputs = self.reinforce_policy(
                T_control=T_control, particles_initial_state_mean=t_dev(initial_state), particles_initial_state_var=t_dev(initial_state_var),
                flg_particles_init_uniform=flg_init_uniform, particles_init_up_bound=t_dev(init_up_bound) if flg_init_uniform else None,
                particles_init_low_bound=t_dev(init_low_bound) if flg_init_uniform else None,
                flg_particles_init_multi_gauss=flg_init_multi_gauss, trial_index=trial, **policy_optimization_dict)
            costs.append(cost_list)
            stds.append(std_list)
            pstates.append(p_states)
            pinputs.append(p_inputs)
            params.append(copy.deepcopy(self.control_policy.state_dict()))
            if self.log_path is not None:
                self.log_dict.update(cost_trial_list=costs, std_cost_trial_list=stds, parameters_trial_list=params, particles_states_list=pstates,
                                     particles_inputs_list=pinputs)
                self._save_log()
            self.model_learning.set_training_mode()
            print("\n\n----- APPLY THE CONTROL POLICY -----")
            self.get_data_from_system(initial_state=self._draw_x0(*x0_args), T_exploration=T_control, flg_exploration=False, trial_index=trial + 1)
            if self.log_path is not None:
                self.log_dict["state_samples_history"] = self.state_samples_history
                self.log_dict["input_samples_history"] = self.input_samples_history
                self.log_dict["noiseless_states_history"] = self.noiseless_states_history
                self._save_log()
        return costs, pstates, pinputs

    # ------------------------------------------------------------------------------------------------------------
    # interaction with the system, mean rollouts, logs
    # ------------------------------------------------------------------------------------------------------------
    def get_data_from_system(self, initial_state, T_exploration, trial_index, flg_exploration=False):
        policy = self.rand_exploration_policy if flg_exploration else self.control_policy
        noisy, inputs, clean = self.system.rollout(s0=initial_state, policy=policy.get_np_policy(), T=T_exploration, dt=self.T_sampling,
                                                   noise=self.std_meas_noise)
        self.state_samples_history.append(noisy)
        self.input_samples_history.append(inputs)
        self.noiseless_states_history.append(clean)
        self.num_data_collection += 1
        self.model_learning.add_data(new_state_samples=noisy, new_input_samples=inputs)

    def _open_loop_fused(self):
        """The open-loop rollouts go through the fused kernel: switched on (``fused_open_loop``) and the model's step is the one its fused
        layout describes (Model_learning.steps_like_the_packed_model)."""
        f = getattr(self.model_learning, "steps_like_the_packed_model", None)
        return bool(self.fused_open_loop) and callable(f) and bool(f())

    def rollout(self, data_collection_index, T_rollout=None, particle_pred=False):
        """Open-loop prediction of one recorded trajectory with the learned model (mean prediction by default).  The mean chain of a model
        with a fused layout is ONE launch (Model_learning.open_loop_rollout); the sampled single path (``particle_pred``) draws from the
        torch generator in the reference's order and keeps the step loop, as do models whose step the layout does not describe."""
        xs = self.state_samples_history[data_collection_index]
        n = xs.shape[0] if T_rollout is None else T_rollout
        self.last_open_loop_fused = bool(not particle_pred and n >= 2 and self._open_loop_fused())
        if self.last_open_loop_fused:
            x0 = torch.tensor(np.asarray(xs[0:1, :]), dtype=self.dtype, device=self.device)
            us = torch.tensor(np.asarray(self.input_samples_history[data_collection_index])[0:n - 1, :], dtype=self.dtype, device=self.device)
            states, status = self.model_learning.open_loop_rollout(x0, us)
            self.last_status = status
            return states[:, 0, :].cpu().numpy()
        us = torch.tensor(self.input_samples_history[data_collection_index], dtype=self.dtype, device=self.device)
        traj = torch.zeros([n, self.state_dim], dtype=self.dtype, device=self.device)
        traj[0:1, :] = torch.tensor(xs[0:1, :], dtype=self.dtype, device=self.device)
        for t in range(1, n):
            traj[t:t + 1, :], _, _ = self.model_learning.get_next_state(current_state=traj[t - 1:t, :], current_input=us[t - 1:t, :],
                                                                         particle_pred=particle_pred)
        return traj.detach().cpu().numpy()

    def rollout_ensemble(self, data_collection_index=None, num_particles=400, T_rollout=None, seed=None):
        """The particle picture of the open-loop check: ``num_particles`` sampled open-loop trajectories per recorded run, each started at
        the run's first recorded state and driven by its recorded inputs -- for every recorded run (``data_collection_index`` None; or one
        index, or a list) in ONE launch (ragged lengths, M = runs x particles).  Returns a list with one array [T_run, num_particles, S] per
        run (the array itself for a single index) and prints, per state, the MSE of the particle mean and the share of recorded samples
        within mean +- 2 std.  The draws are Philox keyed by (``seed``, default ``self.seed``; the run's index; the particle): a run's
        particles do not depend on which other runs share the launch."""
        f = getattr(self.model_learning, "steps_like_the_packed_model", None)
        if not (callable(f) and f()):  # (the predicate of rollout(): a model whose own step the layout does not describe must not be simulated by it)
            raise NotImplementedError("rollout_ensemble needs a model with a fused-rollout layout whose get_next_state is the step that layout "
                                      "describes (Model_learning.steps_like_the_packed_model)")
        single = data_collection_index is not None and np.isscalar(data_collection_index)
        runs = (list(range(len(self.state_samples_history))) if data_collection_index is None
                else [int(data_collection_index)] if single else [int(i) for i in data_collection_index])
        runs = [r % len(self.state_samples_history) for r in runs]
        P = int(num_particles)
        lens = [int(self.state_samples_history[r].shape[0]) if T_rollout is None else min(int(T_rollout), int(self.state_samples_history[r].shape[0]))
                for r in runs]
        if not runs or P < 1 or min(lens) < 2:
            raise ValueError("rollout_ensemble needs at least one recorded run of two samples and one particle")
        # global trajectory id = run index * num_particles + particle (mcp_noise.particle_offset): a run's draws are the same whether it is
        # launched alone or with the others.  Consecutive run indices share a launch -- every recorded run: ONE launch.
        groups = [[0]]
        for k in range(1, len(runs)):
            if runs[k] == runs[k - 1] + 1:
                groups[-1].append(k)
            else:
                groups.append([k])
        sd = self.seed if seed is None else int(seed)
        stat = torch.zeros(1, dtype=torch.int32, device=self.device)
        t_dev = lambda a, dt: torch.tensor(a, dtype=dt, device=self.device)
        U, parts, out = self.input_dim, {}, []
        for grp in groups:
            Tm = max(max(lens[k] for k in grp), 2)
            x0 = np.concatenate([np.repeat(np.asarray(self.state_samples_history[runs[k]])[0:1, :], P, 0) for k in grp], 0)
            u = np.zeros([Tm - 1, len(grp) * P, U])
            for i, k in enumerate(grp):
                u[:lens[k] - 1, i * P:(i + 1) * P, :] = np.asarray(self.input_samples_history[runs[k]])[:lens[k] - 1, None, :]
            noise = ops.NoiseSpec(seed=sd, call=0, particle_offset=runs[grp[0]] * P)
            states, _ = ops.rollout_open(self.model_learning.packed(), t_dev(x0, self.dtype), t_dev(u, self.dtype),
                                         lengths=t_dev(np.repeat([lens[k] for k in grp], P), torch.int32), noise=noise, particle_pred=True, status=stat)
            for i, k in enumerate(grp):
                parts[k] = states[:lens[k], i * P:(i + 1) * P, :].cpu().numpy()
        self.last_status = stat
        for k, r in enumerate(runs):
            part = parts[k]
            obs = np.asarray(self.state_samples_history[r])[:lens[k]]
            mean, std = part.mean(1), part.std(1)
            print("Run", r, "ensemble mean MSE per state:", np.mean((mean - obs) ** 2, 0), " inside mean +- 2 std:",
                  np.mean(np.abs(obs - mean) <= 2 * std, 0))
            out.append(part)
        return out[0] if single else out

    def get_model_learning_performance(self, data_collection_index, flg_pretrain=False):
        """One-step GP predictions on the data of one interaction with the system (MC_PILCO.py:260-306): prints the MSE per GP,
        returns (gp_inputs, targets [numpy per GP], means [numpy per GP], variances [tensors, scaled by norm_list^2])."""
        ml = self.model_learning
        t_dev = lambda a: torch.tensor(a, dtype=self.dtype, device=self.device)
        gp_inputs, targets, means, variances = ml.get_gp_estimate_from_data(states=t_dev(self.state_samples_history[data_collection_index]),
                                                                           inputs=t_dev(self.input_samples_history[data_collection_index]),
                                                                           flg_pretrain=flg_pretrain)
        variances = [variances[i] * ml.norm_list[i] ** 2 for i in range(ml.num_gp)]
        targets = [targets[i].detach().cpu().numpy() for i in range(ml.num_gp)]
        means = [means[i].detach().cpu().numpy() for i in range(ml.num_gp)]
        for i in range(ml.num_gp):
            print("MSE gp" + str(i) + ": ", ((targets[i] - means[i]) ** 2).mean())
        return gp_inputs, targets, means, variances

    def get_rollout_prediction_performance(self, data_collection_index, T_rollout=None, add_name="", particle_pred=False):
        """Open-loop rollout of the learned model on the inputs of one interaction (MC_PILCO.py:308-345); ``particle_pred``:
        sampled instead of mean predictions, as in the reference."""
        pred = self.rollout(data_collection_index, T_rollout=T_rollout, particle_pred=particle_pred)
        obs = self.state_samples_history[data_collection_index][: pred.shape[0]]
        print("Rollout prediction MSE per state:", np.mean((pred - obs) ** 2, 0))
        return pred, obs, self.input_samples_history[data_collection_index]

    def load_policy_from_log(self, num_trial, folder="results_tmp/1/"):
        log = pkl.load(open(folder + "log.pkl", "rb"))
        self.control_policy.load_state_dict(log["parameters_trial_list"][num_trial - 1])

    def load_model_from_log(self, num_trial, folder="results_tmp/1/"):
        """Replays the logged data into the model, restores the GP hyper-parameters of trial ``num_trial-1`` and pretrains."""
        log = pkl.load(open(folder + "log.pkl", "rb"))
        self.log_dict = log
        for k in ("cost_trial_list", "parameters_trial_list", "particles_states_list", "particles_inputs_list"):
            self.log_dict[k] = self.log_dict[k][0:num_trial]
        for j in range(num_trial + 1):
            self.state_samples_history.append(log["state_samples_history"][j])
            self.input_samples_history.append(log["input_samples_history"][j])
            self.noiseless_states_history.append(log["noiseless_states_history"][j])
            self.num_data_collection += 1
            self.model_learning.add_data(new_state_samples=log["state_samples_history"][j], new_input_samples=log["input_samples_history"][j])
        t = num_trial - 1
        ml = self.model_learning
        ml.gp_inputs = log["gp_inputs_" + str(t)].to(self.device)
        ml.gp_output_list = [y.to(self.device) for y in log["gp_output_list_" + str(t)]]
        for k in range(ml.num_gp):
            ml.gp_list[k].load_state_dict(log["parameters_gp_" + str(t)][k])
        with torch.no_grad():
            for k in range(ml.num_gp):
                ml.pretrain_gp(k)


class MC_PILCO4PMS(MC_PILCO):
    """MC-PILCO for partially measurable systems -- drop-in for ``MC_PILCO4PMS`` (MC_PILCO.py:755-958).

    Particles evolve on their true states; the policy is evaluated on a simulated *measurement*: positions plus Gaussian
    noise, velocities by backward difference of the noisy positions, smoothed online by a first-order Butterworth filter
    (``filtering_dict["fc"]``).  With the speed-integration models and the RBF policies the rollout is the same single fused
    launch as ``MC_PILCO.apply_policy``: the kernels carry the filter's states per particle and the reverse sweep its adjoint
    recursion (``mcp_meas``); a trainable ``PD_controller`` runs on its own fused launch and sweep with the same measurement model
    (``mcp_rollout_pd_meas``), and so does an ``MLP_policy`` (``mcp_rollout_mlp_meas``; ``fused_feedback = False``: the step loop for
    both).  ``fused = False`` (or any other model / policy object) runs step by step on the posterior and
    policy operators with the filter as torch device ops.
    """

    def __init__(self, T_sampling, state_dim, input_dim, f_sim, f_model_learning, model_learning_par, f_rand_exploration_policy,
                 rand_exploration_policy_par, f_control_policy, control_policy_par, f_cost_function, cost_function_par, pos_indeces,
                 vel_indeces, std_meas_noise=None, log_path=None, filtering_dict={}, std_meas_noise_sim=None, dtype=torch.float64,
                 device=torch.device("cuda")):
        super().__init__(T_sampling=T_sampling, state_dim=state_dim, input_dim=input_dim, f_sim=f_sim, f_model_learning=f_model_learning,
                         model_learning_par=model_learning_par, f_rand_exploration_policy=f_rand_exploration_policy,
                         rand_exploration_policy_par=rand_exploration_policy_par, f_control_policy=f_control_policy,
                         control_policy_par=control_policy_par, f_cost_function=f_cost_function, cost_function_par=cost_function_par,
                         std_meas_noise=std_meas_noise, log_path=log_path, dtype=dtype, device=device)
        self.system = _sim.PMS_Model(f_sim, filtering_dict)
        self.filtering_dict = filtering_dict
        self.pos_indeces = pos_indeces
        self.vel_indeces = vel_indeces
        # (the reference leaves the attribute unset when a value is passed, MC_PILCO.py:802-803; here it is always defined)
        self.std_meas_noise_sim = std_meas_noise if std_meas_noise_sim is None else std_meas_noise_sim
        self.fused = True  # False: step-by-step rollout on the posterior / policy operators (any model or policy object)

    def _measured_model(self):
        """The packed model a fused rollout on measurements launches."""
        model = self.model_learning.packed()
        if getattr(model, "is_delta", False) and model.Ts != float(self.T_sampling):
            model = self.model_learning.packed(T_sampling=self.T_sampling)  # (a delta-state model has no Ts: the measured velocities need one)
        return model

    def _meas_spec(self, b, a, pos_noise):
        pos = list(self.pos_indeces)
        return ops.MeasSpec(pos=pos, vel=list(self.vel_indeces), std_pos=[float(v) for v in np.asarray(self.std_meas_noise_sim)[pos]], b=b, a=a,
                            pos_noise=pos_noise)

    def apply_policy(self, particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                     particles_init_low_bound, flg_particles_init_multi_gauss, num_particles, T_control, p_dropout=0.0):
        from scipy import signal

        M, T, x = self._begin_rollout(particles_initial_state_mean, particles_initial_state_var, flg_particles_init_uniform, particles_init_up_bound,
                                      particles_init_low_bound, flg_particles_init_multi_gauss, num_particles, T_control)
        pol, ml = self.control_policy, self.model_learning
        ref = self.noise_mode == "reference"  # draw on the CPU with the reference's calls, in its order
        ndev = torch.device("cpu") if ref else self.device
        b, a = signal.butter(1, self.filtering_dict["fc"])
        pos, vel = list(self.pos_indeces), list(self.vel_indeces)
        self.last_feedback_fused = False  # (reset before every branch, as in MC_PILCO.apply_policy)
        self.last_step_fused = False
        # the fused rollouts of MC_PILCO.apply_policy, launched on the measured model with the measurement filter between particles and policy
        out = self._fused_rollout(x, T, p_dropout, self._measured_model, partial(self._meas_spec, b, a), len(pos)) if self.fused else None
        if out is not None:
            return out
        self.last_status = None  # (no fused launch)
        if self._world()[0] > 1:  # (per-LOCAL-particle torch draws: identically seeded ranks would simulate correlated shards)
            raise NotImplementedError("particle sharding needs the fused rollout (fused=True, Sum_of_gaussians, PD_controller, TV_linear_controller or MLP_policy "
                                      "policy, a model with a fused layout)")
        std_pos = torch.tensor(np.asarray(self.std_meas_noise_sim)[pos], dtype=self.dtype, device=self.device)
        step = self._step_fused(T, n_pos=len(pos))
        saved_mode = getattr(pol, "noise_mode", None)
        if ref and saved_mode is not None:
            pol.noise_mode = "torch_cpu"
        try:
            xs = [x]
            noisy_prev, meas_prev = x, x
            us = [pol(x, t=0, p_dropout=p_dropout)]
            for t in range(1, T):
                if step:  # one launch; its eps (and in "reference" mode the position noise below) are _rollout_noise's, in the reference's order
                    x, _, _ = step(xs[-1], us[-1], t - 1)
                    xs.append(x)
                    n = step.pos_noise[t - 1] if step.pos_noise is not None else torch.randn(M, len(pos), dtype=self.dtype, device=self.device)
                else:
                    _, _, mean_list, var_list = ml.get_one_step_gp_out(states=xs[-1], inputs=us[-1])
                    var_list = [v * ml.norm_list[i] ** 2 for i, v in enumerate(var_list)]
                    mean, var = torch.cat(mean_list, 1), torch.cat(var_list, 1)
                    eps = torch.empty(M, ml.num_gp, dtype=self.dtype, device=ndev).normal_().to(self.device)
                    delta = mean + torch.sqrt(var) * eps
                    x, _, _ = ml.get_next_state_from_gp_output(current_state=xs[-1], current_input=us[-1],
                                                               gp_output_mean_list=[delta[:, g:g + 1] for g in range(ml.num_gp)],
                                                               gp_output_var_list=var_list, particle_pred=False)
                    xs.append(x)
                    n = torch.randn(M, len(pos), dtype=self.dtype, device=ndev).to(self.device)
                noisy = x.clone()
                noisy[:, pos] = noisy[:, pos] + std_pos * n
                noisy[:, vel] = (noisy[:, pos] - noisy_prev[:, pos]) / self.T_sampling
                meas = noisy.clone()
                meas[:, vel] = (b[0] * noisy[:, vel] + b[1] * noisy_prev[:, vel] - a[1] * meas_prev[:, vel]) / a[0]
                us.append(pol(meas, t=t, p_dropout=p_dropout))
                noisy_prev, meas_prev = noisy, meas
        finally:
            if saved_mode is not None:
                pol.noise_mode = saved_mode
        return torch.stack(xs), torch.stack(us)

    def get_data_from_system(self, initial_state, T_exploration, trial_index, flg_exploration=False):
        policy = self.rand_exploration_policy if flg_exploration else self.control_policy
        meas, inputs, clean, noisy = self.system.rollout(s0=initial_state, policy=policy.get_np_policy(), T=T_exploration, dt=self.T_sampling,
                                                         noise=self.std_meas_noise, vel_indeces=self.vel_indeces, pos_indeces=self.pos_indeces)
        states, meas, inputs, clean, noisy = self.get_velocities(meas, inputs, clean, noisy)
        self.state_samples_history.append(states)
        self.input_samples_history.append(inputs)
        self.noiseless_states_history.append(clean)
        self.num_data_collection += 1
        self.model_learning.add_data(new_state_samples=states, new_input_samples=inputs)

    def get_velocities(self, meas_states, input_samples, noiseless_samples, noisy_samples):
        """Offline filtering of the collected data for model learning (MC_PILCO.py:938-958): zero-phase second-order Butterworth
        on the positions, central-difference velocities, first and last sample dropped."""
        from scipy import signal

        states = np.zeros([noisy_samples.shape[0] - 2, noisy_samples.shape[1]])
        bb, aa = signal.butter(2, 0.5)
        for i in range(len(self.pos_indeces)):
            pos = signal.filtfilt(bb, aa, noisy_samples[:, self.pos_indeces[i]])
            states[:, self.pos_indeces[i]] = pos[1:-1]
            states[:, self.vel_indeces[i]] = (pos[2:] - pos[:-2]) / (2 * self.T_sampling)
        return states, meas_states[1:-1, :], input_samples[1:-1, :], noiseless_samples[1:-1, :], noisy_samples[1:-1, :]
