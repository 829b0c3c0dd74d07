"""Host-side operators over the C ABI (hipabi): descriptor packing, workspaces and the
torch.autograd.Function wrappers that make the HIP kernels differentiable from Python.

Everything here is plumbing around ``libmcpilco_hip.so``; no arithmetic of the hot path is
done in PyTorch.  All tensors are float64 on the GPU.
"""
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hipabi as abi

DT = torch.float64


def _dev(device=None):
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mc_pilco_amd runs on the GPU only (device=%s requested); there is no CPU path" % device)
    return device


def _t(x, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=DT).contiguous()
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(device).contiguous()


def _count(x):
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(np.asarray(x).size)


def pad16(n):
    return (int(n) + 15) // 16 * 16


# --------------------------------------------------------------------------------------
# kernel hyper-parameters -> mcp_kernel
# --------------------------------------------------------------------------------------
@dataclass
class KernelSpec:
    """SE (+ Volterra polynomial) covariance in the library's parametrisation.

    ``w1`` [D+1], ``w20``/``w21`` [D] are the squared diagonal weights the reference's
    ``MPK_GP.get_Sigma`` builds (Sparse_GP.py:613-623): for MPK_k, factor d has
    s_d = (k-d)*exp(par[d*n:(d+1)*n]) and weight s_d**2.
    """

    lengthscales: torch.Tensor  # [D]
    lam: float
    sigma_n2: float
    mean: float = 0.0
    w1: Optional[torch.Tensor] = None
    w20: Optional[torch.Tensor] = None
    w21: Optional[torch.Tensor] = None
    scal: Optional[torch.Tensor] = None  # device [lambda, sigma_n2, mean]: overrides the three floats (no host round trip to fill them)
    _keep: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def D(self):
        return int(self.lengthscales.numel())

    @property
    def poly_deg(self):
        return 0 if self.w1 is None else (1 if self.w20 is None else 2)

    def _device_operands(self, device):
        """Device copies of the hyper-parameter vectors, uploaded ONCE per device and kept for the life of the spec: every
        descriptor built from this spec (mcp_kernel inside mcp_gp inside mcp_model) points at the same tensors, so a later
        to_c() can never free memory an older descriptor still refers to."""
        key = (device.type, device.index)
        ops_ = self._keep.get(key)
        if ops_ is None:
            ops_ = {"inv_ls": (1.0 / _t(self.lengthscales, device)).contiguous()}
            for name in ("w1", "w20", "w21"):
                v = getattr(self, name)
                ops_[name] = None if v is None else _t(v, device)
            self._keep[key] = ops_
        return ops_

    def to_c(self, device):
        device = _dev(device)
        ops_ = self._device_operands(device)
        k = abi.Kernel()
        k.D = self.D
        k.poly_deg = self.poly_deg
        k.lam = float(self.lam)
        k.sigma_n2 = float(self.sigma_n2)
        k.mean = float(self.mean)
        k.inv_ls = ops_["inv_ls"].data_ptr()
        for name in ("w1", "w20", "w21"):
            setattr(k, name, None if ops_[name] is None else ops_[name].data_ptr())
        k.scal = None if self.scal is None else self.scal.data_ptr()
        return k


def mpk_weights(log_par, k):
    """Squared diagonal weights of MPK_k from its raw log parameters (list over the k factors)."""
    par = torch.as_tensor(log_par, dtype=DT).reshape(-1)
    n = par.numel() // k
    return [((k - d) * torch.exp(par[d * n:(d + 1) * n])) ** 2 for d in range(k)]


# --------------------------------------------------------------------------------------
# pretrain primitives
# --------------------------------------------------------------------------------------
def cov_build(spec: KernelSpec, X1, X2=None, noise=False):
    X1 = _t(X1, X1.device if isinstance(X1, torch.Tensor) else None)
    dev = X1.device
    X2t = X1 if X2 is None else _t(X2, dev)
    K = torch.empty(X1.shape[0], X2t.shape[0], dtype=DT, device=dev)
    kc = spec.to_c(dev)
    abi.check(abi.lib().mcp_cov_build(C.byref(kc), X1.shape[0], abi.ptr(X1), X2t.shape[0], abi.ptr(X2t), int(bool(noise)), abi.ptr(K),
                                      K.shape[1], abi.stream()), "mcp_cov_build")
    return K


def cov_diag(spec: KernelSpec, X, noise=False):
    X = _t(X, X.device)
    d = torch.empty(X.shape[0], dtype=DT, device=X.device)
    kc = spec.to_c(X.device)
    abi.check(abi.lib().mcp_cov_diag(C.byref(kc), X.shape[0], abi.ptr(X), int(bool(noise)), abi.ptr(d), abi.stream()), "mcp_cov_diag")
    return d


def chol_factor(K):
    """Returns (U upper with K=U^T U, logdet, status word tensor).  K is not modified."""
    U = K.detach().clone().contiguous()
    N = U.shape[0]
    logdet = torch.zeros(1, dtype=DT, device=U.device)
    status = torch.zeros(1, dtype=torch.int32, device=U.device)
    abi.check(abi.lib().mcp_chol_factor(N, abi.ptr(U), U.shape[1], abi.ptr(logdet), abi.ptr(status), abi.stream()), "mcp_chol_factor")
    return U, logdet[0], status


def chol_inverse(U):
    N = U.shape[0]
    Ui = torch.zeros(N, N, dtype=DT, device=U.device)
    Kinv = torch.empty(N, N, dtype=DT, device=U.device)
    abi.check(abi.lib().mcp_chol_inverse(N, abi.ptr(U), U.shape[1], abi.ptr(Ui), N, abi.ptr(Kinv), N, abi.stream()), "mcp_chol_inverse")
    return Ui, Kinv


def sym_sandwich(A, G):
    """A G A for a symmetric A (K^-1) and any G, on the library's MFMA GEMM (mcp_sym_sandwich)."""
    N = A.shape[0]
    A = A.detach().to(dtype=DT).contiguous()
    G = G.detach().to(device=A.device, dtype=DT).contiguous()
    out = torch.empty(N, N, dtype=DT, device=A.device)
    scratch = torch.empty(N, N, dtype=DT, device=A.device)
    abi.check(abi.lib().mcp_sym_sandwich(N, abi.ptr(A), N, abi.ptr(G), N, abi.ptr(out), N, abi.ptr(scratch), abi.stream()), "mcp_sym_sandwich")
    return out


def gp_alpha(Kinv, Y, mean=0.0):
    N = Kinv.shape[0]
    Y = _t(Y, Kinv.device).reshape(-1)
    alpha = torch.empty(N, dtype=DT, device=Kinv.device)
    abi.check(abi.lib().mcp_gp_alpha(N, abi.ptr(Kinv), Kinv.shape[1], abi.ptr(Y), float(mean), abi.ptr(alpha), abi.stream()), "mcp_gp_alpha")
    return alpha.reshape(-1, 1)


sod_fallbacks = 0  # calls of sod_select whose multi-workgroup launch reported "never met" and were repeated on one workgroup


def sod_select(spec: KernelSpec, X, threshold, one_workgroup=False) -> List[int]:
    """GP_prior.get_SOD (GP_prior.py:232-257) on the device.  From 256 candidates on the selection runs across workgroups (one per 64 candidates)
    when the workspace has room for their exchange -- `mcp_sod_workspace_bytes` says how much; ``one_workgroup`` passes the first part only (W and
    the running sums) and so keeps the one-workgroup kernel (tests, timing)."""
    X = _t(X, X.device)
    N = X.shape[0]
    dev = X.device
    nbytes = 8 * (N * N + 2 * N) if one_workgroup else abi.lib().mcp_sod_workspace_bytes(N)
    ws = torch.empty((nbytes + 7) // 8, dtype=DT, device=dev)
    idx = torch.zeros(N, dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    kc = spec.to_c(dev)
    abi.check(abi.lib().mcp_sod_select(C.byref(kc), N, abi.ptr(X), float(threshold), abi.ptr(idx), abi.ptr(n), abi.ptr(ws), nbytes,
                                       abi.stream()), "mcp_sod_select")
    cnt = int(n.item())
    if cnt < 0:  # the workgroups never met (the device could not hold the grid, e.g. shared with another process): the one-workgroup kernel
        if one_workgroup:
            raise RuntimeError("mcp_sod_select reported %d kept rows" % cnt)
        global sod_fallbacks
        sod_fallbacks += 1
        if sod_fallbacks == 1:  # (every such call has spun to its limit first -- seconds: say so once, keep counting)
            import warnings

            warnings.warn("mcp_sod_select: the workgroups of the multi-workgroup selection never met (is the GPU shared with another process?); "
                          "this and later such calls are repeated on the one-workgroup kernel (ops.sod_fallbacks counts them)", RuntimeWarning)
        return sod_select(spec, X, threshold, one_workgroup=True)
    return [int(i) for i in idx[:cnt].tolist()]


# --------------------------------------------------------------------------------------
# packed GP / model descriptors
# --------------------------------------------------------------------------------------
class PackedGP:
    """Device-resident operands of one pretrained GP in the kernels' layout (mcp_gp)."""

    def __init__(self, spec: KernelSpec, X, alpha, Kinv):
        dev = _dev(Kinv.device)
        X = _t(X, dev)
        alpha = _t(alpha, dev).reshape(-1)
        Kinv = _t(Kinv, dev)
        N, D = X.shape
        self.N, self.D, self.Npad = N, D, pad16(N)
        self.spec = spec
        self.Xt = torch.empty(D, self.Npad, dtype=DT, device=dev)
        self.X = torch.empty(self.Npad, D, dtype=DT, device=dev)
        self.alpha = torch.empty(self.Npad, dtype=DT, device=dev)
        self.Kinv = torch.empty(self.Npad, self.Npad, dtype=DT, device=dev)
        self.aX = torch.empty(D, dtype=DT, device=dev)
        abi.check(abi.lib().mcp_gp_pack(N, D, abi.ptr(X), abi.ptr(alpha), abi.ptr(Kinv), Kinv.shape[1], self.Npad, abi.ptr(self.Xt),
                                        abi.ptr(self.X), abi.ptr(self.alpha), abi.ptr(self.Kinv), abi.ptr(self.aX), abi.stream()),
                  "mcp_gp_pack")
        self.device = dev

    def fill(self, g: abi.GP):
        g.kern = self.spec.to_c(self.device)
        g.N, g.Npad = self.N, self.Npad
        g.Xt, g.X, g.alpha, g.Kinv, g.aX = (self.Xt.data_ptr(), self.X.data_ptr(), self.alpha.data_ptr(), self.Kinv.data_ptr(),
                                            self.aX.data_ptr())

    def to_c(self):
        g = abi.GP()
        self.fill(g)
        return g


class PackedModel:
    """mcp_model: the dynamics model with its G packed GPs.  Speed integration: ``not_vel[g]`` is the position integrated from
    state ``vel[g]``; -1 there means none (x'[vel[g]] = x[vel[g]] + delta_g) -- ``PackedModel.delta`` builds that layout."""

    @classmethod
    def delta(cls, gps: Sequence[PackedGP], S, U, angle, not_angle, Ts=0.0, var_scale=None):
        """Delta-state model (Model_learning.py:471-493): GP i predicts x_{t+1}[i] - x_t[i] for every state, G = S.  ``Ts`` only
        serves a measurement model (MC_PILCO4PMS's velocity differences); the integrator has no Ts term."""
        if len(gps) != int(S):
            raise ValueError("a delta-state model has one GP per state component (%d GPs, %d states)" % (len(gps), int(S)))
        return cls(gps, S, U, Ts, angle, not_angle, list(range(int(S))), [-1] * int(S), var_scale=var_scale)

    def __init__(self, gps: Sequence[PackedGP], S, U, Ts, angle, not_angle, vel, not_vel, var_scale=None):
        self.gps = list(gps)
        # (what model_lists_ok refuses with a bare MCP_ERR_ARG: every component at most once per role, written by at most one GP)
        for name, lst in (("angle", angle), ("not_angle", not_angle), ("vel", vel), ("not_vel", [v for v in not_vel if int(v) >= 0])):
            ints = [int(v) for v in lst]
            if len(set(ints)) != len(ints):
                raise ValueError("the model's %s list names an index twice: %s" % (name, ints))
        both = sorted(set(int(v) for v in vel) & set(int(v) for v in not_vel))
        if both:
            raise ValueError("the model's vel and not_vel lists share the components %s: a component is written by one GP at the most" % both)
        m = abi.Model()
        m.S, m.U, m.G, m.D = int(S), int(U), len(self.gps), self.gps[0].D
        m.n_angle, m.n_not_angle = len(angle), len(not_angle)
        for i, v in enumerate(angle):
            m.angle[i] = int(v)
        for i, v in enumerate(not_angle):
            m.not_angle[i] = int(v)
        for i, v in enumerate(vel):
            m.vel[i] = int(v)
        for i, v in enumerate(not_vel):
            m.not_vel[i] = int(v)  # (written for every GP: -1 must not be left at the ctypes default 0, a valid position)
        m.Ts = float(Ts)
        for g in range(abi.MAX_GP):
            m.var_scale[g] = 1.0 if var_scale is None or g >= len(var_scale) else float(var_scale[g])
        for g, pg in enumerate(self.gps):
            pg.fill(m.gp[g])
        self.c = m
        self.S, self.U, self.G, self.D = m.S, m.U, m.G, m.D
        self.Ts = m.Ts
        self.is_delta = all(int(v) == -1 for v in not_vel)
        self.device = self.gps[0].device


class PackedPolicy:
    """mcp_policy over the live parameter tensors (no copies: the optimizer's updates are seen)."""

    def __init__(self, kind, S, log_ls, centers, weight, u_max, squash=True, angle=(), non_angle=(), target_traj=None, bias=None):
        dev = _dev(centers.device)
        self.log_ls, self.centers, self.weight = log_ls, centers, weight
        self.bias = bias  # [U] f_linear.bias (flg_bias) or None
        B, P = centers.shape
        U = weight.shape[0]
        if (P > 16 or U > 4) and B > abi.MAX_BASIS_WIDE:
            # (refused here, not at the first backward(): the adjoint sweep of these widths has one thread per basis function, 512 at the most)
            raise ValueError("a policy with more than 16 features or more than 4 inputs (P = %d, U = %d) takes at most MCP_MAX_BASIS_WIDE = %d "
                             "basis functions (%d given): the adjoint sweep of the wide classes has no larger form" % (P, U, abi.MAX_BASIS_WIDE, B))
        um = np.full(U, float(u_max)) if np.isscalar(u_max) else np.asarray(u_max, dtype=np.float64).reshape(-1)
        self.u_max = _t(um, dev)
        self.target_traj = None if target_traj is None else _t(target_traj, dev)
        p = abi.Policy()
        p.kind = {"plain": abi.POLICY_PLAIN, "angles": abi.POLICY_ANGLES, "traj": abi.POLICY_TRAJ}[kind]
        p.S, p.P, p.B, p.U, p.squash = int(S), int(P), int(B), int(U), int(bool(squash))
        p.n_angle, p.n_non_angle = len(angle), len(non_angle)
        for i, v in enumerate(angle):
            p.angle[i] = int(v)
        for i, v in enumerate(non_angle):
            p.non_angle[i] = int(v)
        p.traj_len = 0 if self.target_traj is None else int(self.target_traj.shape[0])
        p.u_max = self.u_max.data_ptr()
        p.target_traj = None if self.target_traj is None else self.target_traj.data_ptr()
        self.c = p
        self.kind, self.S, self.P, self.B, self.U = kind, int(S), int(P), int(B), int(U)
        self.device = dev
        self.grad_flat = None  # optional caller-owned flat fp64 buffer the adjoint sweep writes its gradients into (rollout_backward_raw)

    def grad_numel(self):
        """Doubles of the flat gradient [log_ls | centers | weight | bias]."""
        return self.P + self.B * self.P + self.U * self.B + (self.U if self.bias is not None else 0)

    def bind(self, p_drop):
        """Refreshes parameter pointers (they must be contiguous fp64 GPU tensors) and p_drop."""
        for t in (self.log_ls, self.centers, self.weight) + (() if self.bias is None else (self.bias,)):
            if t.dtype != DT or not t.is_cuda or not t.is_contiguous():
                raise RuntimeError("policy parameters must be contiguous float64 GPU tensors")
        if self.bias is not None and self.bias.numel() != self.U:
            raise RuntimeError("policy bias must have one entry per input")
        self.c.bias = None if self.bias is None else self.bias.data_ptr()
        self.c.g_bias = None
        self.c.log_ls = self.log_ls.data_ptr()
        self.c.centers = self.centers.data_ptr()
        self.c.weight = self.weight.data_ptr()
        self.c.p_drop = float(p_drop)
        return self.c


@dataclass
class NoiseSpec:
    """Parity mode: eps [T-1,M,G] float64 and masks [T,M,B] uint8 on the GPU.  Performance mode:
    both None -> in-kernel Philox keyed by (seed, call) and the global particle id."""

    eps: Optional[torch.Tensor] = None
    masks: Optional[torch.Tensor] = None
    seed: int = 0
    call: int = 0
    particle_offset: int = 0
    call_dev: Optional[torch.Tensor] = None  # device int64 [1] added to ``call`` by the kernels (a rollout replayed from a HIP graph: the graph advances it)

    def to_c(self):
        n = abi.Noise()
        n.eps = None if self.eps is None else self.eps.data_ptr()
        n.masks = None if self.masks is None else self.masks.data_ptr()
        n.seed, n.call, n.particle_offset = int(self.seed) & (2**64 - 1), int(self.call) & (2**64 - 1), int(self.particle_offset)
        if self.call_dev is not None:
            if self.call_dev.dtype != torch.int64 or not self.call_dev.is_cuda or self.call_dev.numel() != 1:
                raise RuntimeError("call_dev must be a one-element int64 GPU tensor")
            n.call_dev = self.call_dev.data_ptr()
        return n


@dataclass
class MeasSpec:
    """Measurement model of ``MC_PILCO4PMS.apply_policy`` (MC_PILCO.py:808-906) for the fused rollout: the policy is fed
    noisy positions and backward-difference velocities smoothed by the first-order filter (b, a) = butter(1, fc).
    ``pos_noise`` [T-1,M,n] standard normals on the GPU (parity mode) or None (in-kernel Philox).  ``measured``: an OUTPUT -- ``rollout_pd``
    leaves the measured states [T,M,S] of its last launch with this spec there."""

    pos: Sequence[int]
    vel: Sequence[int]
    std_pos: Sequence[float]
    b: Sequence[float]
    a: Sequence[float]
    pos_noise: Optional[torch.Tensor] = None
    measured: Optional[torch.Tensor] = None

    def fill(self, m, T, M, meas_buf):
        n = len(self.pos)
        if len(self.vel) != n or len(self.std_pos) != n or n > abi.MAX_STATE:
            raise RuntimeError("pos / vel / std_pos must have the same length")
        m.n = n
        for i in range(n):
            m.pos[i], m.vel[i], m.std_pos[i] = int(self.pos[i]), int(self.vel[i]), float(self.std_pos[i])
        m.b0, m.b1, m.a0, m.a1 = float(self.b[0]), float(self.b[1]), float(self.a[0]), float(self.a[1])
        if self.pos_noise is not None:
            q = self.pos_noise
            if q.dtype != DT or not q.is_cuda or not q.is_contiguous() or tuple(q.shape) != (max(T - 1, 0), M, n):
                raise RuntimeError("pos_noise must be a contiguous float64 GPU tensor of shape [T-1,M,n]")
        m.pos_noise = None if self.pos_noise is None else self.pos_noise.data_ptr()
        m.meas = meas_buf.data_ptr()


def _set_meas(policy, meas, T, M, buf):
    """Points policy.c.meas at the measurement model for the next launch (n = 0: the policy sees the true state)."""
    if meas is None:
        policy.c.meas.n = 0
        policy.c.meas.meas = None
        policy.c.meas.pos_noise = None
    else:
        meas.fill(policy.c.meas, T, M, buf)


# --------------------------------------------------------------------------------------
# fused rollout (autograd)
# --------------------------------------------------------------------------------------
def _check_noise(noise, T, M, G, B):
    if noise.eps is not None:
        e = noise.eps
        if e.dtype != DT or not e.is_cuda or not e.is_contiguous() or tuple(e.shape) != (max(T - 1, 0), M, G):
            raise RuntimeError("eps must be a contiguous float64 GPU tensor of shape [T-1,M,G]")
    if noise.masks is not None:
        k = noise.masks
        if k.dtype != torch.uint8 or not k.is_cuda or not k.is_contiguous() or tuple(k.shape) != (T, M, B):
            raise RuntimeError("masks must be a contiguous uint8 GPU tensor of shape [T,M,B]")


def _status_word(status, dev, where):
    """The caller's status word (an int32[1] on ``dev`` that the kernels OR their flags into) after its check, or a fresh zeroed one."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    if status.dtype != torch.int32 or status.numel() != 1 or status.device != dev or not status.is_contiguous():
        raise RuntimeError("status must be a one-element int32 tensor on " + where)
    return status


def _record_buffers(dev, T, M, S, U, G, D, jac):
    """(states [T,M,S], inputs [T,M,U] -- None for U None --, jac [T-1,M,G,D] -- None unless ``jac``) of a rollout, uninitialised.  (The
    max(): a policy-only call, T == 1 without a model, has G == 0.)"""
    return (torch.empty(T, M, S, dtype=DT, device=dev), None if U is None else torch.empty(T, M, U, dtype=DT, device=dev),
            torch.empty(max(T - 1, 1), M, max(G, 1), D, dtype=DT, device=dev) if jac else None)


def _open_operands(model, x0, u, T, lengths, noise, particle_pred, status, mask_width=0):
    """The operands of the open-loop and PD rollouts as the library takes them: x0 [M,S] and u [T-1,Mu,U] (a 2-D u is one shared sequence;
    u None: the PD forms, ``T`` given) contiguous float64 on the model's device, ``lengths`` int32 [M], a NoiseSpec (checked under
    ``particle_pred``; ``mask_width``: the width of a mask row of a policy with dropout, whose masks are checked either way) and the
    status word.  Returns (x0, u, T, lengths, noise, status)."""
    dev = model.device
    x0 = x0.to(device=dev, dtype=DT).contiguous()
    if x0.dim() != 2 or x0.shape[1] != model.S:
        raise RuntimeError("x0 must be [M,%d]" % model.S)
    M = int(x0.shape[0])
    if u is not None:
        u = u.to(device=dev, dtype=DT)
        if u.dim() == 2:
            u = u.reshape(u.shape[0], 1, u.shape[1])  # (under autograd the gradient comes back in u's own shape)
        if u.dim() != 3 or u.shape[2] != model.U or u.shape[1] not in (1, M) or u.shape[0] < 1:
            raise RuntimeError("u must be [T-1,M,%d] or [T-1,%d]" % (model.U, model.U))
        u, T = u.contiguous(), int(u.shape[0]) + 1
    noise = NoiseSpec() if noise is None else noise
    if particle_pred:
        _check_noise(noise, T, M, model.G, mask_width)
    elif mask_width:
        _check_noise(NoiseSpec(masks=noise.masks), T, M, model.G, mask_width)
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int32).to(dev).contiguous()
        if tuple(lengths.shape) != (M,):
            raise RuntimeError("lengths must have one entry per trajectory")
    return x0, u, T, lengths, noise, _status_word(status, dev, "the rollout's device")


def _mc(model):
    return None if model is None else C.byref(model.c)


def _workspace(model, policy, pc, M, T, which):
    """(bytes, tensor) of the rollout workspace for this (model, policy shape, M, T), kept on the model object: the forward and the
    backward call each have their own (a step's backward runs after its forward on the same stream, and the next forward after that).
    One rollout at a time per model object: two host threads driving the SAME PackedModel on different streams would share these buffers
    (give each its own PackedModel; the operand tensors can be shared)."""
    if model is None:  # (policy-only evaluation: nothing to keep it on)
        nbytes = abi.lib().mcp_rollout_workspace_bytes(None, C.byref(pc), M, T)
        return nbytes, (torch.empty((nbytes + 7) // 8, dtype=DT, device=policy.device) if nbytes else None), None
    cache = model.__dict__.setdefault("_ws_cache", {})
    key = (which, int(M), int(T), policy.kind, policy.B, policy.P, policy.U, policy.c.meas.n)
    hit = cache.get(key)
    if hit is None:
        nbytes = abi.lib().mcp_rollout_workspace_bytes(_mc(model), C.byref(pc), M, T)
        if len(cache) >= 8:  # (a few shapes per model at most: the warm-up rollout, the optimisation, an evaluation)
            cache.clear()
        hit = cache[key] = (nbytes, torch.empty((nbytes + 7) // 8, dtype=DT, device=model.device) if nbytes else None, {"packed": 0})
    return hit


def rollout_forward_raw(model: Optional[PackedModel], policy: PackedPolicy, noise: NoiseSpec, x0, T, p_drop, particle_pred=True, need_jac=True,
                        meas: Optional[MeasSpec] = None, gp_sharding=True, status=None):
    """model None (only with T == 1) evaluates the policy alone.  gp_sharding False: the library never launches GP-sharded (the
    recovery path after MCP_STATUS_SYNC) -- by a flag, the workspace with the kernels' packed operand copies is still passed.
    ``status``: an int32[1] on the device that the kernels OR their flags INTO (a caller that only looks at the flags of many rollouts together
    passes one buffer to all of them: no zero-fill launch per rollout); None: a fresh zeroed word."""
    dev = policy.device if model is None else model.device
    x0 = x0.detach().to(device=dev, dtype=DT).contiguous()
    M = x0.shape[0]
    G, D = (0, policy.U) if model is None else (model.G, model.D)
    _check_noise(noise, T, M, G, policy.B)
    states, inputs, jac = _record_buffers(dev, T, M, policy.S, policy.U, G, D, need_jac and T > 1)
    status = _status_word(status, x0.device, "the rollout's device")
    pc = policy.bind(p_drop)
    nz = noise.to_c()
    meas_buf = torch.empty(T, M, policy.S, dtype=DT, device=dev) if meas is not None else None
    _set_meas(policy, meas, T, M, meas_buf)
    # workspace: the hand-off granules of the GP-sharded launch (small swarms) and the kernels' packed operand copies; the library zeroes /
    # rebuilds what it uses on the stream, so ONE buffer per (model, shape) serves every step of an optimisation (no size query, no
    # allocation per step)
    nbytes, ws, wstate = _workspace(model, policy, pc, M, T, "fwd") if (model is not None and T > 1) else (0, None, None)
    # the packed operand copies in the workspace (the lean kernel's Kinv tiles, the wide classes' phase-J operands) are functions of the model's
    # arrays alone: built by the first rollout that needs them, then kept -- a PackedModel's tensors are never written again, and this buffer
    # belongs to it (MCP_FWD_KT_PACKED / MCP_FWD_XJ_PACKED)
    pflags = 0 if wstate is None else wstate["packed"]
    ev = fwd_events
    try:
        if ev is not None:
            ev[0].record()
        # (the `_ex` entry point = mcp_rollout_fwd + the process's dispatch request / report, all zero unless a test or tool set it)
        abi.check(abi.lib().mcp_rollout_fwd_ex(_mc(model), C.byref(pc), C.byref(nz), M, T,
                                               int(bool(particle_pred)) | (0 if gp_sharding else abi.FWD_NO_GP_SHARDING) | pflags, abi.ptr(x0),
                                               abi.ptr(states), abi.ptr(inputs), abi.ptr(jac), abi.ptr(status), abi.ptr(ws), nbytes, abi.stream(),
                                               C.byref(abi.DISPATCH)), "mcp_rollout_fwd")
        if ev is not None:
            ev[1].record()
        if wstate is not None:  # what this call left in the workspace (it reports which kernel family ran)
            if abi.DISPATCH.ran_fwd_lean:
                wstate["packed"] |= abi.FWD_KT_PACKED
            elif abi.DISPATCH.ran_particles == 16 and model.D + 1 > 16:
                wstate["packed"] |= abi.FWD_XJ_PACKED
    finally:
        _set_meas(policy, None, T, M, None)
    if meas is not None:
        return states, inputs, jac, status, meas_buf
    return states, inputs, jac, status


def rollout_open(model: PackedModel, x0, u, *, lengths=None, noise: Optional[NoiseSpec] = None, particle_pred=False, moments=False, status=None):
    """Open-loop rollout of recorded inputs in ONE launch (mcp_rollout_open): x0 [M,S], u [T-1,M,U] or [T-1,U] / [T-1,1,U] (one input
    sequence shared by all trajectories) -> states [T,M,S].  ``particle_pred``: sampled increments (``noise``: an eps buffer [T-1,M,G] or
    Philox by seed / call / particle_offset), else the posterior mean.  ``lengths`` [M] (1 <= len <= T): trajectory m stops at row
    len - 1, its later rows are zeros.  ``moments``: also the GP means and scaled variances of every step, [T-1,M,G] (rows beyond a
    length stay zero).  Returns (states, status) or (states, mu, var, status).  No autograd: nothing here is differentiated."""
    for name, t in (("x0", x0), ("u", u)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("rollout_open operates on GPU memory only (%s is not a GPU tensor); there is no CPU path" % name)
        if t.requires_grad:
            raise RuntimeError("rollout_open has no gradient: %s requires grad (detach it; the closed-loop ops.rollout is the differentiable one)" % name)
    x0, u, T, lengths, noise, status = _open_operands(model, x0, u, None, lengths, noise, particle_pred, status)
    dev, M, Mu = model.device, int(x0.shape[0]), int(u.shape[1])
    states = torch.empty(T, M, model.S, dtype=DT, device=dev)
    mu = torch.zeros(T - 1, M, model.G, dtype=DT, device=dev) if moments else None
    var = torch.zeros(T - 1, M, model.G, dtype=DT, device=dev) if moments else None
    nz = noise.to_c()
    abi.check(abi.lib().mcp_rollout_open(_mc(model), C.byref(nz), M, T, int(bool(particle_pred)), abi.ptr(x0), abi.ptr(u), Mu, abi.ptr(lengths),
                                         abi.ptr(states), abi.ptr(mu), abi.ptr(var), abi.ptr(status), abi.stream()), "mcp_rollout_open")
    if moments:
        return states, mu, var, status
    return states, status


class RolloutOpenFunction(torch.autograd.Function):
    """(x0 [M,S], u [T-1,Mu,U]) -> states [T,M,S] through the recording form of the fused open-loop rollout (mcp_rollout_open_rec); backward is
    the reverse-time sweep mcp_rollout_open_bwd over the record.  Gradients flow to x0 and u; the GP model is frozen.  In sampled mode the
    draws are those of the NoiseSpec, and the backward differentiates the reparameterised sample."""

    @staticmethod
    def forward(ctx, x0, u, model, lengths, noise, particle_pred, status):
        T, Mu, M = int(u.shape[0]) + 1, int(u.shape[1]), int(x0.shape[0])
        states, _, jac = _record_buffers(model.device, T, M, model.S, None, model.G, model.D, True)  # (jac rows from len - 1 on: never written, never read)
        nz = noise.to_c()
        abi.check(abi.lib().mcp_rollout_open_rec(_mc(model), C.byref(nz), M, T, int(bool(particle_pred)), abi.ptr(x0), abi.ptr(u), Mu,
                                                 abi.ptr(lengths), abi.ptr(states), None, None, abi.ptr(jac), abi.ptr(status), abi.stream()),
                  "mcp_rollout_open_rec")
        ctx.model, ctx.lengths, ctx.Mu = model, lengths, Mu
        ctx.save_for_backward(states, jac)  # (saved tensors: autograd refuses a backward after an in-place change of either)
        return states

    @staticmethod
    def backward(ctx, g_states):
        states, jac = ctx.saved_tensors
        model = ctx.model
        T, M = int(states.shape[0]), int(states.shape[1])
        want_x0, want_u = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gs = g_states.to(dtype=DT).contiguous()
        g_x0 = torch.empty(M, model.S, dtype=DT, device=states.device) if want_x0 else None
        g_u = torch.empty(T - 1, M, model.U, dtype=DT, device=states.device) if want_u else None
        abi.check(abi.lib().mcp_rollout_open_bwd(_mc(model), M, T, abi.ptr(states), abi.ptr(ctx.lengths), abi.ptr(jac), abi.ptr(gs), abi.ptr(g_x0),
                                                 abi.ptr(g_u), abi.stream()), "mcp_rollout_open_bwd")
        if want_u and ctx.Mu == 1 and M > 1:
            g_u = g_u.sum(dim=1, keepdim=True)  # a shared input sequence: the trajectories' gradients added in torch's fixed order
        return g_x0, g_u, None, None, None, None, None


def rollout_open_diff(model: PackedModel, x0, u, *, lengths=None, noise: Optional[NoiseSpec] = None, particle_pred=False, status=None):
    """The differentiable open-loop rollout: arguments and states of ``rollout_open`` (bit for bit), with gradients to ``x0`` [M,S] and ``u``
    ([T-1,M,U], or one shared sequence [T-1,U] / [T-1,1,U]: its gradient has u's own shape, the sum over the trajectories).  The model is
    frozen.  When neither input requires grad nothing is recorded and the call IS ``rollout_open``.  Returns (states, status)."""
    for name, t in (("x0", x0), ("u", u)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("rollout_open_diff operates on GPU memory only (%s is not a GPU tensor); there is no CPU path" % name)
    if not (torch.is_grad_enabled() and (x0.requires_grad or u.requires_grad)):
        return rollout_open(model, x0.detach(), u.detach(), lengths=lengths, noise=noise, particle_pred=particle_pred, status=status)
    x0c, uc, _, lengths, noise, status = _open_operands(model, x0, u, None, lengths, noise, particle_pred, status)
    return RolloutOpenFunction.apply(x0c, uc, model, lengths, noise, bool(particle_pred), status), status


# --------------------------------------------------------------------------------------
# one fused model step (autograd): closed loops under a policy the fused rollouts do not know
# --------------------------------------------------------------------------------------
class ModelStepFunction(torch.autograd.Function):
    """(x [M,S], u [M,U]) -> x_next [M,S], mean [M,G], var [M,G] in one launch (mcp_model_step); the recording launch when an input requires grad,
    and then backward is the one launch of mcp_model_step_bwd over the record.  Gradients flow to x and u through x_next; the GP model is
    frozen and ``mean`` / ``var`` are not differentiated."""

    @staticmethod
    def forward(ctx, x, u, model, t, noise, particle_pred, moments, status):
        M, dev = int(x.shape[0]), model.device
        rec = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        x_next = torch.empty(M, model.S, dtype=DT, device=dev)
        mu = torch.empty(M, model.G, dtype=DT, device=dev) if moments else None
        var = torch.empty(M, model.G, dtype=DT, device=dev) if moments else None
        jac = torch.empty(M, model.G, model.D, dtype=DT, device=dev) if rec else None
        nz = noise.to_c()
        abi.check(abi.lib().mcp_model_step(_mc(model), C.byref(nz), M, int(t), int(bool(particle_pred)), abi.ptr(x), abi.ptr(u), abi.ptr(x_next),
                                           abi.ptr(mu), abi.ptr(var), abi.ptr(jac), abi.ptr(status), abi.stream()), "mcp_model_step")
        ctx.model = model
        if rec:
            ctx.save_for_backward(x, jac)
        if not moments:
            return x_next
        ctx.mark_non_differentiable(mu, var)
        return x_next, mu, var

    @staticmethod
    def backward(ctx, g_next, *_):
        x, jac = ctx.saved_tensors
        model, M = ctx.model, int(x.shape[0])
        g_x = torch.empty(M, model.S, dtype=DT, device=x.device) if ctx.needs_input_grad[0] else None
        g_u = torch.empty(M, model.U, dtype=DT, device=x.device) if ctx.needs_input_grad[1] else None
        gn = g_next.to(dtype=DT).contiguous()
        abi.check(abi.lib().mcp_model_step_bwd(_mc(model), M, abi.ptr(x), abi.ptr(jac), abi.ptr(gn), abi.ptr(g_x), abi.ptr(g_u), abi.stream()),
                  "mcp_model_step_bwd")
        return g_x, g_u, None, None, None, None, None, None


def model_step(model: PackedModel, x, u, t, noise: Optional[NoiseSpec] = None, particle_pred=True, moments=False, status=None):
    """One time step of the model in ONE launch: x [M,S], u [M,U] -> x_next [M,S], differentiable in x and u (the model is frozen), for a
    closed loop whose policy is evaluated in torch between the steps.  ``t``: the step's index in its rollout.  ``noise``: a NoiseSpec whose
    ``eps`` is THIS step's row [M,G], or Philox by seed / call / particle_offset and ``t`` -- a chain of steps carries the bits of
    ``rollout_open`` fed the same inputs.  ``particle_pred`` False: the posterior mean.  ``moments``: also the GP means and scaled variances
    [M,G] (what get_next_state returns; not differentiated).  ``status``: an int32[1] the kernels OR their flags into.
    Returns (x_next, status) or (x_next, mean, var, status)."""
    for name, a in (("x", x), ("u", u)):
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise RuntimeError("model_step operates on GPU memory only (%s is not a GPU tensor); there is no CPU path" % name)
    dev = model.device
    x, u = x.to(device=dev, dtype=DT).contiguous(), u.to(device=dev, dtype=DT).contiguous()
    if x.dim() != 2 or x.shape[1] != model.S or u.dim() != 2 or tuple(u.shape) != (x.shape[0], model.U) or x.shape[0] < 1:
        raise RuntimeError("model_step takes x [M,%d] and u [M,%d]" % (model.S, model.U))
    if int(t) < 0:
        raise RuntimeError("model_step: the step index must not be negative")
    noise = NoiseSpec() if noise is None else noise
    if particle_pred and noise.eps is not None:
        e = noise.eps
        if e.dtype != DT or not e.is_cuda or not e.is_contiguous() or tuple(e.shape) != (x.shape[0], model.G):
            raise RuntimeError("eps must be this step's row: a contiguous float64 GPU tensor of shape [M,G]")
    status = _status_word(status, dev, "the model's device")
    out = ModelStepFunction.apply(x, u, model, t, noise, bool(particle_pred), bool(moments), status)
    return (out[0], out[1], out[2], status) if moments else (out, status)


# --------------------------------------------------------------------------------------
# trajectory optimisation on the model: the dense linearisation of a record and the iLQR backward pass (no autograd)
# --------------------------------------------------------------------------------------
def _lqr_operands(dev, *named):
    """The tensors of ``named`` = (name, tensor or None, shape) as the trajectory-optimisation entries take them -- contiguous float64 of that
    shape on ``dev`` -- or ValueError: every dtype and shape is looked at first, then where the tensors live."""
    for name, t, shape in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != DT:
            raise ValueError("%s must be a float64 tensor" % name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have the shape %s, not %s" % (name, list(shape), list(t.shape)))
    for name, t, _ in named:
        if t is None:
            continue
        if not t.is_cuda or t.device != dev:
            raise ValueError("%s must be on the model's device %s, not on %s; there is no CPU path" % (name, dev, t.device))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    return [None if t is None else t.detach() for _, t, _ in named]


def _lqr_sizes(model, states):
    """(T, M) of a record's states [T,M,S]."""
    if not isinstance(states, torch.Tensor) or states.dim() != 3 or states.shape[0] < 2 or states.shape[1] < 1:
        raise ValueError("states must be a tensor [T,M,%d] with T >= 2 and M >= 1" % model.S)
    if int(states.shape[0]) > abi.LQR_MAX_T:
        raise ValueError("at most %d rows (got %d)" % (abi.LQR_MAX_T, int(states.shape[0])))
    return int(states.shape[0]), int(states.shape[1])


def rollout_open_record(model: PackedModel, x0, u, *, noise: Optional[NoiseSpec] = None, particle_pred=False, status=None):
    """The recording open-loop launch without autograd (mcp_rollout_open_rec): arguments of ``rollout_open`` (no ragged lengths) ->
    (states [T,M,S], jac [T-1,M,G,D], status) -- the operands of ``linearize`` and ``lqr_pass``.  The states carry the bits of
    ``rollout_open``; the mean form's record (``particle_pred`` False) is the nominal trajectory of the GP mean model."""
    for name, t in (("x0", x0), ("u", u)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("rollout_open_record operates on GPU memory only (%s is not a GPU tensor); there is no CPU path" % name)
    x0, u, T, _, noise, status = _open_operands(model, x0.detach(), u.detach(), None, None, noise, particle_pred, status)
    M = int(x0.shape[0])
    states, _, jac = _record_buffers(model.device, T, M, model.S, None, model.G, model.D, True)
    nz = noise.to_c()
    abi.check(abi.lib().mcp_rollout_open_rec(_mc(model), C.byref(nz), M, T, int(bool(particle_pred)), abi.ptr(x0), abi.ptr(u), int(u.shape[1]), None,
                                             abi.ptr(states), None, None, abi.ptr(jac), abi.ptr(status), abi.stream()), "mcp_rollout_open_rec")
    return states, jac, status


def linearize(model: PackedModel, states, jac, du_da=None, want=(True, True)):
    """Dense Jacobians of the model step along a recorded rollout in ONE launch (mcp_linearize): states [T,M,S] and jac [T-1,M,G,D] (the
    record of the recording open-loop or closed-loop launches; the mean form's is the nominal of the GP mean model) -> A [T-1,M,S,S],
    B [T-1,M,S,U] with x_{t+1} ~ A_t dx + B_t da.  ``du_da`` [T,M,U] scales B's columns (the derivative of the squashing at the nominal:
    B then refers to the pre-squash variable of ``TV_linear_controller``); None: ones.  ``want`` = (A, B): an output not wanted is None and
    is not computed.  No autograd.  ValueError for an operand of the wrong dtype, shape or device."""
    T, M = _lqr_sizes(model, states)
    states, jac, du_da = _lqr_operands(model.device, ("states", states, (T, M, model.S)), ("jac", jac, (T - 1, M, model.G, model.D)),
                                       ("du_da", du_da, (T, M, model.U)))
    A = torch.empty(T - 1, M, model.S, model.S, dtype=DT, device=model.device) if want[0] else None
    B = torch.empty(T - 1, M, model.S, model.U, dtype=DT, device=model.device) if want[1] else None
    abi.check(abi.lib().mcp_linearize(_mc(model), M, T, abi.ptr(states), abi.ptr(jac), abi.ptr(du_da), abi.ptr(A), abi.ptr(B), abi.stream()),
              "mcp_linearize")
    return A, B


def lqr_pass(model: PackedModel, states, jac, lx, lu, hxx, huu, reg=0.0, du_da=None, status=None):
    """The iLQR (Gauss-Newton) backward pass of M independent trajectories in ONE launch (mcp_lqr_pass): the record of ``linearize`` and the
    stage cost's expansion along it -- gradients lx [T,M,S], lu [T,M,U], diagonal Hessians hxx [T,M,S], huu [T,M,U], the input terms in the
    pre-squash variable when ``du_da`` is given -- -> (gain [M,T,U,S], kff [M,T,U], dv [M,2]).  gain[m] is a ``TV_linear_controller`` gain
    tensor: with the nominal states as its target the step is ff <- a_nominal + alpha kff[m], and alpha dv[m,0] + alpha^2 dv[m,1] / 2 is the
    predicted change of the cost.  ``reg`` >= 0 is added to the diagonal of Quu.  ``status``: an int32[1] the kernel ORs its flags into
    (MCP_STATUS_NOT_SPD: a pivot <= 0; MCP_STATUS_NAN: a non-finite operand or pivot) -- the outputs of such a trajectory are NaN, the
    others are unaffected (a caller that wants the flags passes its own word; ``dv`` is NaN exactly where a trajectory failed).  No autograd.
    ValueError for an operand of the wrong dtype, shape or device, or a reg that is negative or not finite."""
    T, M = _lqr_sizes(model, states)
    dev, xs, us = model.device, (T, M, model.S), (T, M, model.U)
    states, jac, du_da, lx, lu, hxx, huu = _lqr_operands(dev, ("states", states, xs), ("jac", jac, (T - 1, M, model.G, model.D)), ("du_da", du_da, us),
                                                         ("lx", lx, xs), ("lu", lu, us), ("hxx", hxx, xs), ("huu", huu, us))
    reg = float(reg)
    if not (0.0 <= reg < math.inf):
        raise ValueError("reg must be finite and not negative")
    status = _status_word(status, dev, "the model's device")
    gain = torch.empty(M, T, model.U, model.S, dtype=DT, device=dev)
    kff = torch.empty(M, T, model.U, dtype=DT, device=dev)
    dv = torch.empty(M, 2, dtype=DT, device=dev)
    abi.check(abi.lib().mcp_lqr_pass(_mc(model), M, T, abi.ptr(states), abi.ptr(jac), abi.ptr(du_da), abi.ptr(lx), abi.ptr(lu), abi.ptr(hxx),
                                     abi.ptr(huu), reg, abi.ptr(gain), abi.ptr(kff), abi.ptr(dv), abi.ptr(status), abi.stream()), "mcp_lqr_pass")
    return gain, kff, dv


# --------------------------------------------------------------------------------------
# sampling MPC on the model: the MPPI rollout-cost and update (no autograd)
# --------------------------------------------------------------------------------------
class PackedMPPI:
    """mcp_mppi without its device pointers (include/mcpilco_hip.h): ``K`` candidates x ``P`` model particles over ``H`` rows of ``U`` inputs,
    u = squash(a + sigma xi) with the closed-loop kernels' squashing (``u_max`` a scalar or one bound per input, > 0 with ``squash``),
    ``sigma`` (a scalar or one per input, >= 0) the std of the perturbation in the pre-squash variable, ``lam`` the temperature, ``kappa`` the
    weight of the particles' std in a candidate's cost (kappa != 0 needs P >= 2).  Everything is checked on the host values first: a bad
    descriptor raises ValueError before a device is touched.  ``to_c(a, xi, w, t0)`` binds the nominal [H,U], the perturbation buffer
    [H,K,U] (None: Philox), the time weights [H] (None: ones) and the row offset into the cost's target."""

    def __init__(self, K, P, H, U, sigma, lam, kappa=0.0, u_max=1.0, squash=True):
        K, P, H, U = int(K), int(P), int(H), int(U)
        if K < 1 or P < 1 or H < 2:
            raise ValueError("mppi: K >= 1 candidates, P >= 1 particles and H >= 2 rows are needed (K %d, P %d, H %d)" % (K, P, H))
        if not 1 <= U <= abi.MAX_INPUT:
            raise ValueError("mppi: 1..%d inputs are supported (%d given)" % (abi.MAX_INPUT, U))
        if K > abi.MPPI_MAX_K or K * P > abi.MPPI_MAX_M:
            raise ValueError("mppi: at most %d candidates and %d trajectories (K %d, K P %d)" % (abi.MPPI_MAX_K, abi.MPPI_MAX_M, K, K * P))
        per_input = lambda v, name: np.full(U, float(v)) if np.ndim(v) == 0 else _host(v).reshape(-1)
        sg, um = per_input(sigma, "sigma"), per_input(u_max, "u_max")
        if sg.size != U or um.size != U:
            raise ValueError("mppi: sigma and u_max hold one entry per input or are scalars")
        if not bool(np.all(np.isfinite(sg) & (sg >= 0))):
            raise ValueError("mppi: sigma must be finite and >= 0 (%s)" % (sg.tolist(),))
        if squash and not bool(np.all(um > 0)):
            raise ValueError("mppi: u_max must be > 0 with squashing (%s)" % (um.tolist(),))
        lam, kappa = float(lam), float(kappa)
        if not (0.0 < lam < math.inf):
            raise ValueError("mppi: the temperature lam must be finite and > 0 (%r)" % (lam,))
        if not np.isfinite(kappa) or (kappa != 0.0 and P < 2):
            raise ValueError("mppi: kappa must be finite, and kappa != 0 needs P >= 2 (kappa %r, P %d)" % (kappa, P))
        self.K, self.P, self.H, self.U, self.M = K, P, H, U, K * P
        self.sigma, self.u_max, self.lam, self.kappa, self.squash = sg, um, lam, kappa, bool(squash)

    def to_c(self, a, xi=None, w=None, t0=0):
        if int(t0) < 0:
            raise ValueError("mppi: t0 must be >= 0 (%d)" % int(t0))
        c = abi.MPPI()
        c.K, c.P, c.H, c.U, c.squash, c.lam, c.kappa, c.t0 = self.K, self.P, self.H, self.U, int(self.squash), self.lam, self.kappa, int(t0)
        for k in range(self.U):
            c.u_max[k], c.sigma[k] = float(self.u_max[k]), float(self.sigma[k])
        c.a = a.data_ptr()
        c.xi = None if xi is None else xi.data_ptr()
        c.w = None if w is None else w.data_ptr()
        return c


def _mppi_operands(mp, dev, a, xi, w):
    """a [H,U], xi [H,K,U] or None, w [H] or None as the planner's entries take them (the checks of ``_lqr_operands``)."""
    return _lqr_operands(dev, ("a", a, (mp.H, mp.U)), ("xi", xi, (mp.H, mp.K, mp.U)), ("w", w, (mp.H,)))


def mppi_rollout(model: PackedModel, mppi: PackedMPPI, cost: "PackedCost", x0, a, *, cost_inputs: Optional["PackedCostInputs"] = None,
                 noise: Optional[NoiseSpec] = None, particle_pred=False, xi=None, w=None, t0=0, want_states=False, want_inputs=False,
                 traj_cost=None, status=None):
    """The planner's rollout-cost in ONE launch (mcp_mppi_rollout): K P trajectories from the one state ``x0`` [S] under the inputs
    squash(a + sigma xi) -- candidate 0 unperturbed, ``xi`` [H,K,U] or Philox stream 3 of ``noise`` (seed, call) -- each reduced to
    traj_cost[k P + p] = sum_t w_t c(x_t, u_t, u_t-1) with ``cost`` / ``cost_inputs`` read at target row t0 + t.  ``particle_pred``: sampled
    increments with COMMON random numbers -- ``noise.eps`` is [H-1,P,G], Philox counts particle p -- else the mean model (P may be 1).
    ``want_states`` / ``want_inputs``: also [H,M,S] / [H,M,U] (tests, reading one plan's prediction back); without them nothing of that
    size is written.  ``traj_cost``: an output buffer [M] to reuse.  Returns (traj_cost, states or None, inputs or None, status).  No
    autograd.  ValueError for an operand of the wrong dtype, shape or device, or a trajectory cost shorter than t0 + H rows."""
    dev = model.device
    if mppi.U != model.U:
        raise ValueError("mppi: the plan has %d inputs, the model %d" % (mppi.U, model.U))
    a, xi, w = _mppi_operands(mppi, dev, a, xi, w)
    (x0,) = _lqr_operands(dev, ("x0", x0, (model.S,)))
    (traj_cost,) = _lqr_operands(dev, ("traj_cost", traj_cost, (mppi.M,)))
    if cost.kind == "traj" and cost.traj_len < int(t0) + mppi.H:
        raise ValueError("target trajectory has %d rows but the plan reads rows %d .. %d" % (cost.traj_len, int(t0), int(t0) + mppi.H - 1))
    if cost_inputs is not None and cost_inputs.U != model.U:
        raise ValueError("mppi: the input cost is over %d inputs, the model has %d" % (cost_inputs.U, model.U))
    noise = NoiseSpec() if noise is None else noise
    if particle_pred:
        _check_noise(noise, mppi.H, mppi.P, model.G, 0)
    status = _status_word(status, dev, "the model's device")
    if traj_cost is None:
        traj_cost = torch.empty(mppi.M, dtype=DT, device=dev)
    states = torch.empty(mppi.H, mppi.M, model.S, dtype=DT, device=dev) if want_states else None
    inputs = torch.empty(mppi.H, mppi.M, model.U, dtype=DT, device=dev) if want_inputs else None
    mc, nz = mppi.to_c(a, xi, w, t0), noise.to_c()
    abi.check(abi.lib().mcp_mppi_rollout(_mc(model), C.byref(mc), C.byref(cost.c), None if cost_inputs is None else C.byref(cost_inputs.c),
                                         C.byref(nz), int(bool(particle_pred)), abi.ptr(x0), abi.ptr(traj_cost), abi.ptr(states),
                                         abi.ptr(inputs), abi.ptr(status), abi.stream()), "mcp_mppi_rollout")
    return traj_cost, states, inputs, status


def mppi_update(mppi: PackedMPPI, traj_cost, a, *, noise: Optional[NoiseSpec] = None, xi=None, a_new=None, out=None, status=None):
    """The MPPI update in two small launches (mcp_mppi_update): candidate costs S_k = mean_p J + kappa std_p J, softmax weights
    exp(-(S_k - S_min) / lam) over the finite candidates, a_new = a + sigma sum_k w_k xi(k) with the perturbations REGENERATED (``xi``
    [H,K,U], or Philox stream 3 of ``noise``: the rollout's own).  ``a_new`` [H,U] (not ``a``) and ``out`` = (cand_cost [K], weights [K],
    stats [4]) are buffers to reuse.  Returns (a_new, cand_cost, weights, stats, status); stats = S_min, argmin k, the effective sample
    size 1 / sum w^2, sum_k w_k S_k.  A non-finite candidate gets weight 0 and raises MCP_STATUS_NAN in ``status``; with no finite
    candidate a_new = a.  Bitwise reproducible.  No autograd.  ValueError for an operand of the wrong dtype, shape or device."""
    if not isinstance(traj_cost, torch.Tensor):
        raise ValueError("traj_cost must be a float64 tensor")
    dev = traj_cost.device
    cand, wts, stats = (None, None, None) if out is None else out
    traj_cost, a, xi, a_new, cand, wts, stats = _lqr_operands(dev, ("traj_cost", traj_cost, (mppi.M,)), ("a", a, (mppi.H, mppi.U)),
                                                              ("xi", xi, (mppi.H, mppi.K, mppi.U)), ("a_new", a_new, (mppi.H, mppi.U)),
                                                              ("cand_cost", cand, (mppi.K,)), ("weights", wts, (mppi.K,)), ("stats", stats, (4,)))
    if a_new is not None and a_new.data_ptr() == a.data_ptr():
        raise ValueError("mppi: a_new must not be the nominal's own buffer")
    new = lambda *s: torch.empty(*s, dtype=DT, device=dev)
    a_new = new(mppi.H, mppi.U) if a_new is None else a_new
    cand, wts, stats = (new(mppi.K) if cand is None else cand), (new(mppi.K) if wts is None else wts), (new(4) if stats is None else stats)
    status = _status_word(status, dev, "the plan's device")
    noise = NoiseSpec() if noise is None else noise
    mc, nz = mppi.to_c(a, xi, None, 0), noise.to_c()
    abi.check(abi.lib().mcp_mppi_update(C.byref(mc), C.byref(nz), abi.ptr(traj_cost), abi.ptr(a_new), abi.ptr(cand), abi.ptr(wts), abi.ptr(stats),
                                        abi.ptr(status), abi.stream()), "mcp_mppi_update")
    return a_new, cand, wts, stats, status


class PackedPlanExt:
    """mcp_plan_ext without its device pointers (include/mcpilco_hip.h): the planner's extension over ``H`` rows of ``U`` inputs.  ``beta`` in
    [0, 1): the AR(1) coefficient of the perturbations (0: white); ``sigma_rows`` [H,U] HOST values (None: PackedMPPI's sigma for every row)
    -- a std per row and input, >= 0 and finite, uploaded once per device --; and what the CEM update alone reads: ``n_elite`` >= 1 (at most
    MCP_CEM_MAX_ELITE; against K when an entry sees the plan), the smoothing ``alpha`` in [0, 1), the floor ``sigma_min`` of the new std (a
    scalar or one per input, >= 0 and finite).  Everything is checked on the host values first: a bad descriptor raises ValueError before a
    device is touched.  ``to_c(dev, sigma_rows, u_prev)`` binds the std -- ``sigma_rows``: a DEVICE buffer [H,U] in place of this object's own,
    e.g. the CEM update's output, which the caller vouches for -- and the input applied before row 0 (device [U], or None)."""

    def __init__(self, H, U, beta=0.0, sigma_rows=None, n_elite=1, alpha=0.0, sigma_min=0.0):
        H, U = int(H), int(U)
        if H < 2 or not 1 <= U <= abi.MAX_INPUT:
            raise ValueError("plan ext: H >= 2 rows and 1..%d inputs are needed (H %d, U %d)" % (abi.MAX_INPUT, H, U))
        beta, alpha, n_elite = float(beta), float(alpha), int(n_elite)
        if not 0.0 <= beta < 1.0:
            raise ValueError("plan ext: the AR(1) coefficient beta must lie in [0, 1) (%r)" % (beta,))
        if not 0.0 <= alpha < 1.0:
            raise ValueError("plan ext: the smoothing alpha must lie in [0, 1) (%r)" % (alpha,))
        if not 1 <= n_elite <= abi.CEM_MAX_ELITE:
            raise ValueError("plan ext: 1..%d elites are supported (%d given)" % (abi.CEM_MAX_ELITE, n_elite))
        smin = np.full(U, float(sigma_min)) if np.ndim(sigma_min) == 0 else _host(sigma_min).reshape(-1)
        if smin.size != U or not bool(np.all(np.isfinite(smin) & (smin >= 0))):
            raise ValueError("plan ext: sigma_min holds one finite entry >= 0 per input or is such a scalar (%s)" % (smin.tolist(),))
        if sigma_rows is not None:
            sigma_rows = np.ascontiguousarray(_host(sigma_rows))
            if sigma_rows.shape != (H, U):
                raise ValueError("plan ext: sigma_rows must have the shape [%d, %d], not %s" % (H, U, list(sigma_rows.shape)))
            if not bool(np.all(np.isfinite(sigma_rows) & (sigma_rows >= 0))):
                raise ValueError("plan ext: every entry of sigma_rows must be finite and >= 0")
        self.H, self.U, self.beta, self.alpha, self.n_elite, self.sigma_min, self.sigma_rows = H, U, beta, alpha, n_elite, smin, sigma_rows
        self._dev = {}

    def rows_on(self, dev):
        """This object's own sigma_rows on ``dev`` (uploaded once), or None."""
        if self.sigma_rows is None:
            return None
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = _t(self.sigma_rows, dev)
        return self._dev[key]

    def to_c(self, dev, sigma_rows=None, u_prev=None):
        rows = self.rows_on(dev) if sigma_rows is None else sigma_rows
        c = abi.PlanExt()
        c.beta, c.alpha, c.n_elite = self.beta, self.alpha, self.n_elite
        for k in range(self.U):
            c.sigma_min[k] = float(self.sigma_min[k])
        c.sigma_rows = None if rows is None else rows.data_ptr()
        c.u_prev = None if u_prev is None else u_prev.data_ptr()
        c._keep = (rows, u_prev)  # (the buffers live as long as the descriptor)
        return c


def _ext_operands(ext, mp, dev, sigma_rows, u_prev):
    """The extension against the plan, its device operands checked: (ext or None, sigma_rows, u_prev)."""
    if ext is not None and (ext.H != mp.H or ext.U != mp.U):
        raise ValueError("plan ext: made for H %d, U %d, the plan has H %d, U %d" % (ext.H, ext.U, mp.H, mp.U))
    if ext is None and (sigma_rows is not None or u_prev is not None):
        ext = PackedPlanExt(mp.H, mp.U)
    sigma_rows, u_prev = _lqr_operands(dev, ("sigma_rows", sigma_rows, (mp.H, mp.U)), ("u_prev", u_prev, (mp.U,)))
    return ext, sigma_rows, u_prev


def plan_rollout(model: PackedModel, mppi: PackedMPPI, ext: Optional[PackedPlanExt], cost: "PackedCost", x0, a, *, sigma_rows=None, u_prev=None,
                 cost_inputs: Optional["PackedCostInputs"] = None, noise: Optional[NoiseSpec] = None, particle_pred=False, xi=None, w=None, t0=0,
                 want_states=False, want_inputs=False, traj_cost=None, status=None):
    """``mppi_rollout`` under the planner's extension (mcp_plan_rollout): inputs squash(a[t] + s(t) xi_t) with the std per row of ``ext`` --
    or of the DEVICE buffer ``sigma_rows`` [H,U] in its place -- and the perturbations coloured by ext.beta (``xi`` [H,K,U] holds the WHITE
    normals; the colouring happens in the kernel); ``u_prev`` (device [U], post-squash): the input applied before row 0, which the rate term
    at t = 0 is then taken against.  ``ext`` None and neither buffer given, or an ext with every field at its default: the launch of
    ``mppi_rollout``, bit for bit.  Everything else as ``mppi_rollout``."""
    dev = model.device
    if mppi.U != model.U:
        raise ValueError("mppi: the plan has %d inputs, the model %d" % (mppi.U, model.U))
    ext, sigma_rows, u_prev = _ext_operands(ext, mppi, dev, sigma_rows, u_prev)
    a, xi, w = _mppi_operands(mppi, dev, a, xi, w)
    (x0,) = _lqr_operands(dev, ("x0", x0, (model.S,)))
    (traj_cost,) = _lqr_operands(dev, ("traj_cost", traj_cost, (mppi.M,)))
    if cost.kind == "traj" and cost.traj_len < int(t0) + mppi.H:
        raise ValueError("target trajectory has %d rows but the plan reads rows %d .. %d" % (cost.traj_len, int(t0), int(t0) + mppi.H - 1))
    if cost_inputs is not None and cost_inputs.U != model.U:
        raise ValueError("mppi: the input cost is over %d inputs, the model has %d" % (cost_inputs.U, model.U))
    noise = NoiseSpec() if noise is None else noise
    if particle_pred:
        _check_noise(noise, mppi.H, mppi.P, model.G, 0)
    status = _status_word(status, dev, "the model's device")
    if traj_cost is None:
        traj_cost = torch.empty(mppi.M, dtype=DT, device=dev)
    states = torch.empty(mppi.H, mppi.M, model.S, dtype=DT, device=dev) if want_states else None
    inputs = torch.empty(mppi.H, mppi.M, model.U, dtype=DT, device=dev) if want_inputs else None
    mc, nz = mppi.to_c(a, xi, w, t0), noise.to_c()
    ec = None if ext is None else ext.to_c(dev, sigma_rows, u_prev)
    abi.check(abi.lib().mcp_plan_rollout(_mc(model), C.byref(mc), None if ec is None else C.byref(ec), C.byref(cost.c),
                                         None if cost_inputs is None else C.byref(cost_inputs.c), C.byref(nz), int(bool(particle_pred)),
                                         abi.ptr(x0), abi.ptr(traj_cost), abi.ptr(states), abi.ptr(inputs), abi.ptr(status), abi.stream()),
              "mcp_plan_rollout")
    return traj_cost, states, inputs, status


def mppi_update_ext(mppi: PackedMPPI, ext: Optional[PackedPlanExt], traj_cost, a, *, sigma_rows=None, noise: Optional[NoiseSpec] = None, xi=None,
                    a_new=None, out=None, status=None):
    """``mppi_update`` under the planner's extension (mcp_mppi_update_ext): a_new = a + s(t) sum_k w_k xi_t(k) with the std per row and the
    AR(1) colouring of ``ext`` (``sigma_rows``: a DEVICE buffer [H,U] in place of ext's own; ``xi`` holds the WHITE normals): the weighted
    sums of the white normals per row, then the filter over those H U sums.  A default ext (or None): ``mppi_update``, bit for bit.
    Returns (a_new, cand_cost, weights, stats, status) as ``mppi_update``."""
    if not isinstance(traj_cost, torch.Tensor):
        raise ValueError("traj_cost must be a float64 tensor")
    dev = traj_cost.device
    cand, wts, stats = (None, None, None) if out is None else out
    traj_cost, a, xi, a_new, cand, wts, stats = _lqr_operands(dev, ("traj_cost", traj_cost, (mppi.M,)), ("a", a, (mppi.H, mppi.U)),
                                                              ("xi", xi, (mppi.H, mppi.K, mppi.U)), ("a_new", a_new, (mppi.H, mppi.U)),
                                                              ("cand_cost", cand, (mppi.K,)), ("weights", wts, (mppi.K,)), ("stats", stats, (4,)))
    ext, sigma_rows, _ = _ext_operands(ext, mppi, dev, sigma_rows, None)
    if a_new is not None and a_new.data_ptr() == a.data_ptr():
        raise ValueError("mppi: a_new must not be the nominal's own buffer")
    new = lambda *s: torch.empty(*s, dtype=DT, device=dev)
    a_new = new(mppi.H, mppi.U) if a_new is None else a_new
    cand, wts, stats = (new(mppi.K) if cand is None else cand), (new(mppi.K) if wts is None else wts), (new(4) if stats is None else stats)
    status = _status_word(status, dev, "the plan's device")
    noise = NoiseSpec() if noise is None else noise
    mc, nz = mppi.to_c(a, xi, None, 0), noise.to_c()
    ec = None if ext is None else ext.to_c(dev, sigma_rows, None)
    abi.check(abi.lib().mcp_mppi_update_ext(C.byref(mc), None if ec is None else C.byref(ec), C.byref(nz), abi.ptr(traj_cost), abi.ptr(a_new),
                                            abi.ptr(cand), abi.ptr(wts), abi.ptr(stats), abi.ptr(status), abi.stream()), "mcp_mppi_update_ext")
    return a_new, cand, wts, stats, status


def cem_update(mppi: PackedMPPI, ext: PackedPlanExt, traj_cost, a, *, sigma_rows=None, noise: Optional[NoiseSpec] = None, xi=None, a_new=None,
               sigma_new=None, out=None, status=None):
    """The CEM update in two small launches (mcp_cem_update): candidate costs as ``mppi_update``; the elites are the E' = min(ext.n_elite,
    #finite) candidates with the smallest (S_k, k), selected and ranked on the device; with the perturbations REGENERATED for the elites
    alone (``xi`` [H,K,U] white normals or Philox stream 3 of ``noise``, coloured by ext.beta), m and v their mean and (two-pass, 1 / E')
    variance per row and input, a_new = alpha a + (1 - alpha)(a + s m) and sigma_new = max(sigma_min, sqrt(alpha s^2 + (1 - alpha) s^2 v))
    around the current std s of ``ext`` (``sigma_rows``: a DEVICE buffer [H,U] in its place).  ``a_new``, ``sigma_new`` [H,U] (neither of
    them ``a`` or the std's buffer) and ``out`` = (cand_cost [K], elite int32 [n_elite], stats [4]) are buffers to reuse.  Returns (a_new,
    sigma_new, cand_cost, elite, stats, status); elite holds -1 behind the E' used, stats = S_min, argmin k, E', the elites' mean cost.
    With no finite candidate a_new = a and sigma_new = s.  Bitwise reproducible.  No autograd."""
    if not isinstance(traj_cost, torch.Tensor):
        raise ValueError("traj_cost must be a float64 tensor")
    if ext is None:
        raise ValueError("cem: a PackedPlanExt (n_elite, alpha, sigma_min) is needed")
    if ext.n_elite > mppi.K:
        raise ValueError("cem: %d elites of %d candidates" % (ext.n_elite, mppi.K))
    dev = traj_cost.device
    cand, elite, stats = (None, None, None) if out is None else out
    traj_cost, a, xi, a_new, sigma_new, cand, stats = _lqr_operands(dev, ("traj_cost", traj_cost, (mppi.M,)), ("a", a, (mppi.H, mppi.U)),
                                                                    ("xi", xi, (mppi.H, mppi.K, mppi.U)), ("a_new", a_new, (mppi.H, mppi.U)),
                                                                    ("sigma_new", sigma_new, (mppi.H, mppi.U)), ("cand_cost", cand, (mppi.K,)),
                                                                    ("stats", stats, (4,)))
    ext, sigma_rows, _ = _ext_operands(ext, mppi, dev, sigma_rows, None)
    if elite is not None and (not isinstance(elite, torch.Tensor) or elite.dtype != torch.int32 or tuple(elite.shape) != (ext.n_elite,)
                              or elite.device != dev or not elite.is_contiguous()):
        raise ValueError("elite must be a contiguous int32 tensor [%d] on the plan's device" % ext.n_elite)
    ec = ext.to_c(dev, sigma_rows, None)
    taken = {a.data_ptr()} | ({ec._keep[0].data_ptr()} if ec._keep[0] is not None else set())
    outs = [t.data_ptr() for t in (a_new, sigma_new) if t is not None]
    if any(p in taken for p in outs) or len(set(outs)) != len(outs):
        raise ValueError("cem: a_new and sigma_new are buffers of their own, neither the nominal's nor the std's")
    new = lambda *s: torch.empty(*s, dtype=DT, device=dev)
    a_new, sigma_new = (new(mppi.H, mppi.U) if a_new is None else a_new), (new(mppi.H, mppi.U) if sigma_new is None else sigma_new)
    cand, stats = (new(mppi.K) if cand is None else cand), (new(4) if stats is None else stats)
    elite = torch.empty(ext.n_elite, dtype=torch.int32, device=dev) if elite is None else elite
    status = _status_word(status, dev, "the plan's device")
    noise = NoiseSpec() if noise is None else noise
    mc, nz = mppi.to_c(a, xi, None, 0), noise.to_c()
    abi.check(abi.lib().mcp_cem_update(C.byref(mc), C.byref(ec), C.byref(nz), abi.ptr(traj_cost), abi.ptr(a_new), abi.ptr(sigma_new), abi.ptr(cand),
                                       abi.ptr(elite), abi.ptr(stats), abi.ptr(status), abi.stream()), "mcp_cem_update")
    return a_new, sigma_new, cand, elite, stats, status


# --------------------------------------------------------------------------------------
# the batched planner: B plans of one shape in the launches of one (no autograd)
# --------------------------------------------------------------------------------------
class PackedPlanBatch:
    """mcp_plan_batch without its buffer strides (include/mcpilco_hip.h): ``B`` problems of ``P`` model particles per candidate each.
    ``x0_per_particle``: the start states are [B,P,S], trajectory k P + p of problem b starts at x0[b,p] (else [B,S]); ``particle_stride``
    >= 0: problem b draws both Philox streams as the single-problem entry does at ``noise.particle_offset + b * particle_stride`` (0: common
    random numbers across the problems).  Checked on the host values first: ValueError before a device is touched.  ``to_c(xi_stride,
    eps_stride)``: the doubles between the problems' xi / eps buffers (0: one buffer for all)."""

    def __init__(self, B, P, x0_per_particle=False, particle_stride=0):
        if isinstance(particle_stride, float) and not float(particle_stride).is_integer():
            raise ValueError("plan batch: particle_stride is a whole number (%r)" % (particle_stride,))
        B, P, stride = int(B), int(P), int(particle_stride)
        if not 1 <= B <= abi.PLAN_MAX_B:
            raise ValueError("plan batch: 1..%d problems are supported (%d given)" % (abi.PLAN_MAX_B, B))
        if P < 1 or B * P > abi.MPPI_MAX_M:
            raise ValueError("plan batch: P >= 1 particles, and at most %d trajectories over all problems (P %d, B P %d)" % (abi.MPPI_MAX_M, P, B * P))
        if not 0 <= stride < 2 ** 40:
            raise ValueError("plan batch: particle_stride must be >= 0 and below 2^40, the range of a particle id (%d)" % stride)
        self.B, self.P, self.x0_per_particle, self.particle_stride = B, P, bool(x0_per_particle), stride

    def to_c(self, xi_stride=0, eps_stride=0):
        c = abi.PlanBatch()
        c.B, c.x0_per_particle, c.particle_stride, c.xi_stride, c.eps_stride = self.B, int(self.x0_per_particle), self.particle_stride, int(xi_stride), int(eps_stride)
        return c


def _batch_plan(bt, mp):
    if not isinstance(bt, PackedPlanBatch):
        raise ValueError("plan batch: a PackedPlanBatch is needed")
    if bt.P != mp.P:
        raise ValueError("plan batch: made for P %d, the plan has P %d" % (bt.P, mp.P))
    if bt.B * mp.M > abi.MPPI_MAX_M:
        raise ValueError("plan batch: at most %d trajectories over all problems (B K P %d)" % (abi.MPPI_MAX_M, bt.B * mp.M))


def _batch_shared(t, one, B):
    """(shape to check ``t`` against, stride in doubles between the problems) of a buffer that is one for all problems (``one``) or one per
    problem ([B] + one)."""
    if isinstance(t, torch.Tensor) and t.dim() == len(one) + 1:
        return (B,) + tuple(one), int(np.prod(one))
    return tuple(one), 0


def _batch_status(status, dev, B, where):
    if status is None:
        return torch.zeros(B, dtype=torch.int32, device=dev)
    if not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or tuple(status.shape) != (B,) or status.device != dev or not status.is_contiguous():
        raise ValueError("status must be a contiguous int32 tensor [%d] on %s" % (B, where))
    return status


def _batch_ext(ext, mp, bt, dev, sigma_rows, u_prev):
    """``_ext_operands`` for B problems: sigma_rows [B,H,U] and u_prev [B,U] on the device -- an ext's own host rows [H,U] are every
    problem's."""
    if ext is not None and (ext.H != mp.H or ext.U != mp.U):
        raise ValueError("plan ext: made for H %d, U %d, the plan has H %d, U %d" % (ext.H, ext.U, mp.H, mp.U))
    if ext is None and (sigma_rows is not None or u_prev is not None):
        ext = PackedPlanExt(mp.H, mp.U)
    sigma_rows, u_prev = _lqr_operands(dev, ("sigma_rows", sigma_rows, (bt.B, mp.H, mp.U)), ("u_prev", u_prev, (bt.B, mp.U)))
    if ext is not None and sigma_rows is None and ext.sigma_rows is not None:
        sigma_rows = ext.rows_on(dev).unsqueeze(0).repeat(bt.B, 1, 1)
    return ext, sigma_rows, u_prev


def plan_batch_rollout(model: PackedModel, mppi: PackedMPPI, ext: Optional[PackedPlanExt], batch: PackedPlanBatch, cost: "PackedCost", x0, a, *,
                       sigma_rows=None, u_prev=None, cost_inputs: Optional["PackedCostInputs"] = None, noise: Optional[NoiseSpec] = None,
                       particle_pred=False, xi=None, w=None, t0=0, want_states=False, want_inputs=False, traj_cost=None, status=None):
    """``plan_rollout`` for ``batch.B`` problems in ONE launch (mcp_plan_batch_rollout): ``x0`` [B,S] (or [B,P,S] with
    batch.x0_per_particle), ``a`` [B,H,U], ``sigma_rows`` [B,H,U] and ``u_prev`` [B,U] on the device; ``xi`` [H,K,U] (one buffer for all) or
    [B,H,K,U]; ``noise.eps`` [H-1,P,G] or [B,H-1,P,G]; model, cost, ``w``, ``t0`` and the plan's scalars are shared.  Problem b's slices
    carry the bits of ``plan_rollout`` on its operands with noise.particle_offset + b * batch.particle_stride.  Returns (traj_cost [B,K P],
    states [B,H,K P,S] or None, inputs [B,H,K P,U] or None, status int32 [B] -- one word per problem).  No autograd.  ValueError for an
    operand of the wrong dtype, shape or device."""
    dev = model.device
    if mppi.U != model.U:
        raise ValueError("mppi: the plan has %d inputs, the model %d" % (mppi.U, model.U))
    _batch_plan(batch, mppi)
    B = batch.B
    ext, sigma_rows, u_prev = _batch_ext(ext, mppi, batch, dev, sigma_rows, u_prev)
    xi_shape, xi_stride = _batch_shared(xi, (mppi.H, mppi.K, mppi.U), B)
    a, xi, w, x0, traj_cost = _lqr_operands(dev, ("a", a, (B, mppi.H, mppi.U)), ("xi", xi, xi_shape), ("w", w, (mppi.H,)),
                                            ("x0", x0, (B, mppi.P, model.S) if batch.x0_per_particle else (B, model.S)),
                                            ("traj_cost", traj_cost, (B, mppi.M)))
    if cost.kind == "traj" and cost.traj_len < int(t0) + mppi.H:
        raise ValueError("target trajectory has %d rows but the plan reads rows %d .. %d" % (cost.traj_len, int(t0), int(t0) + mppi.H - 1))
    if cost_inputs is not None and cost_inputs.U != model.U:
        raise ValueError("mppi: the input cost is over %d inputs, the model has %d" % (cost_inputs.U, model.U))
    noise = NoiseSpec() if noise is None else noise
    eps_stride = 0
    if particle_pred and noise.eps is not None:
        eps_shape, eps_stride = _batch_shared(noise.eps, (mppi.H - 1, mppi.P, model.G), B)
        _lqr_operands(dev, ("noise.eps", noise.eps, eps_shape))
    status = _batch_status(status, dev, B, "the model's device")
    if traj_cost is None:
        traj_cost = torch.empty(B, mppi.M, dtype=DT, device=dev)
    states = torch.empty(B, mppi.H, mppi.M, model.S, dtype=DT, device=dev) if want_states else None
    inputs = torch.empty(B, mppi.H, mppi.M, model.U, dtype=DT, device=dev) if want_inputs else None
    mc, nz, bc = mppi.to_c(a, xi, w, t0), noise.to_c(), batch.to_c(xi_stride, eps_stride)
    ec = None if ext is None else ext.to_c(dev, sigma_rows, u_prev)
    abi.check(abi.lib().mcp_plan_batch_rollout(_mc(model), C.byref(mc), None if ec is None else C.byref(ec), C.byref(bc), C.byref(cost.c),
                                               None if cost_inputs is None else C.byref(cost_inputs.c), C.byref(nz), int(bool(particle_pred)),
                                               abi.ptr(x0), abi.ptr(traj_cost), abi.ptr(states), abi.ptr(inputs), abi.ptr(status), abi.stream()),
              "mcp_plan_batch_rollout")
    return traj_cost, states, inputs, status


def _batch_update_operands(mppi, batch, traj_cost, a, xi, named):
    """The operands every batched update shares, checked: (dev, xi_stride, [traj_cost, a, xi] + the tensors of ``named``)."""
    if not isinstance(traj_cost, torch.Tensor):
        raise ValueError("traj_cost must be a float64 tensor")
    _batch_plan(batch, mppi)
    dev, B = traj_cost.device, batch.B
    xi_shape, xi_stride = _batch_shared(xi, (mppi.H, mppi.K, mppi.U), B)
    return dev, xi_stride, _lqr_operands(dev, ("traj_cost", traj_cost, (B, mppi.M)), ("a", a, (B, mppi.H, mppi.U)), ("xi", xi, xi_shape), *named)


def plan_batch_update(mppi: PackedMPPI, ext: Optional[PackedPlanExt], batch: PackedPlanBatch, traj_cost, a, *, sigma_rows=None,
                      noise: Optional[NoiseSpec] = None, xi=None, a_new=None, out=None, status=None):
    """``mppi_update_ext`` for ``batch.B`` problems (mcp_plan_batch_update; two launches, three under a std per row or beta != 0):
    ``traj_cost`` [B,K P], ``a`` [B,H,U], ``sigma_rows`` [B,H,U] on the device, ``xi`` [H,K,U] or [B,H,K,U]; ``a_new`` [B,H,U] and ``out`` =
    (cand_cost [B,K], weights [B,K], stats [B,4]) are buffers to reuse.  Returns (a_new, cand_cost, weights, stats, status int32 [B]); problem
    b's slices carry the bits of ``mppi_update_ext`` on its operands.  No autograd."""
    B = batch.B if isinstance(batch, PackedPlanBatch) else 0
    cand, wts, stats = (None, None, None) if out is None else out
    dev, xi_stride, (traj_cost, a, xi, a_new, cand, wts, stats) = _batch_update_operands(
        mppi, batch, traj_cost, a, xi, (("a_new", a_new, (B, mppi.H, mppi.U)), ("cand_cost", cand, (B, mppi.K)), ("weights", wts, (B, mppi.K)),
                                        ("stats", stats, (B, 4))))
    ext, sigma_rows, _ = _batch_ext(ext, mppi, batch, dev, sigma_rows, None)
    if a_new is not None and a_new.data_ptr() == a.data_ptr():
        raise ValueError("mppi: a_new must not be the nominal's own buffer")
    new = lambda *s: torch.empty(*s, dtype=DT, device=dev)
    a_new = new(B, mppi.H, mppi.U) if a_new is None else a_new
    cand, wts, stats = (new(B, mppi.K) if cand is None else cand), (new(B, mppi.K) if wts is None else wts), (new(B, 4) if stats is None else stats)
    status = _batch_status(status, dev, B, "the plan's device")
    noise = NoiseSpec() if noise is None else noise
    mc, nz, bc = mppi.to_c(a, xi, None, 0), noise.to_c(), batch.to_c(xi_stride, 0)
    ec = None if ext is None else ext.to_c(dev, sigma_rows, None)
    abi.check(abi.lib().mcp_plan_batch_update(C.byref(mc), None if ec is None else C.byref(ec), C.byref(bc), C.byref(nz), abi.ptr(traj_cost),
                                              abi.ptr(a_new), abi.ptr(cand), abi.ptr(wts), abi.ptr(stats), abi.ptr(status), abi.stream()),
              "mcp_plan_batch_update")
    return a_new, cand, wts, stats, status


def cem_batch_update(mppi: PackedMPPI, ext: PackedPlanExt, batch: PackedPlanBatch, traj_cost, a, *, sigma_rows=None, noise: Optional[NoiseSpec] = None,
                     xi=None, a_new=None, sigma_new=None, out=None, status=None):
    """``cem_update`` for ``batch.B`` problems (mcp_cem_batch_update; two launches): ``traj_cost`` [B,K P], ``a`` [B,H,U], ``sigma_rows``
    [B,H,U] on the device (None: the ext's own rows, or the plan's sigma, for every problem); ``a_new``, ``sigma_new`` [B,H,U] and ``out`` =
    (cand_cost [B,K], elite int32 [B,n_elite], stats [B,4]) are buffers to reuse.  Returns (a_new, sigma_new, cand_cost, elite, stats, status
    int32 [B]); problem b's slices carry the bits of ``cem_update`` on its operands.  No autograd."""
    if ext is None:
        raise ValueError("cem: a PackedPlanExt (n_elite, alpha, sigma_min) is needed")
    if ext.n_elite > mppi.K:
        raise ValueError("cem: %d elites of %d candidates" % (ext.n_elite, mppi.K))
    B = batch.B if isinstance(batch, PackedPlanBatch) else 0
    cand, elite, stats = (None, None, None) if out is None else out
    dev, xi_stride, (traj_cost, a, xi, a_new, sigma_new, cand, stats) = _batch_update_operands(
        mppi, batch, traj_cost, a, xi, (("a_new", a_new, (B, mppi.H, mppi.U)), ("sigma_new", sigma_new, (B, mppi.H, mppi.U)),
                                        ("cand_cost", cand, (B, mppi.K)), ("stats", stats, (B, 4))))
    ext, sigma_rows, _ = _batch_ext(ext, mppi, batch, dev, sigma_rows, None)
    if elite is not None and (not isinstance(elite, torch.Tensor) or elite.dtype != torch.int32 or tuple(elite.shape) != (B, ext.n_elite)
                              or elite.device != dev or not elite.is_contiguous()):
        raise ValueError("elite must be a contiguous int32 tensor [%d, %d] on the plan's device" % (B, ext.n_elite))
    ec = ext.to_c(dev, sigma_rows, None)
    taken = {a.data_ptr()} | ({ec._keep[0].data_ptr()} if ec._keep[0] is not None else set())
    outs = [t.data_ptr() for t in (a_new, sigma_new) if t is not None]
    if any(p in taken for p in outs) or len(set(outs)) != len(outs):
        raise ValueError("cem: a_new and sigma_new are buffers of their own, neither the nominal's nor the std's")
    new = lambda *s: torch.empty(*s, dtype=DT, device=dev)
    a_new, sigma_new = (new(B, mppi.H, mppi.U) if a_new is None else a_new), (new(B, mppi.H, mppi.U) if sigma_new is None else sigma_new)
    cand, stats = (new(B, mppi.K) if cand is None else cand), (new(B, 4) if stats is None else stats)
    elite = torch.empty(B, ext.n_elite, dtype=torch.int32, device=dev) if elite is None else elite
    status = _batch_status(status, dev, B, "the plan's device")
    noise = NoiseSpec() if noise is None else noise
    mc, nz, bc = mppi.to_c(a, xi, None, 0), noise.to_c(), batch.to_c(xi_stride, 0)
    abi.check(abi.lib().mcp_cem_batch_update(C.byref(mc), C.byref(ec), C.byref(bc), C.byref(nz), abi.ptr(traj_cost), abi.ptr(a_new),
                                             abi.ptr(sigma_new), abi.ptr(cand), abi.ptr(elite), abi.ptr(stats), abi.ptr(status), abi.stream()),
              "mcp_cem_batch_update")
    return a_new, sigma_new, cand, elite, stats, status


# --------------------------------------------------------------------------------------
# fused closed loop under a feedback policy (autograd): the PD law, the tanh MLP
# --------------------------------------------------------------------------------------
# What the one host path below (_closed_launch, _closed_sweep, RolloutClosedFunction, _rollout_closed) reads of a packed policy:
#   params         the policy's own parameter tensors (where they live is checked); tensors(): the LIVE tensors one launch takes, to_c(*tensors)
#                  its descriptor over them, shapes: their shapes -- a sweep's raw gradient buffer, summed over its rows, is cut in this order
#   fwd, bwd       the C entries (plain, measured) of the rollout and of the sweep; fwd_outputs: the order of the forward entry's output
#                  pointers between ``inputs`` and ``status`` -- the two policies' entries differ there, and only there
#   grad_tile, grad_shape   the raw parameter-gradient buffer of a sweep is [ceil(M / grad_tile)] + grad_shape
#   fwd_drop, bwd_drop, drop_width   (a policy with dropout) the entries that take the probability -- and a measurement model or NULL, and
#                  in the sweep the noise -- and the width of a row of its masks
#   fwd_track, bwd_track, track_c()   (a policy that can track) the entries that take an mcp_mlp_track ahead of the dropout entries' arguments,
#                  and the track itself -- None: the policy has no target, and the calls are the ones above
#   fwd_res, bwd_res, res_c()   (a policy that can carry a PD term) the entries that take an mcp_mlp_pd behind the track, and the term itself --
#                  None: the policy has none, and the calls are the ones above
#   fwd_hist, bwd_hist, hist_c(), history   (a policy with memory, ``history`` > 1) the entries that take an mcp_mlp_hist behind the policy and
#                  ahead of the track, and the depth itself -- ``history`` == 1: the calls are the ones above
#   fwd_pid, bwd_pid, term_c(integ)   (a policy with the integral term) the ONE pair of entries that take an mcp_pid_term behind the policy and
#                  a measurement model or NULL behind that, and the term over a launch's buffer ``integ`` [T,M,U] -- which the launch
#                  allocates, leaves in ``packed.integ`` and the Function saves for the sweep like the measurement buffer
#   check(model, T)   the policy's own refusals
class PackedPD:
    """mcp_pd_policy of a ``Policy.PD_controller`` (reference policy_learning/Policy.py:406-449): the two gain parameters are kept as they
    are -- every launch takes views of the LIVE tensors, so an optimizer's in-place updates are seen -- and the target trajectory is held
    on the device.  The reference's index layout: input k reads the errors of position k and of velocity h + k, h = S / 2."""

    fwd, bwd = ("mcp_rollout_pd", "mcp_rollout_pd_meas"), ("mcp_rollout_pd_bwd", "mcp_rollout_pd_meas_bwd")
    fwd_outputs = ("jac", "mu", "var")
    grad_tile = 1  # one row of gain gradients per trajectory

    def __init__(self, policy):
        self.sqrt_kp, self.sqrt_kd = policy.sqrt_Kp_gains, policy.sqrt_Kd_gains
        self.params = [self.sqrt_kp, self.sqrt_kd]
        self.S, self.U = int(policy.state_dim), int(policy.input_dim)
        self.shapes, self.grad_shape = [(self.U,), (self.U,)], (2, self.U)
        dev = _dev(self.sqrt_kp.device)
        if policy.target_traj is None:
            raise RuntimeError("the PD controller has no target trajectory")
        self.target_traj = _t(policy.target_traj, dev).reshape(-1, self.S).contiguous()
        h = self.S // 2
        self.pos, self.vel = list(range(self.U)), list(range(h, h + self.U))
        self.squash = bool(policy.flg_squash)
        self.u_max = np.full(self.U, float(policy.u_max)) if np.isscalar(policy.u_max) else np.asarray(policy.u_max, dtype=np.float64).reshape(-1)
        if self.u_max.size != self.U or self.U > abi.MAX_INPUT:
            raise RuntimeError("u_max must be a scalar or hold one bound per input (at most %d inputs)" % abi.MAX_INPUT)
        self.device = dev

    def gains(self):
        """(sqrt_kp, sqrt_kd) as [U] tensors on the autograd graph of the parameters: views, or a scalar gain expanded to every input."""
        out = []
        for g in (self.sqrt_kp, self.sqrt_kd):
            g = g.reshape(-1)
            if g.numel() == 1 and self.U > 1:
                g = g.expand(self.U)
            if g.numel() != self.U:
                raise RuntimeError("the PD gains must hold one value per input (or one for all)")
            out.append(g)
        return out

    tensors = gains

    def check(self, model, T):
        if self.S != model.S or self.U != model.U:
            raise RuntimeError("the PD controller is for %d states and %d inputs, the model has %d and %d" % (self.S, self.U, model.S, model.U))
        if T < 1 or self.target_traj.shape[0] < T:
            raise RuntimeError("the target trajectory has %d rows, the rollout needs %d" % (self.target_traj.shape[0], T))

    def to_c(self, kp, kd):
        """The descriptor over the gains (kp, kd): contiguous float64 GPU tensors [U]."""
        for t in (kp, kd):
            if t.dtype != DT or not t.is_cuda or not t.is_contiguous() or t.numel() != self.U:
                raise RuntimeError("the PD gains must be contiguous float64 GPU tensors with one value per input")
        c = abi.PDPolicy()
        c.U, c.squash = self.U, int(self.squash)
        for k in range(self.U):
            c.pos[k], c.vel[k], c.u_max[k] = self.pos[k], self.vel[k], float(self.u_max[k])
        c.sqrt_kp, c.sqrt_kd = kp.data_ptr(), kd.data_ptr()
        c.target_traj, c.target_rows = self.target_traj.data_ptr(), int(self.target_traj.shape[0])
        return c


class PackedPID(PackedPD):
    """mcp_pd_policy and mcp_pid_term of a ``Policy.PID_controller``: PackedPD with the third gain parameter ``sqrt_Ki_gains`` behind the two,
    the step ``dt`` (the class passes T_sampling) and the bound ``i_max`` of the integral per input (inf: no clamp).  ``integ`` is the
    integral I [T,M,U] of the LAST launch made through this object (not differentiable; the recording launch's is saved with the record)."""

    fwd_pid, bwd_pid = "mcp_rollout_pid", "mcp_rollout_pid_bwd"

    def __init__(self, policy):
        super().__init__(policy)
        self.sqrt_ki = policy.sqrt_Ki_gains
        self.params = [self.sqrt_kp, self.sqrt_kd, self.sqrt_ki]
        self.shapes, self.grad_shape = [(self.U,)] * 3, (3, self.U)
        self.dt = float(policy.T_sampling)
        im = policy.i_max
        self.i_max = np.full(self.U, np.inf if im is None else float(im)) if (im is None or np.isscalar(im)) else np.asarray(im, dtype=np.float64).reshape(-1)
        if self.i_max.size != self.U:
            raise RuntimeError("i_max must be None, a scalar or hold one bound per input")
        if not self.dt > 0.0 or not bool(np.all(self.i_max > 0.0)):
            raise RuntimeError("the integral term needs T_sampling > 0 and every i_max > 0 (inf: no clamp)")
        self.integ = None

    def gains(self):
        """(sqrt_kp, sqrt_kd, sqrt_ki) as [U] tensors on the autograd graph of the parameters, as PackedPD.gains has the two."""
        g = self.sqrt_ki.reshape(-1)
        if g.numel() == 1 and self.U > 1:
            g = g.expand(self.U)
        if g.numel() != self.U:
            raise RuntimeError("the PID gains must hold one value per input (or one for all)")
        return super().gains() + [g]

    tensors = gains

    def to_c(self, kp, kd, ki):
        """The PD descriptor over (kp, kd); the integral gain of this launch is kept for ``term_c``."""
        if ki.dtype != DT or not ki.is_cuda or not ki.is_contiguous() or ki.numel() != self.U:
            raise RuntimeError("the PID gains must be contiguous float64 GPU tensors with one value per input")
        self._ki = ki
        return super().to_c(kp, kd)

    def term_c(self, integ):
        """The mcp_pid_term over the integral gain handed to ``to_c`` and the buffer ``integ`` [T,M,U]."""
        c = abi.PIDTerm()
        c.on, c.sqrt_ki, c.dt, c.integ = 1, self._ki.data_ptr(), self.dt, integ.data_ptr()
        for k in range(self.U):
            c.i_max[k] = float(self.i_max[k])
        return c


class PackedTVL:
    """mcp_tvl_policy of a ``Policy.TV_linear_controller``: the LIVE tensors ``gain`` ([rows, U, S], or [U, S] shared by every row) and
    ``ff`` ([rows, U], or None) are kept as they are -- every launch reads them where they lie, so an optimizer's in-place updates are seen --
    and the target trajectory is held on the device.  The sweep leaves one partial [T, U, S + 1] per workgroup of ``grad_tile``
    trajectories; ``split_grad`` adds them (and the rows, for a shared gain) and cuts the sum into the two tensors' shapes."""

    fwd, bwd = ("mcp_rollout_tvl",) * 2, ("mcp_rollout_tvl_bwd",) * 2
    meas_slot = True  # (one entry for both forms: the measurement model or NULL always stands between the policy and the rest)
    fwd_outputs = ("jac", "mu", "var")
    grad_tile = 16  # one partial per workgroup of the sweep

    def __init__(self, policy):
        self.gain, self.ff = policy.gain, policy.ff
        self.params = [self.gain] + ([self.ff] if self.ff is not None else [])
        self.S, self.U = int(policy.state_dim), int(policy.input_dim)
        self.shared = self.gain.dim() == 2
        if tuple(self.gain.shape[-2:]) != (self.U, self.S) or self.gain.dim() not in (2, 3):
            raise RuntimeError("the gain must be [rows, U, S] or [U, S]")
        if self.ff is not None and (self.ff.dim() != 2 or int(self.ff.shape[1]) != self.U):
            raise RuntimeError("the feedforward must be [rows, U]")
        self.shapes = [tuple(q.shape) for q in self.params]
        dev = _dev(self.gain.device)
        if policy.target_traj is None:
            raise RuntimeError("the controller has no target trajectory")
        self.target_traj = _t(policy.target_traj, dev).reshape(-1, self.S).contiguous()
        self.squash = bool(policy.flg_squash)
        self.u_max = np.full(self.U, float(policy.u_max)) if np.isscalar(policy.u_max) else np.asarray(policy.u_max, dtype=np.float64).reshape(-1)
        if self.u_max.size != self.U or self.U > abi.MAX_INPUT or self.S > abi.MAX_STATE:
            raise RuntimeError("u_max must be a scalar or hold one bound per input (at most %d inputs, %d states)" % (abi.MAX_INPUT, abi.MAX_STATE))
        self.device = dev

    def tensors(self):
        return self.params

    def grad_shape_of(self, T):
        return (int(T), self.U, self.S + 1)  # (the sweep's partial has one row per policy evaluation)

    def check(self, model, T):
        if self.S != model.S or self.U != model.U:
            raise RuntimeError("the controller is for %d states and %d inputs, the model has %d and %d" % (self.S, self.U, model.S, model.U))
        rows = [int(self.target_traj.shape[0])] + ([] if self.shared else [int(self.gain.shape[0])]) + ([int(self.ff.shape[0])] if self.ff is not None else [])
        if T < 1 or min(rows) < T:
            raise RuntimeError("the gain, the feedforward and the target trajectory must have at least %d rows (have %s)" % (T, rows))

    def to_c(self, gain, ff=None):
        """The descriptor over (gain, ff): contiguous float64 GPU tensors of the parameters' shapes."""
        for t, shp in zip((gain, ff), self.shapes):
            if t.dtype != DT or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shp:
                raise RuntimeError("the gain and the feedforward must be contiguous float64 GPU tensors of their declared shapes")
        c = abi.TVLPolicy()
        c.U, c.S, c.squash = self.U, self.S, int(self.squash)
        c.gain_rows = 1 if self.shared else int(gain.shape[0])
        c.ff_rows = 0 if ff is None else int(ff.shape[0])
        c.target_rows = int(self.target_traj.shape[0])
        for k in range(self.U):
            c.u_max[k] = float(self.u_max[k])
        c.gain, c.ff, c.target_traj = gain.data_ptr(), None if ff is None else ff.data_ptr(), self.target_traj.data_ptr()
        return c

    def split_grad(self, raw, want):
        """The sweep's partials [tiles, T, U, S + 1] -> the gradients of (gain, ff) in their shapes (None where ``want`` is False): the slabs
        added in torch's fixed order, the rows too for a shared gain; rows beyond T of a longer tensor get zeros."""
        tot, T = raw.sum(0), int(raw.shape[1])
        g_gain = g_ff = None
        if want[0]:
            g = tot[..., :self.S]
            if self.shared:
                g_gain = g.sum(0)
            else:
                g_gain = g.new_zeros(self.shapes[0])
                g_gain[:T] = g
        if self.ff is not None and want[1]:
            g_ff = tot.new_zeros(self.shapes[1])
            g_ff[:T] = tot[..., self.S]
        return [g_gain] + ([g_ff] if self.ff is not None else [])


class PackedMLP:
    """mcp_mlp_policy of a ``Policy.MLP_policy``: the parameter tensors (W0, b0, [W1, b1], Wout, bout) are kept as they are -- every
    launch takes the LIVE tensors, so an optimizer's in-place updates are seen.  Features f = [x[non_angle], sin x[angle], cos x[angle]]
    (both lists empty: f = x).  A policy with a target trajectory (``policy.target_traj`` [rows, S], ``policy.error_indices``) appends the
    tracking errors target[t][idx[i]] - x[idx[i]] behind them (mcp_mlp_track): ``track_idx`` and ``target`` (a contiguous float64 GPU copy,
    not differentiable) are carried here, ``P`` counts them, and the launches go to the track entries.  A ``Policy.Residual_MLP_policy`` adds
    the PD term of mcp_mlp_pd ahead of the squashing: its two gain parameters come LAST in ``params`` / ``shapes`` / ``n_param`` (a launch takes
    them as [U] tensors, ``tensors()``), ``res_target`` / ``res_pos`` / ``res_vel`` are carried here, and the launches go to the residual
    entries (``res_c()``), whose sweep's slabs hold g_sqrt_kp | g_sqrt_kd behind bout.  A policy with memory (``policy.history`` = H > 1) reads
    the last H rows' features, newest block first, ahead of the errors: ``history`` is carried here, ``P`` = H P0 + the errors, and the
    launches go to the history entries (``hist_c()``) whatever the measurement, the dropout, the track and the PD term are."""

    fwd, bwd = ("mcp_rollout_mlp", "mcp_rollout_mlp_meas"), ("mcp_rollout_mlp_bwd", "mcp_rollout_mlp_meas_bwd")
    fwd_drop, bwd_drop = "mcp_rollout_mlp_drop", "mcp_rollout_mlp_drop_bwd"
    fwd_track, bwd_track = "mcp_rollout_mlp_track", "mcp_rollout_mlp_track_bwd"  # (a policy with a track: whatever meas and p_drop are)
    fwd_res, bwd_res = "mcp_rollout_mlp_res", "mcp_rollout_mlp_res_bwd"  # (a policy with the PD term: whatever meas, p_drop and the track are)
    fwd_hist, bwd_hist = "mcp_rollout_mlp_hist", "mcp_rollout_mlp_hist_bwd"  # (history > 1: whatever meas, p_drop, the track and the PD term are)
    fwd_outputs = ("mu", "var", "jac")
    grad_tile = 16  # one slab of parameter gradients per workgroup of the sweep

    def __init__(self, policy):
        self.params = list(policy.mlp_parameters())
        self.n_net = len(self.params)  # the network's own tensors; a residual policy's two gains come behind them
        self.S, self.U = int(policy.state_dim), int(policy.input_dim)
        self.hidden = [int(h) for h in policy.hidden_sizes]
        self.angle, self.non_angle = [int(i) for i in policy.angle_indices], [int(i) for i in policy.non_angle_indices]
        self.history = int(getattr(policy, "history", 1))
        if not 1 <= self.history <= abi.MAX_HIST:
            raise RuntimeError("the MLP policy reads 1 .. %d rows" % abi.MAX_HIST)
        self.P = self.history * (len(self.non_angle) + 2 * len(self.angle) if (self.angle or self.non_angle) else self.S)
        self.track_idx, self.target = None, None
        if getattr(policy, "target_traj", None) is not None:
            self.track_idx = [int(i) for i in policy.error_indices]
            if len(self.track_idx) > abi.MAX_STATE:
                raise RuntimeError("at most %d error features" % abi.MAX_STATE)
            self.target = _t(policy.target_traj, _dev(self.params[0].device)).reshape(-1, self.S).contiguous()
            self.P += len(self.track_idx)
        self.squash = bool(policy.flg_squash)
        um = policy._u_max_values() or ()  # (floats, wherever the bounds are kept)
        self.u_max = np.full(self.U, um[0]) if len(um) == 1 else np.asarray(um, dtype=np.float64)
        if self.u_max.size != self.U or self.U > abi.MAX_INPUT:
            raise RuntimeError("u_max must be a scalar or hold one bound per input (at most %d inputs)" % abi.MAX_INPUT)
        if len(self.hidden) not in (1, 2) or self.n_net != 2 * len(self.hidden) + 2:
            raise RuntimeError("the MLP policy has one or two hidden layers")
        if len(self.angle) > abi.MAX_STATE or len(self.non_angle) > abi.MAX_STATE:
            raise RuntimeError("at most %d indices per feature list" % abi.MAX_STATE)
        self.shapes = [tuple(q.shape) for q in self.params]
        self.n_param = sum(int(q.numel()) for q in self.params)
        # the PD term of a Policy.Residual_MLP_policy (mcp_mlp_pd): the two gain parameters last in params / shapes / n_param -- a launch takes
        # them as [U] tensors (a scalar gain expanded on the parameter's graph, as PackedPD.gains), the sweep's slab has 2 U more entries
        self.res_gains, self.res_target, self._res_live = None, None, None
        if getattr(policy, "pd_target_traj", None) is not None:
            self.res_gains = [policy.sqrt_Kp_gains, policy.sqrt_Kd_gains]
            self.res_pos, self.res_vel = [int(i) for i in policy.pd_pos_indices], [int(i) for i in policy.pd_vel_indices]
            if len(self.res_pos) != self.U or len(self.res_vel) != self.U or any(int(g.numel()) not in (1, self.U) for g in self.res_gains):
                raise RuntimeError("the PD term has one position, one velocity and one gain pair per input (or one gain for all)")
            same = self.target is not None and policy.pd_target_traj is policy.target_traj
            self.res_target = self.target if same else _t(policy.pd_target_traj, _dev(self.params[0].device)).reshape(-1, self.S).contiguous()
            self.params += self.res_gains
            self.shapes += [(self.U,), (self.U,)]
            self.n_param += 2 * self.U
        self.grad_shape = (self.n_param,)
        self.drop_width = sum(self.hidden)  # a row of keep-masks: the hidden units, layer 0's first
        self.device = self.params[0].device

    def tensors(self):
        if self.res_gains is None:
            return self.params
        return self.params[:self.n_net] + [g.reshape(-1).expand(self.U) if g.numel() == 1 and self.U > 1 else g.reshape(-1) for g in self.res_gains]

    def check(self, model, T):
        if self.S != model.S or self.U != model.U:
            raise RuntimeError("the MLP policy is for %d states and %d inputs, the model has %d and %d" % (self.S, self.U, model.S, model.U))
        if T < 1:
            raise RuntimeError("the rollout needs at least one row")
        if self.target is not None and self.target.shape[0] < T:
            raise RuntimeError("the target trajectory has %d rows, the rollout needs %d" % (self.target.shape[0], T))
        if self.res_target is not None and self.res_target.shape[0] < T:
            raise RuntimeError("the PD term's target has %d rows, the rollout needs %d" % (self.res_target.shape[0], T))

    def res_c(self):
        """mcp_mlp_pd over the gains of the launch whose descriptor ``to_c`` made last, or None for a policy without the PD term."""
        if self.res_gains is None:
            return None
        kp, kd = self._res_live
        c = abi.MLPResidual()
        c.on, c.rows, c.target = 1, int(self.res_target.shape[0]), self.res_target.data_ptr()
        c.sqrt_kp, c.sqrt_kd = kp.data_ptr(), kd.data_ptr()
        for k in range(self.U):
            c.pos[k], c.vel[k] = self.res_pos[k], self.res_vel[k]
        return c

    def hist_c(self):
        """mcp_mlp_hist: the depth of the window (1: none)."""
        c = abi.MLPHist()
        c.h = self.history
        return c

    def track_c(self):
        """mcp_mlp_track over the target held here, or None for a policy without one."""
        if self.target is None:
            return None
        c = abi.MLPTrack()
        c.n, c.rows, c.target = len(self.track_idx), int(self.target.shape[0]), self.target.data_ptr()
        for i, v in enumerate(self.track_idx):
            c.idx[i] = v
        return c

    def to_c(self, *tensors):
        """The descriptor over ``tensors``: contiguous float64 GPU tensors in the parameter order, of the parameters' shapes."""
        for t, shp in zip(tensors, self.shapes):
            if t.dtype != DT or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shp:
                raise RuntimeError("the MLP parameters must be contiguous float64 GPU tensors of their declared shapes")
        if self.res_gains is not None:
            self._res_live = (tensors[self.n_net], tensors[self.n_net + 1])  # (this launch's gains: res_c points at them)
        c = abi.MLPPolicy()
        c.S, c.U, c.P, c.n_hidden, c.squash = self.S, self.U, self.P, len(self.hidden), int(self.squash)
        for l, h in enumerate(self.hidden):
            c.h[l] = h
        c.n_angle, c.n_non_angle = len(self.angle), len(self.non_angle)
        for i, v in enumerate(self.angle):
            c.angle[i] = v
        for i, v in enumerate(self.non_angle):
            c.non_angle[i] = v
        for k in range(self.U):
            c.u_max[k] = float(self.u_max[k])
        slots = (0, 2) if len(self.hidden) == 1 else (0, 1, 2)  # (the output layer is always slot 2)
        for l, sl in enumerate(slots):
            c.W[sl], c.b[sl] = tensors[2 * l].data_ptr(), tensors[2 * l + 1].data_ptr()
        return c


def _meas_arg(meas, T, M, meas_buf):
    """The measured entries' extra argument, the mcp_meas of ``meas`` over ``meas_buf`` [T,M,S] (a list, to splice in); empty without one."""
    if meas is None:
        return []
    mc = abi.Meas()
    meas.fill(mc, T, M, meas_buf)
    return [C.byref(mc)]


def _drop_args(meas_arg, nz, p_drop):
    """What a dropout entry takes between the policy and the sizes: the measurement model or NULL, the noise (None: NULL), the probability."""
    return [meas_arg[0] if meas_arg else None, None if nz is None else C.byref(nz), float(p_drop)]


def _entry(packed, names, plain, marg, nz, p_drop, integ=None):
    """(name, arguments between the policy and the sizes) of the launch or sweep of ``packed``, ``names`` = (plain and measured, dropout,
    track, residual, integral): a policy with the integral term (PackedPID.term_c, ``integ`` its buffer) takes its one entry -- the term, the
    measurement or NULL, then ``plain``; a policy with the PD term (PackedMLP.res_c) takes its residual entry whatever the rest is; a policy with a track takes its track entry (the track, then the dropout entry's arguments) whatever ``marg`` and ``p_drop``
    are; else p_drop > 0 the dropout entry; else the plain or measured one with ``plain`` behind the measurement."""
    if integ is not None:
        return names[4], [C.byref(packed.term_c(integ)), marg[0] if marg else None] + plain
    if getattr(packed, "meas_slot", False):  # (one entry for the true state and the measurement: the model or NULL, then ``plain``)
        return names[0][0], [marg[0] if marg else None] + plain
    tc = packed.track_c() if names[2] else None
    rc = packed.res_c() if len(names) > 3 and names[3] else None
    if len(names) > 5 and names[5] and getattr(packed, "history", 1) > 1:  # (memory: the depth, the track or NULL, the term or NULL, the rest)
        return names[5], [C.byref(packed.hist_c()), None if tc is None else C.byref(tc), None if rc is None else C.byref(rc)] + _drop_args(marg, nz, p_drop)
    if rc is not None:  # (the PD term: the track or NULL, the term, then the dropout entry's arguments)
        return names[3], [None if tc is None else C.byref(tc), C.byref(rc)] + _drop_args(marg, nz, p_drop)
    if tc is not None:
        return names[2], [C.byref(tc)] + _drop_args(marg, nz, p_drop)
    if p_drop > 0.0:
        return names[1], _drop_args(marg, nz, p_drop)
    return names[0][bool(marg)], marg + plain


def _closed_launch(model, packed, tensors, noise, x0, T, particle_pred, status, record, meas=None, p_drop=0.0):
    """(states [T,M,S], inputs [T,M,U], jac or None) of ONE launch of the closed loop under ``packed`` over its parameter ``tensors``
    (packed.fwd); ``record`` and T > 1: the recording form.  With ``meas`` the measured entry, which writes ``meas.measured`` [T,M,S].
    ``p_drop`` > 0: the policy's dropout entry (packed.fwd_drop), whatever ``meas`` is.  A packed policy with a track (PackedMLP.track_c):
    its track entry (packed.fwd_track), whatever ``meas`` and ``p_drop`` are; without one exactly the calls above.  A packed policy with the
    integral term (PackedPID): its entry (packed.fwd_pid), which writes ``packed.integ`` [T,M,U]."""
    M, dev = int(x0.shape[0]), model.device
    states, inputs, jac = _record_buffers(dev, T, M, model.S, model.U, model.G, model.D, record and T > 1)
    pc, nz = packed.to_c(*tensors), noise.to_c()
    meas_buf = None
    if meas is not None:
        meas_buf = meas.measured = torch.empty(T, M, model.S, dtype=DT, device=dev)  # (allocated as rollout_forward_raw allocates it)
    outputs = {"jac": jac, "mu": None, "var": None}
    marg = _meas_arg(meas, T, M, meas_buf)
    integ = None
    if getattr(packed, "fwd_pid", None):
        integ = packed.integ = torch.empty(T, M, model.U, dtype=DT, device=dev)
    name, head = _entry(packed, (packed.fwd, getattr(packed, "fwd_drop", None), getattr(packed, "fwd_track", None),
                                 getattr(packed, "fwd_res", None), getattr(packed, "fwd_pid", None), getattr(packed, "fwd_hist", None)),
                        [C.byref(nz)], marg, nz, p_drop, integ)
    abi.check(getattr(abi.lib(), name)(_mc(model), C.byref(pc), *head, M, T,
                                       int(bool(particle_pred)), abi.ptr(x0), abi.ptr(states), abi.ptr(inputs),
                                       *[abi.ptr(outputs[k]) for k in packed.fwd_outputs], abi.ptr(status), abi.stream()), name)
    return states, inputs, jac


def _closed_sweep(model, packed, tensors, states, inputs, jac, g_states, g_inputs, want_params, want_x0, meas=None, meas_buf=None, noise=None,
                  p_drop=0.0, integ=None):
    """(raw parameter gradients [ceil(M / grad_tile)] + grad_shape or None, g_x0 [M,S] or None) of ONE reverse-time sweep over the record
    (packed.bwd); with ``meas`` (and the measured states ``meas_buf`` its forward launch wrote) the measured entry.  ``p_drop`` > 0: the
    policy's dropout entry (packed.bwd_drop) with the forward launch's ``noise``, from which it recomputes the keep decisions.  A packed
    policy with a track: packed.bwd_track, as in ``_closed_launch``.  ``integ``: the integral the forward launch of a PackedPID wrote
    (packed.bwd_pid)."""
    T, M, dev = int(states.shape[0]), int(states.shape[1]), states.device
    g_x0 = torch.empty(M, model.S, dtype=DT, device=dev) if want_x0 else None
    grad_shape = packed.grad_shape_of(T) if hasattr(packed, "grad_shape_of") else packed.grad_shape  # (a per-row gradient: its rows are the launch's)
    raw = torch.empty(((M + packed.grad_tile - 1) // packed.grad_tile,) + grad_shape, dtype=DT, device=dev) if want_params else None
    pc = packed.to_c(*tensors)
    marg = _meas_arg(meas, T, M, meas_buf)
    nz = noise.to_c() if p_drop > 0.0 else None  # (only the keep decisions are drawn again)
    name, head = _entry(packed, (packed.bwd, getattr(packed, "bwd_drop", None), getattr(packed, "bwd_track", None),
                                 getattr(packed, "bwd_res", None), getattr(packed, "bwd_pid", None), getattr(packed, "bwd_hist", None)), [],
                        marg, nz, p_drop, integ)
    abi.check(getattr(abi.lib(), name)(_mc(model), C.byref(pc), *head, M, T, abi.ptr(states), abi.ptr(inputs),
                                       abi.ptr(jac), abi.ptr(g_states), abi.ptr(g_inputs), abi.ptr(raw), abi.ptr(g_x0), abi.stream()), name)
    return raw, g_x0


class RolloutClosedFunction(torch.autograd.Function):
    """(x0 [M,S], the policy's parameter tensors) -> states [T,M,S], inputs [T,M,U] through the recording form of the fused closed loop
    under ``packed`` (a PackedPD or a PackedMLP); backward is the reverse-time sweep over the record, with both upstream gradients.  The
    sweep's raw parameter gradients (per trajectory, or per workgroup) are added in torch's fixed order (``sum(0)``); the GP model is
    frozen.  With a measurement model (``meas``) the two launches are the measured entries; the measured states [T,M,S] the forward launch
    wrote (``meas.measured``) are saved with the record and handed to the sweep.  With dropout (``p_drop`` > 0) the launch's noise goes to
    the sweep as well: the keep decisions are not recorded, the sweep draws them again.  Under a PackedPID the integral [T,M,U] the forward
    launch wrote (``packed.integ``) is saved with the record too."""

    @staticmethod
    def forward(ctx, model, packed, noise, T, particle_pred, status, meas, p_drop, x0, *tensors):
        states, inputs, jac = _closed_launch(model, packed, tensors, noise, x0, T, particle_pred, status, True, meas, p_drop)
        ctx.model, ctx.packed, ctx.has_jac, ctx.meas = model, packed, jac is not None, meas
        ctx.noise, ctx.p_drop = noise, p_drop
        integ = packed.integ if getattr(packed, "fwd_pid", None) else None
        ctx.has_integ = integ is not None
        ctx.set_materialize_grads(False)
        # (saved tensors: autograd refuses a backward after an in-place change of any of them -- the record, or a parameter stepped too early)
        ctx.save_for_backward(states, inputs, *tensors, *((jac,) if jac is not None else ()), *((meas.measured,) if meas is not None else ()),
                              *((integ,) if integ is not None else ()))
        return states, inputs

    @staticmethod
    def backward(ctx, g_states, g_inputs):
        packed, n = ctx.packed, len(ctx.packed.shapes)
        states, inputs, tensors, rest = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:2 + n], list(ctx.saved_tensors[2 + n:])
        jac = rest.pop(0) if ctx.has_jac else None
        meas_buf = rest.pop(0) if ctx.meas is not None else None
        integ = rest.pop(0) if ctx.has_integ else None
        gs = torch.zeros_like(states) if g_states is None else g_states.to(dtype=DT).contiguous()
        gi = None if g_inputs is None else g_inputs.to(dtype=DT).contiguous()
        want_x0, want = ctx.needs_input_grad[8], ctx.needs_input_grad[9:]
        raw, g_x0 = _closed_sweep(ctx.model, packed, tensors, states, inputs, jac, gs, gi, any(want), want_x0, ctx.meas, meas_buf, ctx.noise, ctx.p_drop,
                                  integ)
        grads = [None] * n
        if raw is not None and hasattr(packed, "split_grad"):  # (a gradient per row: the policy's own cut of the partials)
            grads = packed.split_grad(raw, want)
        elif raw is not None:
            flat, o = raw.sum(0).reshape(-1), 0  # the trajectories' / workgroups' rows added in torch's fixed order
            for i, shp in enumerate(packed.shapes):  # (only the parameters that need one get a gradient)
                k = int(np.prod(shp))
                if want[i]:
                    grads[i] = flat[o:o + k].reshape(shp)
                o += k
        return (None, None, None, None, None, None, None, None, g_x0) + tuple(grads)


def _rollout_closed(op, noun, model, packed, noise, x0, T, particle_pred, status, meas, p_drop=0.0):
    """What ``rollout_pd`` and ``rollout_mlp`` do (``op``: which, ``noun``: what its message calls the parameters -- the device refusal comes
    first and is raised whatever ``packed`` is, so the two words are not read from it): the checks, then the recording Function or, with
    nothing to differentiate, one launch on detached tensors.  ``p_drop``: the dropout probability of a policy that has dropout entries
    (0: the calls made without it); its masks, [T,M,packed.drop_width] uint8, are checked here."""
    if not isinstance(x0, torch.Tensor) or not x0.is_cuda or any(not q.is_cuda for q in packed.params):
        raise RuntimeError("%s operates on GPU memory only (x0 and %s must be GPU tensors); there is no CPU path" % (op, noun))
    T = int(T)
    packed.check(model, T)
    p_drop = float(p_drop)
    if not 0.0 <= p_drop < 1.0:
        raise RuntimeError("%s: p_drop must be in [0, 1)" % op)
    x0c, _, _, _, noise, status = _open_operands(model, x0, None, T, None, noise, particle_pred, status, packed.drop_width if p_drop > 0.0 else 0)
    tensors = [q.contiguous() for q in packed.tensors()]
    if torch.is_grad_enabled() and (x0c.requires_grad or any(q.requires_grad for q in tensors)):
        states, inputs = RolloutClosedFunction.apply(model, packed, noise, T, bool(particle_pred), status, meas, p_drop, x0c, *tensors)
    else:
        states, inputs, _ = _closed_launch(model, packed, [q.detach() for q in tensors], noise, x0c.detach(), T, particle_pred, status, False, meas,
                                           p_drop)
    return states, inputs, status


def rollout_pd(model: PackedModel, pd: PackedPD, noise: Optional[NoiseSpec], x0, T, particle_pred=True, status=None, meas: Optional[MeasSpec] = None):
    """Closed-loop rollout under a PD controller in ONE launch: x0 [M,S] -> states [T,M,S], inputs [T,M,U] (row T - 1 included) and the
    status word.  ``noise``: an eps buffer [T-1,M,G] or Philox by seed / call / particle_offset (``particle_pred``), as ``rollout_open``.
    With gradients enabled and x0 or a gain requiring grad the recording launch runs and backward is the fused sweep (gradients to
    ``sqrt_Kp_gains``, ``sqrt_Kd_gains`` and x0); otherwise nothing is recorded.  The same states and inputs, bit for bit, either way.
    ``meas``: a measurement model between the particles and the PD law (partially measurable systems, as in ``rollout``); the measured
    states [T,M,S] the law was evaluated on are left in ``meas.measured`` (not differentiable).  None: the law sees the true state, and
    the calls made are the ones made without the argument.  The return has the same three elements either way.
    ``pd`` a PackedPID (``Policy.PID_controller``): the law with the clamped integral of the position error, mcp_rollout_pid and its sweep
    (gradients to ``sqrt_Ki_gains`` too); the integral [T,M,U] is left in ``pd.integ`` (not differentiable)."""
    return _rollout_closed("rollout_pd", "the gains", model, pd, noise, x0, T, particle_pred, status, meas)


def rollout_tvl(model: PackedModel, packed: PackedTVL, noise: Optional[NoiseSpec], x0, T, particle_pred=True, status=None,
                meas: Optional[MeasSpec] = None):
    """Closed-loop rollout under a time-varying linear feedback law (``Policy.TV_linear_controller``) in ONE launch: arguments, return and
    recording rule of ``rollout_pd``, with u_t = squash(gain[t] (target[t] - r_t) + ff[t]) in the PD law's place (mcp_rollout_tvl and its
    sweep); the gradients go to ``gain`` and ``ff`` where they require one, per row, and to x0.  The target gets no gradient."""
    return _rollout_closed("rollout_tvl", "the gain and the feedforward", model, packed, noise, x0, T, particle_pred, status, meas)


def rollout_mlp(model: PackedModel, mlp: PackedMLP, noise: Optional[NoiseSpec], x0, T, particle_pred=True, status=None,
                meas: Optional[MeasSpec] = None, p_drop=0.0):
    """Closed-loop rollout under a tanh-MLP policy in ONE launch: arguments, return and recording rule of ``rollout_pd``, with the network in
    the PD law's place; the gradients go to the parameters that require them and to x0.  ``p_drop`` > 0: inverted dropout on the hidden
    units, h = keep ? tanh(.) / (1 - p_drop) : 0, one row of decisions per policy evaluation -- ``noise.masks`` [T,M,H] uint8 (H: the
    hidden widths added, layer 0's units first) or, without a buffer, Philox by seed / call / global particle, shard-invariant; the sweep
    draws the same decisions again.  0 (the default): the calls made without the argument.  A tracking policy (``mlp.target`` [rows >= T, S]:
    features [x[non_angle], sin x[angle], cos x[angle], target[t][idx] - x[idx]], under ``meas`` with the measurement in x's place) runs the
    track entries; the target gets no gradient."""
    if meas is not None and getattr(mlp, "history", 1) > 1:
        raise RuntimeError("rollout_mlp: a policy with memory (history > 1) has no fused form on a simulated measurement")
    return _rollout_closed("rollout_mlp", "the parameters", model, mlp, noise, x0, T, particle_pred, status, meas, p_drop)


# measurement hook (bench.py): a pair of torch.cuda.Event recorded on the launch stream right around mcp_rollout_bwd -- the adjoint sweep
# runs inside autograd's backward, where the caller cannot bracket it.  None (the default) = nothing is recorded.  ``fwd_events``: the same
# around mcp_rollout_fwd (operand packing + hand-off buffer reset + the rollout kernel, without the host's tensor allocations).
bwd_events = None
fwd_events = None


def rollout_backward_raw(model: PackedModel, policy: PackedPolicy, noise: NoiseSpec, states, inputs, jac, g_states, g_inputs, p_drop,
                         want_gx0=False, meas: Optional[MeasSpec] = None, meas_buf=None):
    dev = policy.device
    T, M = states.shape[0], states.shape[1]
    pc = policy.bind(p_drop)
    nz = noise.to_c()
    nbytes, ws, _ = _workspace(model, policy, pc, M, T, "bwd")
    # ONE flat buffer [dJ/dlog_ls (P) | dJ/dcenters (B P) | dJ/dweight (U B) | dJ/dbias (U)]: the three (four) gradients are views of it --
    # autograd hands them to the parameters' .grad as they are, so a particle-sharded step all-reduces its message IN PLACE when the caller
    # supplies the head of that message as ``policy.grad_flat`` (sharding.StepMessage); otherwise one allocation per step instead of four
    P_, B_, U_ = policy.P, policy.B, policy.U
    n_ls, n_c, n_w = P_, B_ * P_, U_ * B_
    n_all = n_ls + n_c + n_w + (U_ if policy.bias is not None else 0)
    flat = getattr(policy, "grad_flat", None)
    if flat is None or flat.numel() < n_all or flat.dtype != DT or flat.device != dev or not flat.is_contiguous():
        flat = torch.empty(n_all, dtype=DT, device=dev)
    g_ls = flat[0:n_ls].view(1, P_)
    g_c = flat[n_ls:n_ls + n_c].view(B_, P_)
    g_w = flat[n_ls + n_c:n_ls + n_c + n_w].view(U_, B_)
    g_b = flat[n_ls + n_c + n_w:n_all] if policy.bias is not None else None
    g_x0 = torch.empty(M, policy.S, dtype=DT, device=dev) if want_gx0 else None
    pc.g_bias = None if g_b is None else g_b.data_ptr()
    gs = None if g_states is None else g_states.to(dtype=DT).contiguous()
    gi = None if g_inputs is None else g_inputs.to(dtype=DT).contiguous()
    _set_meas(policy, meas, T, M, meas_buf)
    ev = bwd_events
    try:
        if ev is not None:
            ev[0].record()
        abi.check(abi.lib().mcp_rollout_bwd_ex(_mc(model), C.byref(pc), C.byref(nz), M, T, abi.ptr(states), abi.ptr(inputs), abi.ptr(jac),
                                               abi.ptr(gs), abi.ptr(gi), abi.ptr(g_ls), abi.ptr(g_c), abi.ptr(g_w), abi.ptr(g_x0), abi.ptr(ws),
                                               nbytes, abi.stream(), C.byref(abi.DISPATCH)), "mcp_rollout_bwd")
        if ev is not None:
            ev[1].record()
    finally:
        _set_meas(policy, None, T, M, None)
        pc.g_bias = None
    return g_ls, g_c, g_w, g_x0, g_b


class RolloutFunction(torch.autograd.Function):
    """(x0, log_lengthscales, centers, weight) -> (states [T,M,S], inputs [T,M,U]) through the fused
    HIP rollout; backward is the fused reverse-time adjoint.  Gradients flow to the three policy
    parameters (and x0); the GP model is frozen, as after ``Model_learning.set_eval_mode``."""

    @staticmethod
    def forward(ctx, x0, log_ls, centers, weight, bias, model, policy, noise, T, p_drop, particle_pred, meas=None, gp_sharding=True, status_acc=None):
        need = any(ctx.needs_input_grad[:5])
        ctx.set_materialize_grads(False)  # (an output the cost does not use -- usually the inputs -- arrives as None, not as a zero-filled tensor)
        out = rollout_forward_raw(model, policy, noise, x0, T, p_drop, particle_pred, need_jac=need, meas=meas, gp_sharding=gp_sharding, status=status_acc)
        states, inputs, jac, status = out[:4]
        if status_acc is not None:
            status = status.view(1)  # (an output must not BE an input; a view launches nothing)
        ctx.model, ctx.policy, ctx.noise, ctx.p_drop = model, policy, noise, p_drop
        ctx.meas, ctx.meas_buf = meas, (out[4] if meas is not None else None)
        ctx.has_jac = jac is not None
        ctx.save_for_backward(states, inputs, jac if jac is not None else torch.empty(0, device=states.device))
        ctx.mark_non_differentiable(status)
        return states, inputs, status

    @staticmethod
    def backward(ctx, g_states, g_inputs, _g_status):
        states, inputs, jac = ctx.saved_tensors
        if not ctx.has_jac:
            jac = None
        if g_states is None and g_inputs is None:  # (nothing downstream depends on the rollout)
            g_states = torch.zeros_like(states)
        g_ls, g_c, g_w, g_x0, g_b = rollout_backward_raw(ctx.model, ctx.policy, ctx.noise, states, inputs, jac, g_states, g_inputs, ctx.p_drop,
                                                         want_gx0=ctx.needs_input_grad[0], meas=ctx.meas, meas_buf=ctx.meas_buf)
        if g_b is not None:
            g_b = g_b.reshape(ctx.policy.bias.shape)
        return g_x0, g_ls.reshape(ctx.policy.log_ls.shape), g_c, g_w, g_b, None, None, None, None, None, None, None, None, None


def rollout(model, policy, noise, x0, T, p_drop=0.0, particle_pred=True, meas: Optional[MeasSpec] = None, gp_sharding=True, status=None):
    """Differentiable fused rollout.  Returns (states, inputs, status).  ``meas``: measurement model between the particles and
    the policy (partially measurable systems); None = the policy sees the true state.  ``gp_sharding`` False forbids the
    GP-sharded launch forms (used to repeat a step whose hand-off reported MCP_STATUS_SYNC).  ``status``: see rollout_forward_raw."""
    return RolloutFunction.apply(x0, policy.log_ls, policy.centers, policy.weight, policy.bias, model, policy, noise, int(T), float(p_drop),
                                 bool(particle_pred), meas, bool(gp_sharding), status)


# --------------------------------------------------------------------------------------
# cost (autograd)
# --------------------------------------------------------------------------------------
class PackedCost:
    def __init__(self, kind, S, device, **kw):
        dev = _dev(device)
        c = abi.Cost()
        c.S = int(S)
        self._keep = []
        if kind == "cartpole":
            c.kind = abi.COST_CARTPOLE
            c.angle_index, c.pos_index = int(kw["angle_index"]), int(kw["pos_index"])
            ts = [float(v) for v in kw["target_state"]]
            ls = [float(v) for v in kw["lengthscales"]]
            c.target_angle, c.target_pos, c.ls_angle, c.ls_pos = ts[0], ts[1], ls[0], ls[1]
        elif kind == "traj":
            c.kind = abi.COST_TRAJ
            used = list(range(S)) if kw.get("used") is None else [int(u) for u in kw["used"]]
            c.n_used = len(used)
            for i, u in enumerate(used):
                c.used[i] = u
            tt = _t(kw["target_traj"], dev)
            ls = _t(kw["lengthscales"], dev).reshape(-1)
            if ls.numel() != len(used):
                raise ValueError("trajectory cost: one lengthscale per used state index is required")
            self._keep = [tt, ls]
            c.target_traj, c.lengthscales = tt.data_ptr(), ls.data_ptr()
            self.traj_len = int(tt.shape[0])
        elif kind == "target":
            # target-state costs (Cost_function.py:39-101): ONE target row over ``active_dims``; saturate False = the plain distance.
            # Everything is checked on the host values first: a bad descriptor never reaches the device.
            c.kind = abi.COST_TARGET if kw.get("saturate", True) else abi.COST_TARGET_QUAD
            act = [int(i) for i in np.asarray(kw["active_dims"]).reshape(-1)]
            n_t, n_l = _count(kw["target_state"]), _count(kw["lengthscales"])
            if not (len(act) == n_t == n_l):
                raise ValueError("target cost: %d active dims, %d target entries (one row) and %d lengthscales must agree" % (len(act), n_t, n_l))
            if not 1 <= len(act) <= abi.MAX_STATE:
                raise ValueError("target cost: 1..%d active dims are supported (%d given)" % (abi.MAX_STATE, len(act)))
            if any(i < 0 or i >= int(S) for i in act):
                raise ValueError("target cost: active dims %s outside the state [0, %d)" % (act, int(S)))
            c.n_used = len(act)
            for i, u in enumerate(act):
                c.used[i] = u
            tg = _t(kw["target_state"], dev).reshape(-1)
            ls = _t(kw["lengthscales"], dev).reshape(-1)
            self._keep = [tg, ls]
            c.target_traj, c.lengthscales = tg.data_ptr(), ls.data_ptr()
        else:
            raise ValueError(kind)
        self.kind, self.c, self.device = kind, c, dev


def _host(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


class PackedCostInputs:
    """mcp_cost_inputs: control-effort and input-rate terms next to a PackedCost (include/mcpilco_hip.h).  ``input_indices`` (None: every
    input) are the columns of the inputs the terms read; ``lengthscales`` l_i / ``rate_lengthscales`` r_i switch the effort term
    sum_i ((u_i - u*_i) / l_i)^2 and the rate term sum_i ((u_t,i - u_t-1,i) / r_i)^2 on (at least one is required);
    ``target_input`` u* (None: 0); ``joint``: f(d_x + d_u + d_r) instead of f(d_x) + d_u + d_r.  Everything is checked on the host values
    first: a bad descriptor raises ValueError before a device is touched."""

    def __init__(self, U, device, input_indices=None, lengthscales=None, rate_lengthscales=None, target_input=None, joint=False):
        U = int(U)
        if not 1 <= U <= abi.MAX_INPUT:
            raise ValueError("input cost: 1..%d inputs are supported (%d given)" % (abi.MAX_INPUT, U))
        idx = list(range(U)) if input_indices is None else [int(i) for i in np.asarray(input_indices).reshape(-1)]
        if not 1 <= len(idx) <= abi.MAX_INPUT:
            raise ValueError("input cost: 1..%d input indices are supported (%d given)" % (abi.MAX_INPUT, len(idx)))
        if any(i < 0 or i >= U for i in idx):
            raise ValueError("input cost: input indices %s outside [0, %d)" % (idx, U))
        if len(set(idx)) != len(idx):
            raise ValueError("input cost: an input index is listed twice in %s" % (idx,))
        if lengthscales is None and rate_lengthscales is None:
            raise ValueError("input cost: lengthscales (effort term) or rate_lengthscales (rate term) must be given")
        host = {}
        for name, v in (("lengthscales", lengthscales), ("rate_lengthscales", rate_lengthscales), ("target_input", target_input)):
            if v is None:
                continue
            h = _host(v).reshape(-1)
            if h.size != len(idx):
                raise ValueError("input cost: %d input indices but %d entries in %s" % (len(idx), h.size, name))
            if name != "target_input" and not bool(np.all(np.isfinite(h) & (h > 0))):
                raise ValueError("input cost: %s must be finite and > 0 (%s)" % (name, h.tolist()))
            if name == "target_input" and not bool(np.all(np.isfinite(h))):
                raise ValueError("input cost: target_input must be finite (%s)" % (h.tolist(),))
            host[name] = h
        dev = _dev(device)
        c = abi.CostInputs()
        c.U, c.mode, c.n_used = U, (abi.COST_U_JOINT if joint else abi.COST_U_ADD), len(idx)
        for i, u in enumerate(idx):
            c.used[i] = u
        self._keep = {k: _t(h, dev) for k, h in host.items()}
        for field, name in (("scales", "lengthscales"), ("rate_scales", "rate_lengthscales"), ("target", "target_input")):
            if name in self._keep:
                setattr(c, field, self._keep[name].data_ptr())
        self.c, self.device, self.U, self.used, self.joint = c, dev, U, idx, bool(joint)


class PackedObjective:
    """mcp_objective: J = sum_t w_t (mean_t + kappa std_t) over the T steps of a rollout (include/mcpilco_hip.h).  ``time_weights`` (at least T
    entries, the first T are used; None: ones), ``discount`` gamma in (0, 1] (w_t = gamma^t; None: 1), or the product of both; ``risk``
    kappa, any finite real.  Everything is checked on the host values first: a bad objective raises ValueError before a device is touched.
    The [T] device tensor of the weights is kept alive here (``w``; None when neither option is given: the kernels take NULL as ones)."""

    def __init__(self, T, device, time_weights=None, discount=None, risk=0.0):
        T = int(T)
        if T < 1:
            raise ValueError("objective: T must be at least 1 (%d given)" % T)
        host = objective_weights(T, time_weights, discount)
        kappa = float(risk)
        if not np.isfinite(kappa):
            raise ValueError("objective: risk must be finite (%r)" % (risk,))
        dev = _dev(device)
        c = abi.Objective()
        c.kappa = kappa
        self.w = None if host is None else _t(host, dev)
        if self.w is not None:
            c.w = self.w.data_ptr()
        self.c, self.device, self.T, self.kappa = c, dev, T, kappa
        self._mean = None

    def mean_part(self):
        """The same weights (the same device tensor) with kappa = 0: what a rank's share of a sharded step is formed with."""
        if self.kappa == 0.0:
            return self
        if self._mean is None:
            m = object.__new__(PackedObjective)
            m.c = abi.Objective()
            m.c.w, m.c.kappa = self.c.w, 0.0
            m.w, m.device, m.T, m.kappa, m._mean = self.w, self.device, self.T, 0.0, None
            self._mean = m
        return self._mean

    def check_particles(self, n_total):
        if self.kappa != 0.0 and int(n_total) < 2:
            raise ValueError("objective: the std term (risk = %g) needs at least two particles (%d given)" % (self.kappa, int(n_total)))


def objective_weights(T, time_weights=None, discount=None):
    """The host values w_t = time_weights[t] gamma^t, t < T, of an objective (None: neither option is given), checked: finite, >= 0, not all
    zero, at least T entries, gamma in (0, 1]."""
    if time_weights is None and discount is None:
        return None
    w = np.ones(T)
    if time_weights is not None:
        h = _host(time_weights).reshape(-1)
        if h.size < T:
            raise ValueError("objective: %d time weights for %d time steps" % (h.size, T))
        w = h[:T].copy()
        if not bool(np.all(np.isfinite(w) & (w >= 0))):
            raise ValueError("objective: time weights must be finite and >= 0 (%s)" % (w.tolist(),))
    if discount is not None:
        g = float(discount)
        if not (0.0 < g <= 1.0):  # (NaN fails both comparisons)
            raise ValueError("objective: discount must lie in (0, 1] (%r)" % (discount,))
        w = w * g ** np.arange(T)
    if not bool(np.any(w > 0)):
        raise ValueError("objective: at least one time weight must be > 0")
    return w


def _check_cost_inputs(states, inputs, cost_inputs):
    """The inputs [T,M,U] of a cost with input terms, detached and contiguous."""
    if inputs is None or cost_inputs is None:
        raise ValueError("a cost with input terms takes both `inputs` and `cost_inputs`")
    T, M, _ = states.shape
    if inputs.dim() != 3 or tuple(inputs.shape) != (T, M, cost_inputs.U) or inputs.dtype != DT or inputs.device != states.device:
        raise RuntimeError("inputs must be float64 [T=%d, M=%d, U=%d] on the states' device (got %s %s)"
                           % (T, M, cost_inputs.U, tuple(inputs.shape), inputs.dtype))
    return inputs.detach().contiguous()


def _cost_u_bwd(cost, states, g_cost, gscale, inputs, cost_inputs, want_g_inputs=True):
    """mcp_cost_u_bwd -> (g_states, g_inputs or None)."""
    T, M, _ = states.shape
    st = states.contiguous()
    g = torch.empty_like(st)
    g_in = torch.empty_like(inputs) if want_g_inputs else None
    abi.check(abi.lib().mcp_cost_u_bwd(C.byref(cost.c), C.byref(cost_inputs.c), T, M, abi.ptr(st), abi.ptr(inputs), abi.ptr(g_cost), gscale,
                                       abi.ptr(g), abi.ptr(g_in), abi.stream()), "mcp_cost_u_bwd")
    return g, g_in


_COST_STATUS_SINK = {}  # per device: where mcp_cost_fwd ORs its flags when the caller does not ask for them (never read, never zeroed again)


def cost_moments(cost: PackedCost, states, status=None, inputs=None, cost_inputs=None):
    """Per-time-step (mean, centred sum of squares) over this rank's particles -> [T,2], plus costs [T,M].  ``status``: a zeroed int32[1] to receive the
    kernel's flags (NaN in the costs); None: the flags go to a per-device sink -- the loops decide on the NaN of the cost itself, and a zero-fill
    launch per optimizer step is 4 us of the 0.8 ms a launch-script step takes.  With ``inputs`` [T,M,U] and ``cost_inputs`` (a
    PackedCostInputs) the costs carry the control-effort / input-rate terms (mcp_cost_u_fwd)."""
    T, M, _ = states.shape
    if inputs is not None or cost_inputs is not None:
        inputs = _check_cost_inputs(states, inputs, cost_inputs)
    if cost.kind == "traj" and cost.traj_len != T:
        raise RuntimeError("target trajectory has %d rows but the rollout has %d steps" % (cost.traj_len, T))
    st = states.detach().contiguous()
    costs = torch.empty(T, M, dtype=DT, device=st.device)
    mom = torch.empty(T, 2, dtype=DT, device=st.device)
    if status is None:
        status = _COST_STATUS_SINK.get(st.device)
        if status is None:
            status = _COST_STATUS_SINK[st.device] = torch.zeros(1, dtype=torch.int32, device=st.device)
    if cost_inputs is not None:
        abi.check(abi.lib().mcp_cost_u_fwd(C.byref(cost.c), C.byref(cost_inputs.c), T, M, abi.ptr(st), abi.ptr(inputs), abi.ptr(costs),
                                           abi.ptr(mom), abi.ptr(status), abi.stream()), "mcp_cost_u_fwd")
        return mom, costs, status
    abi.check(abi.lib().mcp_cost_fwd(C.byref(cost.c), T, M, abi.ptr(st), abi.ptr(costs), abi.ptr(mom), abi.ptr(status), abi.stream()),
              "mcp_cost_fwd")
    return mom, costs, status


def cost_finalize(moments_all, counts):
    """moments_all [R,T,2] (all ranks), counts: list of R ints -> tensor [2] = (cost, std)."""
    R, T = moments_all.shape[0], moments_all.shape[1]
    out = torch.empty(2, dtype=DT, device=moments_all.device)
    cnt = (C.c_int64 * R)(*[int(c) for c in counts])
    abi.check(abi.lib().mcp_cost_finalize(T, R, abi.ptr(moments_all.contiguous()), cnt, abi.ptr(out), abi.stream()), "mcp_cost_finalize")
    return out


class ExpectedCostFunction(torch.autograd.Function):
    """states [T,M,S] -> (sum_t mean_m c, sum_t std_m c) with the HIP cost kernels; with a
    torch.distributed ``group`` the mean/std pool all ranks' particles (one all-gather of the
    [T,2] moments).  ``counts``: particles per rank (default: every rank holds M).  With ``inputs`` [T,M,U] and ``cost_inputs`` the cost
    carries the input terms and the backward returns a gradient for the inputs as well."""

    @staticmethod
    def forward(ctx, states, cost, group, counts, inputs=None, cost_inputs=None):
        ctx.set_materialize_grads(False)
        mom, _, _ = cost_moments(cost, states, None, inputs, cost_inputs)
        ctx.cost_inputs = cost_inputs
        M = states.shape[1]
        if group is not None:
            from . import sharding

            mom_all = sharding.gather_moments(mom, group)
            counts = [M] * mom_all.shape[0] if counts is None else [int(c) for c in counts]
        else:
            counts = [M]
            mom_all = mom.unsqueeze(0)
        out = cost_finalize(mom_all, counts)
        ctx.cost, ctx.m_total = cost, sum(counts)
        if cost_inputs is None:
            ctx.save_for_backward(states.detach())
        else:
            ctx.save_for_backward(states.detach(), inputs.detach().contiguous())
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cost, _g_std):
        if ctx.cost_inputs is not None:
            states, inputs = ctx.saved_tensors
            if g_cost is None:
                return torch.zeros_like(states), None, None, None, (torch.zeros_like(inputs) if ctx.needs_input_grad[4] else None), None
            gc = g_cost.detach().to(dtype=DT).reshape(1).contiguous()
            g, g_in = _cost_u_bwd(ctx.cost, states, gc, 1.0 / float(ctx.m_total), inputs, ctx.cost_inputs, ctx.needs_input_grad[4])
            return g, None, None, None, g_in, None
        (states,) = ctx.saved_tensors
        T, M, _ = states.shape
        if g_cost is None:  # (only the std output is used downstream: this operator carries no gradient through it, as before)
            return (torch.zeros_like(states),) + (None,) * (len(ctx.needs_input_grad) - 1)
        g = torch.empty_like(states)
        st = states.contiguous()
        gc = g_cost.detach().to(dtype=DT).reshape(1).contiguous()  # stays on the device: no host sync
        abi.check(abi.lib().mcp_cost_bwd(C.byref(ctx.cost.c), T, M, abi.ptr(st), abi.ptr(gc), 1.0 / float(ctx.m_total), abi.ptr(g), abi.stream()),
                  "mcp_cost_bwd")
        return (g,) + (None,) * (len(ctx.needs_input_grad) - 1)


def expected_cost_raw(cost: PackedCost, states, g_one, inputs=None, cost_inputs=None, want_g_inputs=False, objective=None):
    """(cost, std, dJ/dstates) of this process's particles without autograd: exactly the launches ExpectedCostFunction's forward and backward
    make (``g_one``: a device scalar 1.0, the upstream gradient ``cost.backward()`` starts from).  For callers that replay the step from a
    HIP graph (MC_PILCO.reinforce_policy): the autograd engine's own stream bookkeeping does not survive a stream capture.  With
    ``inputs`` / ``cost_inputs`` the cost carries the input terms; ``want_g_inputs``: dJ/dinputs is returned as a fourth value (None for a
    cost without input terms: the adjoint sweeps take that as "no gradient").  With ``objective`` (a PackedObjective) the three launches are
    mcp_cost_fwd / mcp_cost_rows / mcp_cost_bwd_shaped and (cost, std) are (J, S)."""
    if objective is not None:
        T, M, _ = states.shape
        _check_objective(objective, T, M)
        mom, costs, _ = cost_moments(cost, states, None, inputs, cost_inputs)
        rows, out = cost_rows(mom.unsqueeze(0), [M], objective)
        g, g_in = _cost_bwd_shaped(cost, cost_inputs, objective, states.detach().contiguous(), None if cost_inputs is None else inputs.detach().contiguous(),
                                   costs, rows, g_one, M, want_g_inputs and cost_inputs is not None)
        return (out[0], out[1], g, g_in) if want_g_inputs else (out[0], out[1], g)
    mom, _, _ = cost_moments(cost, states, None, inputs, cost_inputs)
    T, M, _ = states.shape
    out = cost_finalize(mom.unsqueeze(0), [M])
    st = states.detach().contiguous()
    if cost_inputs is not None:
        g, g_in = _cost_u_bwd(cost, st, g_one, 1.0 / float(M), inputs.detach().contiguous(), cost_inputs, want_g_inputs)
        return (out[0], out[1], g, g_in) if want_g_inputs else (out[0], out[1], g)
    g = torch.empty_like(st)
    abi.check(abi.lib().mcp_cost_bwd(C.byref(cost.c), T, M, abi.ptr(st), abi.ptr(g_one), 1.0 / float(M), abi.ptr(g), abi.stream()), "mcp_cost_bwd")
    return (out[0], out[1], g, None) if want_g_inputs else (out[0], out[1], g)


def expected_cost(cost: PackedCost, states, group=None, counts=None, inputs=None, cost_inputs=None, objective=None):
    if objective is not None:
        return ShapedCostFunction.apply(states, cost, group, counts, inputs, cost_inputs, objective)
    if inputs is None and cost_inputs is None:
        return ExpectedCostFunction.apply(states, cost, group, counts)
    return ExpectedCostFunction.apply(states, cost, group, counts, inputs, cost_inputs)


class LocalCostFunction(torch.autograd.Function):
    """This rank's share of a particle-sharded expected cost, in the form ONE all-reduce(sum) can pool:
    states [T,M_local,S] -> (share = sum_t sum_m c_tm / m_total  [differentiable; its gradient is what this rank contributes to
    d(sum_t mean_m c)/dtheta],  sums [2T] = mcp_cost_sums: per time step sum_m (c - shift_t) and sum_m (c - shift_t)^2)."""

    @staticmethod
    def forward(ctx, states, cost, m_total, shift, sums_out=None, inputs=None, cost_inputs=None):
        mom, _, _ = cost_moments(cost, states, None, inputs, cost_inputs)
        ctx.cost_inputs = cost_inputs
        T, M = states.shape[0], states.shape[1]
        # (sums_out: a 1-tuple holding the caller's slot of the step's all-reduce message, sharding.StepMessage.sums -- in a tuple so that
        #  autograd does not take the slot for an input of this function)
        sums = sums_out[0] if sums_out is not None else torch.empty(2 * T, dtype=DT, device=states.device)
        if sums.numel() != 2 * T or sums.dtype != DT or not sums.is_contiguous():
            raise RuntimeError("sums_out must be a contiguous float64 tensor of 2 T entries")
        abi.check(abi.lib().mcp_cost_sums(T, M, abi.ptr(mom), abi.ptr(shift), abi.ptr(sums), abi.stream()), "mcp_cost_sums")
        local = cost_finalize(mom.unsqueeze(0), [M])[0] * (float(M) / float(m_total))
        ctx.cost, ctx.m_total = cost, int(m_total)
        if cost_inputs is None:
            ctx.save_for_backward(states.detach())
        else:
            ctx.save_for_backward(states.detach(), inputs.detach().contiguous())
        ctx.mark_non_differentiable(sums)
        return local, sums

    @staticmethod
    def backward(ctx, g_local, _g_sums):
        if ctx.cost_inputs is not None:
            states, inputs = ctx.saved_tensors
            gc = g_local.detach().to(dtype=DT).reshape(1).contiguous()
            g, g_in = _cost_u_bwd(ctx.cost, states, gc, 1.0 / float(ctx.m_total), inputs, ctx.cost_inputs, ctx.needs_input_grad[5])
            return g, None, None, None, None, g_in, None
        (states,) = ctx.saved_tensors
        T, M, _ = states.shape
        g = torch.empty_like(states)
        st = states.contiguous()
        gc = g_local.detach().to(dtype=DT).reshape(1).contiguous()
        abi.check(abi.lib().mcp_cost_bwd(C.byref(ctx.cost.c), T, M, abi.ptr(st), abi.ptr(gc), 1.0 / float(ctx.m_total), abi.ptr(g), abi.stream()),
                  "mcp_cost_bwd")
        return (g,) + (None,) * (len(ctx.needs_input_grad) - 1)


def local_cost(cost: PackedCost, states, m_total, shift=None, sums_out=None, inputs=None, cost_inputs=None, objective=None, reducer=None):
    """``objective`` (a PackedObjective): the share is this rank's part of J.  With kappa != 0 the gradient needs the POOLED rows of this very
    step, so ``reducer`` (sharding.StepReducer) is required: one additional small all-reduce of a copy of the 2T sums (ShapedLocalCostFunction)."""
    if objective is not None:
        return ShapedLocalCostFunction.apply(states, cost, int(m_total), shift, None if sums_out is None else (sums_out,), inputs, cost_inputs,
                                             objective, reducer)
    if inputs is None and cost_inputs is None:
        return LocalCostFunction.apply(states, cost, int(m_total), shift, None if sums_out is None else (sums_out,))
    return LocalCostFunction.apply(states, cost, int(m_total), shift, None if sums_out is None else (sums_out,), inputs, cost_inputs)


def cost_from_sums(sums, n_total, shift=None, mean_out=None, objective=None):
    """Pooled (sum_t mean_m c, sum_t unbiased std_m c) from the all-reduced sums of ``local_cost`` -> tensor [2]; with ``objective`` the
    pooled (J, S) (mcp_cost_rows_sums)."""
    if objective is not None:
        return cost_rows_sums(sums, n_total, shift, mean_out, objective)[1]
    T = sums.numel() // 2
    out = torch.empty(2, dtype=DT, device=sums.device)
    abi.check(abi.lib().mcp_cost_finalize_sums(T, int(n_total), abi.ptr(sums.contiguous()), abi.ptr(shift), abi.ptr(out), abi.ptr(mean_out),
                                               abi.stream()), "mcp_cost_finalize_sums")
    return out


# ---- the time-weighted, risk-sensitive objective (PackedObjective; mcp_cost_rows / mcp_cost_rows_sums / mcp_cost_bwd_shaped) ------------------
def _check_objective(objective, T, n_total):
    if objective.T != int(T):
        raise RuntimeError("the objective holds %d time weights but the rollout has %d steps" % (objective.T, int(T)))
    objective.check_particles(n_total)


def cost_rows(moments_all, counts, objective=None):
    """moments_all [R,T,2] (all ranks), counts: R ints -> (rows [T,2] = pooled (mean_t, unbiased std_t), out [2] = (J, S)).  objective None:
    out holds cost_finalize's bits."""
    R, T = moments_all.shape[0], moments_all.shape[1]
    rows = torch.empty(T, 2, dtype=DT, device=moments_all.device)
    out = torch.empty(2, dtype=DT, device=moments_all.device)
    cnt = (C.c_int64 * R)(*[int(c) for c in counts])
    abi.check(abi.lib().mcp_cost_rows(T, R, abi.ptr(moments_all.contiguous()), cnt, None if objective is None else C.byref(objective.c), abi.ptr(rows),
                                      abi.ptr(out), abi.stream()), "mcp_cost_rows")
    return rows, out


def cost_rows_sums(sums, n_total, shift=None, mean_out=None, objective=None):
    """The all-reduced sums of ``local_cost`` -> (rows [T,2], out [2] = (J, S)) of the pooled swarm."""
    T = sums.numel() // 2
    rows = torch.empty(T, 2, dtype=DT, device=sums.device)
    out = torch.empty(2, dtype=DT, device=sums.device)
    abi.check(abi.lib().mcp_cost_rows_sums(T, int(n_total), abi.ptr(sums.contiguous()), abi.ptr(shift), None if objective is None else C.byref(objective.c),
                                           abi.ptr(rows), abi.ptr(out), abi.ptr(mean_out), abi.stream()), "mcp_cost_rows_sums")
    return rows, out


def _cost_bwd_shaped(cost, cost_inputs, objective, states, inputs, costs, rows, g_cost, n_total, want_g_inputs=True):
    """mcp_cost_bwd_shaped -> (g_states, g_inputs or None); states / inputs detached and contiguous."""
    T, M, _ = states.shape
    g = torch.empty_like(states)
    g_in = torch.empty_like(inputs) if (want_g_inputs and cost_inputs is not None) else None
    abi.check(abi.lib().mcp_cost_bwd_shaped(C.byref(cost.c), None if cost_inputs is None else C.byref(cost_inputs.c),
                                            None if objective is None else C.byref(objective.c), T, M, int(n_total), abi.ptr(states), abi.ptr(inputs),
                                            abi.ptr(costs), abi.ptr(rows), abi.ptr(g_cost), abi.ptr(g), abi.ptr(g_in), abi.stream()),
              "mcp_cost_bwd_shaped")
    return g, g_in


class ShapedCostFunction(torch.autograd.Function):
    """ExpectedCostFunction under a PackedObjective: states [T,M,S] (and inputs) -> (J, S) = (sum_t w_t (mean_t + kappa std_t), sum_t w_t std_t)
    with the gradient of J (S carries none).  Three launches on one rank, as without an objective: forward, rows + objective, backward; with a
    ``group`` the rows pool every rank's gathered moments and the backward takes n_total = sum(counts)."""

    @staticmethod
    def forward(ctx, states, cost, group, counts, inputs, cost_inputs, objective):
        ctx.set_materialize_grads(False)
        T, M, _ = states.shape
        if group is not None:
            from . import sharding

            mom, costs, _ = cost_moments(cost, states, None, inputs, cost_inputs)
            mom_all = sharding.gather_moments(mom, group)
            counts = [M] * mom_all.shape[0] if counts is None else [int(c) for c in counts]
            _check_objective(objective, T, sum(counts))
        else:
            counts = [M]
            _check_objective(objective, T, M)
            mom, costs, _ = cost_moments(cost, states, None, inputs, cost_inputs)
            mom_all = mom.unsqueeze(0)
        rows, out = cost_rows(mom_all, counts, objective)
        ctx.cost, ctx.cost_inputs, ctx.objective, ctx.m_total = cost, cost_inputs, objective, sum(counts)
        if cost_inputs is None:
            ctx.save_for_backward(states.detach(), costs, rows)
        else:
            ctx.save_for_backward(states.detach(), costs, rows, inputs.detach().contiguous())
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cost, _g_std):
        states, costs, rows = ctx.saved_tensors[:3]
        inputs = ctx.saved_tensors[3] if ctx.cost_inputs is not None else None
        want_in = ctx.cost_inputs is not None and ctx.needs_input_grad[4]
        if g_cost is None:  # (only S is used downstream: no gradient goes through it)
            return torch.zeros_like(states), None, None, None, (torch.zeros_like(inputs) if want_in else None), None, None
        gc = g_cost.detach().to(dtype=DT).reshape(1).contiguous()  # stays on the device: no host sync
        g, g_in = _cost_bwd_shaped(ctx.cost, ctx.cost_inputs, ctx.objective, states.contiguous(), inputs, costs, rows, gc, ctx.m_total, want_in)
        return g, None, None, None, g_in, None, None


class ShapedLocalCostFunction(torch.autograd.Function):
    """LocalCostFunction under a PackedObjective: (share, sums [2T]) of a particle-sharded step; the sums are those of the plain cost (the
    pooled (J, S) are finalised from their all-reduced form with the weights: cost_from_sums(..., objective)).
      kappa == 0: share = sum_t w_t sum_m c_tm / m_total; the gradient needs nothing from the other ranks, the step keeps its ONE all-reduce.
      kappa != 0: the gradient factor holds the pooled (mean_t, std_t) of THIS step, so the forward all-reduces a copy of the 2T sums through
                  ``reducer`` (one additional small collective) and forms the pooled rows (mcp_cost_rows_sums) before the sweep.  The share's
                  value stays the mean part above (the value only feeds the NaN flag; the step's J comes from the reduced message).  A NaN on
                  another rank makes these rows NaN and this rank's gradient NaN -- harmless: the pooled cost is then non-finite on every rank
                  and the attempt is discarded, as without an objective."""

    @staticmethod
    def forward(ctx, states, cost, m_total, shift, sums_out, inputs, cost_inputs, objective, reducer):
        T, M = states.shape[0], states.shape[1]
        _check_objective(objective, T, m_total)
        if objective.kappa != 0.0 and reducer is None:
            raise ValueError("a sharded cost with risk != 0 needs the step's reducer for the pooled rows")
        mom, costs, _ = cost_moments(cost, states, None, inputs, cost_inputs)
        sums = sums_out[0] if sums_out is not None else torch.empty(2 * T, dtype=DT, device=states.device)
        if sums.numel() != 2 * T or sums.dtype != DT or not sums.is_contiguous():
            raise RuntimeError("sums_out must be a contiguous float64 tensor of 2 T entries")
        abi.check(abi.lib().mcp_cost_sums(T, M, abi.ptr(mom), abi.ptr(shift), abi.ptr(sums), abi.stream()), "mcp_cost_sums")
        rows, out = cost_rows(mom.unsqueeze(0), [M], objective.mean_part())
        local = out[0] * (float(M) / float(m_total))
        if objective.kappa != 0.0:
            rows, _ = cost_rows_sums(reducer.allreduce_(sums.clone()), m_total, shift, None, objective)
        ctx.cost, ctx.cost_inputs, ctx.objective, ctx.m_total = cost, cost_inputs, objective, int(m_total)
        if cost_inputs is None:
            ctx.save_for_backward(states.detach(), costs, rows)
        else:
            ctx.save_for_backward(states.detach(), costs, rows, inputs.detach().contiguous())
        ctx.mark_non_differentiable(sums)
        return local, sums

    @staticmethod
    def backward(ctx, g_local, _g_sums):
        states, costs, rows = ctx.saved_tensors[:3]
        inputs = ctx.saved_tensors[3] if ctx.cost_inputs is not None else None
        gc = g_local.detach().to(dtype=DT).reshape(1).contiguous()
        g, g_in = _cost_bwd_shaped(ctx.cost, ctx.cost_inputs, ctx.objective, states.contiguous(), inputs, costs, rows, gc, ctx.m_total,
                                   ctx.cost_inputs is not None and ctx.needs_input_grad[5])
        return g, None, None, None, None, g_in, None, None, None


# --------------------------------------------------------------------------------------
# single-step posterior (autograd)
# --------------------------------------------------------------------------------------
class PosteriorFunction(torch.autograd.Function):
    """Z [M,D] -> (mu [M,1], var [M]) = GP_prior.get_estimate_from_alpha on the packed GP."""

    @staticmethod
    def forward(ctx, Z, gp: PackedGP, status=None):
        Zc = Z.detach().to(dtype=DT).contiguous()
        M, D = Zc.shape
        need = ctx.needs_input_grad[0]
        mu = torch.empty(M, dtype=DT, device=Zc.device)
        var = torch.empty(M, dtype=DT, device=Zc.device)
        Jm = torch.empty(M, D, dtype=DT, device=Zc.device) if need else None
        Jv = torch.empty(M, D, dtype=DT, device=Zc.device) if need else None
        status = _status_word(status, Zc.device, "the test points' device")  # (None, nobody asked: the flags go to a scratch word)
        g = gp.to_c()
        abi.check(abi.lib().mcp_posterior_fwd_ex(C.byref(g), M, abi.ptr(Zc), abi.ptr(mu), abi.ptr(var), abi.ptr(Jm), abi.ptr(Jv), abi.ptr(status),
                                                 abi.stream(), C.byref(abi.DISPATCH)), "mcp_posterior_fwd")
        if need:
            ctx.save_for_backward(Jm, Jv)
        return mu.reshape(-1, 1), var

    @staticmethod
    def backward(ctx, g_mu, g_var):
        Jm, Jv = ctx.saved_tensors
        M, D = Jm.shape
        gz = torch.empty(M, D, dtype=DT, device=Jm.device)
        gm = (torch.zeros(M, dtype=DT, device=Jm.device) if g_mu is None else g_mu.reshape(-1)).contiguous()
        gv = (torch.zeros(M, dtype=DT, device=Jm.device) if g_var is None else g_var.reshape(-1)).contiguous()
        abi.check(abi.lib().mcp_posterior_bwd(M, D, abi.ptr(gm), abi.ptr(gv), abi.ptr(Jm), abi.ptr(Jv), abi.ptr(gz), abi.stream()),
                  "mcp_posterior_bwd")
        return gz, None, None


def posterior(gp: PackedGP, Z, status=None):
    """(mu [M,1], var [M]) at the test points Z [M,D], differentiable w.r.t. Z.  ``status``: an int32[1] on the device that the kernel ORs its
    flags INTO (MCP_STATUS_NAN, MCP_STATUS_NONPOS_VAR; decode with ``status_flags``), as ``rollout_open`` takes it; None: the flags are dropped."""
    return PosteriorFunction.apply(Z, gp, status)


def status_flags(status):
    """Decodes a device status word (synchronises)."""
    v = int(status.item())
    return {"nan": bool(v & abi.STATUS_NAN), "nonpos_var": bool(v & abi.STATUS_NONPOS_VAR), "not_spd": bool(v & abi.STATUS_NOT_SPD),
            "sync": bool(v & abi.STATUS_SYNC)}
