"""Extended-precision reference of the GP operators (helper of tests/test_gp_truth_cpu.py and tests/test_gpu_gp_operators.py; no tests here).

The truth is the exact value of the library's OWN formula (header comment of ``mcp_kernel``, include/mcpilco_hip.h) on the float64
operands exactly as the kernel receives them -- X, alpha, the symmetrised Kinv, 1/l, lambda, mean, w1, w20, w21, Z --, evaluated in
``np.longdouble`` where that carries a 64-bit significand (x86-64) and in mpmath at 113 bits elsewhere.  It does not depend on how
good Kinv is as an inverse.

  mu     = m + sum_j alpha_j k_j                                       S = |m| + sum_j |alpha_j k_j|
  var    = k(z,z) - k^T Kinv k                                         S = |k(z,z)| + sum_ij |k_i Kinv_ij k_j|
  Jmu_d  = sum_j alpha_j dk_j/dz_d                                     S = sum_j |alpha_j dk_j/dz_d|
  Jvar_d = dk(z,z)/dz_d - 2 sum_ij dk_i/dz_d Kinv_ij k_j               S = |dk(z,z)/dz_d| + 2 sum_ij |dk_i/dz_d Kinv_ij k_j|
  A G A                                                                S = |A| |G| |A|  (entrywise)

Errors are reported as r = |got - truth| / (2^-53 S): the a-priori form of a float64 sum's rounding error (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 4.2), independent of the order of summation and finite where mu cancels.

The bounds C (below) are NOT chosen from what the kernels give: C = 16 x r_orc rounded up to a power of two, where r_orc is the
worst r of the float64 CPU oracle (oracle/mcpilco_oracle.py, torch autograd for the Jacobians) against this truth over every case
of ``POSTERIOR_CASES`` -- the reference's own noise floor, measured by tests/test_gp_truth_cpu.py.  The factor 16 covers what differs
between two correct float64 evaluations: the kernels add the N terms in another tree, contract with fma, use their own exp and the
centred distance form (the oracle expands the square).
"""
import functools
import math

import numpy as np
import torch

U53 = 2.0 ** -53

# ----------------------------------------------------------------------------------------------------------------------------------
# recorded floor of the float64 oracle (worst r over all cases; tests/test_gp_truth_cpu.py re-measures and prints it) and the bounds
# ----------------------------------------------------------------------------------------------------------------------------------
R_ORC = {"mu": 1.889, "var": 1.145, "Jmu": 1.899, "Jvar": 1.799, "sandwich": 8.986}


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


C = {q: pow2_ceil(16.0 * v) for q, v in R_ORC.items()}

# (N, D, M): every Npad edge (N = 1, 15, 16, 17, 65, 129), M not a multiple of 2 / 4, the 15 / 16 boundary of phase J's operand form,
# both limits of the GP-input dimension, one shape with more than one chunk of Kinv columns and a real swarm of test points
SHAPES = [(1, 1, 1), (15, 3, 5), (16, 6, 7), (17, 6, 9), (65, 8, 13), (129, 15, 6), (129, 16, 6), (300, 6, 70), (200, 32, 5)]
DEGREES = [0, 1, 2]
# (N, D, M, degree, prior mean): the shapes above for every degree, one case with a prior mean, one per branch of the automatic dispatch
POSTERIOR_CASES = [(N, D, M, deg, 0.0) for (N, D, M) in SHAPES for deg in DEGREES]
MEAN_CASE = (65, 8, 13, 2, 0.7)
AUTO_CASES = [(65, 6, 300, 1, 0.0), (65, 6, 1030, 2, 0.0)]  # M = 300 -> 2 particles per workgroup, M = 1030 -> 4
ALL_POSTERIOR_CASES = POSTERIOR_CASES + [MEAN_CASE] + AUTO_CASES
SANDWICH_SIZES = [1, 17, 63, 64, 65, 129, 300]


# ----------------------------------------------------------------------------------------------------------------------------------
# the two extended-precision back ends
# ----------------------------------------------------------------------------------------------------------------------------------
class LongDouble:
    name = "longdouble"

    @staticmethod
    def up(a):
        return np.asarray(a, dtype=np.longdouble)

    exp = staticmethod(np.exp)
    log = staticmethod(np.log)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def down(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=np.longdouble)


class MpMath:
    """Object arrays of mpmath numbers at 113 bits (the significand of IEEE binary128)."""
    name = "mpmath113"

    def __init__(self):
        import mpmath

        self.ctx = mpmath.MPContext()
        self.ctx.prec = 113
        self._mpf = np.frompyfunc(lambda v: self.ctx.mpf(float(v)), 1, 1)
        self.exp = np.frompyfunc(self.ctx.exp, 1, 1)
        self.log = np.frompyfunc(self.ctx.log, 1, 1)
        self.sqrt = np.frompyfunc(self.ctx.sqrt, 1, 1)

    def up(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        return np.asarray(self._mpf(np.asarray(a, dtype=np.float64)), dtype=object).reshape(a.shape)

    @staticmethod
    def down(a):
        return np.asarray(a, dtype=object).astype(np.float64)

    def zeros(self, shape):
        return self.up(np.zeros(shape))


def backend():
    return LongDouble if np.finfo(np.longdouble).nmant >= 63 else MpMath()


def _np(a):
    return a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------------------------------
# the single-step posterior
# ----------------------------------------------------------------------------------------------------------------------------------
def posterior_truth(op, Z=None, be=None):
    """op: dict of float64 operands (X [N,D], alpha [N], Kinv [N,N] symmetric, inv_ls [D], lam, mean, deg, w1 [D+1], w20, w21 [D], Z [M,D]).
    Returns {"mu", "var" [M]; "Jmu", "Jvar" [M,D]} -> (value, term sum S), both in the back end's precision (and "kzz": the prior variance k(z,z))."""
    be = backend() if be is None else be
    up = be.up
    X, Zx = up(_np(op["X"])), up(_np(op["Z"] if Z is None else Z))
    alpha, Kinv, u = up(_np(op["alpha"]).reshape(-1)), up(_np(op["Kinv"])), up(_np(op["inv_ls"]).reshape(-1))
    lam, mean, deg = up(float(op["lam"])), up(float(op["mean"])), int(op["deg"])
    M, D = Zx.shape
    diff = Zx[:, None, :] - X[None, :, :]  # [M,N,D]
    su = diff * u
    kse = lam * be.exp(-(su * su).sum(2))  # [M,N]
    k = kse
    dk = -2 * (u * u) * diff * kse[:, :, None]  # [M,N,D]
    kzz = lam + be.zeros(M)
    dkzz = be.zeros((M, D))
    if deg >= 1:
        w1 = up(_np(op["w1"]).reshape(-1))
        zx = Zx[:, None, :] * X[None, :, :]
        k = k + (zx * w1[:D]).sum(2) + w1[D]
        dk = dk + (w1[:D] * X)[None, :, :]
        kzz = kzz + (w1[:D] * Zx * Zx).sum(1) + w1[D]
        dkzz = dkzz + 2 * w1[:D] * Zx
    if deg >= 2:
        w20, w21 = up(_np(op["w20"]).reshape(-1)), up(_np(op["w21"]).reshape(-1))
        A, B = (zx * w20).sum(2), (zx * w21).sum(2)  # [M,N]
        k = k + A * B
        dk = dk + (w20 * X)[None, :, :] * B[:, :, None] + A[:, :, None] * (w21 * X)[None, :, :]
        Sa, Sb = (w20 * Zx * Zx).sum(1), (w21 * Zx * Zx).sum(1)
        kzz = kzz + Sa * Sb
        dkzz = dkzz + 2 * Zx * (w20 * Sb[:, None] + w21 * Sa[:, None])
    ak, adk, aal, aKi = abs(k), abs(dk), abs(alpha), abs(Kinv)
    Kk, aKk = k @ Kinv, ak @ aKi  # [M,N]
    out = {"kzz": (kzz, abs(kzz))}
    out["mu"] = (mean + k @ alpha, abs(mean) + ak @ aal)
    out["var"] = (kzz - (Kk * k).sum(1), abs(kzz) + (aKk * ak).sum(1))
    out["Jmu"] = ((dk * alpha[None, :, None]).sum(1), (adk * aal[None, :, None]).sum(1))
    out["Jvar"] = (dkzz - 2 * (dk * Kk[:, :, None]).sum(1), abs(dkzz) + 2 * (adk * aKk[:, :, None]).sum(1))
    return out


def sandwich_truth(A, G, be=None):
    be = backend() if be is None else be
    A, G = be.up(_np(A)), be.up(_np(G))
    return A @ G @ A, abs(A) @ abs(G) @ abs(A)


def r_of(got, truth, S, be=None):
    """Worst r = |got - truth| / (2^-53 S) over the entries (float)."""
    be = backend() if be is None else be
    g = be.up(_np(got)).reshape(np.shape(truth))
    return float(np.max(be.down(abs(g - truth) / (be.up(U53) * S))))


# ----------------------------------------------------------------------------------------------------------------------------------
# cases (seeded; all float64 operands are produced once, here, and handed unchanged to the truth, the oracle and the kernels)
# ----------------------------------------------------------------------------------------------------------------------------------
def _targets(rs, X):
    return np.sin(X[:, 0] + X[:, min(1, X.shape[1] - 1)]) + 0.1 * rs.randn(X.shape[0])


@functools.lru_cache(maxsize=None)
def posterior_case(N, D, M, deg, mean):
    """X, Z uniform in [-1, 1]; lengthscales in [0.8, 1.6] sqrt(D); lambda 1.3; sigma_n 0.1; positive polynomial weights about 0.03;
    alpha / Kinv from the oracle's gp_alpha on Y = sin(x0 + x1) + noise.  The hyper-parameters are held as the oracle holds them (logs);
    the kernel's operands are the oracle's own float64 values exp(log l), exp(log lambda), ((k - d) exp(par))^2, so both evaluate the same model."""
    from oracle import mcpilco_oracle as orc

    rs = np.random.RandomState(1000 * N + 10 * D + deg)
    X = rs.uniform(-1.0, 1.0, (N, D))
    Z = rs.uniform(-1.0, 1.0, (M, D))
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    log_ls = torch.log(T(np.sqrt(D) * rs.uniform(0.8, 1.6, D)))
    pw = None if deg == 0 else [0.03 * (0.5 + rs.rand(D + 1))] + ([0.03 * (0.5 + rs.rand(2 * D))] if deg == 2 else [])
    h = orc.GPHyper(log_ls=log_ls, log_lambda=torch.log(T([1.3])), log_sigma_n=torch.log(T([0.1])), mean=T([mean]),
                    poly_log_par=None if pw is None else [torch.log(T(w)) for w in pw])
    Y = T(_targets(rs, X)).reshape(-1, 1) + mean
    with torch.no_grad():
        alpha, _, Kinv = orc.gp_alpha(h, T(X), Y)
        Kinv = ((Kinv + Kinv.t()) / 2).contiguous()
        ls, lam = torch.exp(h.log_ls), float(torch.exp(h.log_lambda))
        w1 = w20 = w21 = None
        if deg >= 1:
            s = orc.mpk_scales(h.poly_log_par[0], 1)[0]
            w1 = s * s
        if deg >= 2:
            s0, s1 = orc.mpk_scales(h.poly_log_par[1], 2)
            w20, w21 = s0 * s0, s1 * s1
    return dict(N=N, D=D, M=M, deg=deg, mean=float(mean), lam=lam, h=h, X=T(X), Z=T(Z), alpha=alpha.reshape(-1).contiguous(), Kinv=Kinv, ls=ls,
                inv_ls=1.0 / ls, w1=w1, w20=w20, w21=w21)


@functools.lru_cache(maxsize=None)
def posterior_case_truth(case):
    return posterior_truth(posterior_case(*case))


def oracle_posterior(op, Z=None):
    """mu, var, Jmu, Jvar of the float64 oracle (orc.gp_estimate_from_alpha, torch autograd for the Jacobians) on one thread."""
    from oracle import mcpilco_oracle as orc

    Zt = (op["Z"] if Z is None else Z).clone().requires_grad_(True)
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # (the floor is a recorded number: one summation order)
    try:
        mu, var = orc.gp_estimate_from_alpha(op["h"], op["X"], Zt, op["alpha"].reshape(-1, 1), op["Kinv"])
        Jmu = torch.autograd.grad(mu.sum(), Zt, retain_graph=True)[0]
        Jvar = torch.autograd.grad(var.sum(), Zt)[0]
    finally:
        torch.set_num_threads(n)
    return dict(mu=mu.detach().reshape(-1), var=var.detach(), Jmu=Jmu, Jvar=Jvar)


@functools.lru_cache(maxsize=None)
def sandwich_case(N):
    """A: a symmetric K^-1 (SE Gram of N points in [-1, 1]^3 + 0.1^2 I, inverted by the oracle's route), G: any matrix, NOT symmetric."""
    rs = np.random.RandomState(7000 + N)
    X = rs.uniform(-1.0, 1.0, (N, 3))
    K = np.exp(-((X[:, None, :] - X[None, :, :]) ** 2).sum(2) / 3.0) + 0.01 * np.eye(N)
    A = np.linalg.inv(K)
    A = (A + A.T) / 2
    G = rs.randn(N, N)
    return torch.as_tensor(A).contiguous(), torch.as_tensor(G).contiguous()


@functools.lru_cache(maxsize=None)
def sandwich_case_truth(N):
    return sandwich_truth(*sandwich_case(N))


# ----------------------------------------------------------------------------------------------------------------------------------
# the marginal likelihood
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nll_data(N, D, seed=0):
    """X uniform in [-1, 1]^D, Y = sin(x0 + x1) + 0.1 noise, lengthscales in [0.8, 1.6] sqrt(D) (float64 numpy)."""
    rs = np.random.RandomState(50000 + 100 * N + D + 7919 * seed)
    X = rs.uniform(-1.0, 1.0, (N, D))
    Y = _targets(rs, X).reshape(-1, 1)
    ls = np.sqrt(D) * rs.uniform(0.8, 1.6, D)
    return X, Y, ls


def nll_poly_weights(D, deg, seed=0):
    rs = np.random.RandomState(60000 + 10 * D + deg + 7919 * seed)
    return None if deg == 0 else [0.03 * (0.5 + rs.rand(D + 1))] + ([0.03 * (0.5 + rs.rand(2 * D))] if deg == 2 else [])


def nll_truth(X, Y, log_ls, log_lambda, log_sigma_n, mean=0.0, sigma_n_num=0.0, be=None):
    """SE marginal likelihood 1/2 ((Y-m)^T K^-1 (Y-m) + logdet K) and its gradient w.r.t. (log_ls [D], log_lambda, log_sigma_n, mean) from
    the float64 raw parameters, in extended precision: Cholesky by columns, K^-1 by two triangular solves,
    dL/dtheta = 1/2 tr((K^-1 - a a^T) dK/dtheta)."""
    be = backend() if be is None else be
    up = be.up
    X, Y = up(_np(X)), up(_np(Y)).reshape(-1)
    N, D = X.shape
    ls = be.exp(up(_np(log_ls)).reshape(-1))
    lam, sn = be.exp(up(float(log_lambda))), be.exp(up(float(log_sigma_n)))
    sq = ((X[:, None, :] - X[None, :, :]) / ls) ** 2  # [N,N,D]
    Kse = lam * be.exp(-sq.sum(2))
    K = Kse + (sn * sn + up(float(sigma_n_num)) ** 2) * up(np.eye(N))
    L = be.zeros((N, N))
    for j in range(N):  # Cholesky, lower, by columns
        d = K[j, j] - (L[j, :j] * L[j, :j]).sum()
        L[j, j] = be.sqrt(d)
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = be.zeros((N, N))  # L^-1 by forward substitution on the identity
    for j in range(N):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, N):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
    Kinv = Li.T @ Li
    r = Y - up(float(mean))
    a = Kinv @ r
    loss = (r @ a + 2 * be.log(np.diagonal(L)).sum()) / 2
    W = (Kinv - a[:, None] * a[None, :]) / 2
    g_ls = np.array([(W * (2 * sq[:, :, d] * Kse)).sum() for d in range(D)])
    g_lam = (W * Kse).sum()
    g_sn = np.trace(W) * 2 * sn * sn
    g_mean = -a.sum()
    return loss, g_ls, g_lam, g_sn, g_mean
