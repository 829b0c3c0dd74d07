"""Extended-precision reference of the GP operators (helper of tests/test_gp_truth_cpu.py, tests/test_gpu_gp_operators.py and
tests/test_gpu_nll_grad.py; no tests here).

The truth is the exact value of the library's OWN formula (header comment of ``mcp_kernel``, include/mcpilco_hip.h) on the float64
operands exactly as the kernel receives them -- X, alpha, the symmetrised Kinv, 1/l, lambda, mean, w1, w20, w21, Z --, evaluated in
``np.longdouble`` where that carries a 64-bit significand (x86-64) and in mpmath at 113 bits elsewhere.  It does not depend on how
good Kinv is as an inverse.

  mu     = m + sum_j alpha_j k_j                                       S = |m| + sum_j |alpha_j k_j|
  var    = k(z,z) - k^T Kinv k                                         S = |k(z,z)| + sum_ij |k_i Kinv_ij k_j|
  Jmu_d  = sum_j alpha_j dk_j/dz_d                                     S = sum_j |alpha_j dk_j/dz_d|
  Jvar_d = dk(z,z)/dz_d - 2 sum_ij dk_i/dz_d Kinv_ij k_j               S = |dk(z,z)/dz_d| + 2 sum_ij |dk_i/dz_d Kinv_ij k_j|
  A G A                                                                S = |A| |G| |A|  (entrywise)
  g_p    = 1/2 sum_ij (W_ij - alpha_i alpha_j) dK_ij/dtheta_p          S = 1/2 sum_ij (|W_ij| + |alpha_i alpha_j|) |dK_ij/dtheta_p|
           (the marginal-likelihood gradient operator, mcp_nll_grad's 4D + 3 log-parameters; W = Kinv, or any matrix)

Errors are reported as r = |got - truth| / (2^-53 S): the a-priori form of a float64 sum's rounding error (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 4.2), independent of the order of summation and finite where mu cancels.

The bounds C (below) are NOT chosen from what the kernels give: C = 16 x r_orc rounded up to a power of two, where r_orc is the
worst r of the float64 CPU oracle (oracle/mcpilco_oracle.py, torch autograd for the Jacobians) against this truth over every case
of ``POSTERIOR_CASES`` -- the reference's own noise floor, measured by tests/test_gp_truth_cpu.py.  The factor 16 covers what differs
between two correct float64 evaluations: the kernels add the N terms in another tree, contract with fma, use their own exp and the
centred distance form (the oracle expands the square).  For the gradient operator the floor is ``nll_grad_float64``, a float64 torch
evaluation of the same formula on the same operands, over ``ALL_GRAD_CASES``.
"""
import functools
import math

import numpy as np
import torch

U53 = 2.0 ** -53

# ----------------------------------------------------------------------------------------------------------------------------------
# recorded floor of the float64 oracle (worst r over all cases; tests/test_gp_truth_cpu.py re-measures and prints it) and the bounds
# ----------------------------------------------------------------------------------------------------------------------------------
R_ORC = {"mu": 1.889, "var": 1.145, "Jmu": 1.899, "Jvar": 1.799, "sandwich": 8.986, "nll_grad": 2.445}


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


# ----------------------------------------------------------------------------------------------------------------------------------
# the marginal-likelihood gradient operator (mcp_nll_grad and the gradient stage of mcp_nll_epoch), at operand level
# ----------------------------------------------------------------------------------------------------------------------------------
# (N, D, degree).  mcp_nll_grad directly: N below the segment count of nll_grad_row (256 / NPpad segments of NPpad >= 4D + 3 lanes), every
# NPpad boundary (32 | 64 at D = 7 | 8, 64 | 128 at 15 | 16, 128 | 256 at 31 | 32) at N = 257, the 256-stride of stage 1 and the tails of
# nll_colsum_kernel's four-way unroll (N mod 4 = 3, 0, 2, 3, 1), and the limit N = 4096 (133 KB of LDS)
GRAD_SMALL_CASES = [(1, 1, 0), (3, 2, 2), (7, 7, 2)]
GRAD_NPPAD_CASES = [(257, D, 2) for D in (7, 8, 15, 16, 31, 32)]
GRAD_STRIDE_CASES = [(255, 6, 0), (256, 6, 1), (258, 6, 2), (259, 6, 1), (1153, 6, 2)]
GRAD_LIMIT_CASE = (4096, 2, 1)
GRAD_VARIANT_CASE = (65, 8, 2)  # ldk > N, kern->scal, non-symmetric W with alpha = 0
GRAD_CASES = GRAD_SMALL_CASES + GRAD_NPPAD_CASES + GRAD_STRIDE_CASES + [GRAD_LIMIT_CASE, GRAD_VARIANT_CASE]
# mcp_nll_epoch, the LDS-rows form: nll_grad_rows_per_wg = 2 at N = 129; (257, 8): 3 rows per workgroup, the last one has 2; (1025, 6): a
# second pass of one thread over j; the last shapes before the form flips at D = 24 and at N = 1152
EPOCH_ROWS_CASES = [(129, 6, 0), (129, 6, 1), (129, 6, 2), (257, 8, 2), (1025, 6, 2), (681, 24, 1), (1152, 12, 2)]
# ... the row-per-workgroup form (nll_grad_batch_kernel): (N, D, degree, ard)
EPOCH_FALLBACK_CASES = [(530, 32, 2, True), (682, 24, 1, True), (682, 24, 0, False), (1152, 13, 0, True), (1152, 15, 2, True)]
EPOCH_BATCH_CASE = (530, 32, 1)  # G = 3, each GP with its own hyper-parameters and targets
ALL_GRAD_CASES = sorted(set(GRAD_CASES + EPOCH_ROWS_CASES + [c[:3] for c in EPOCH_FALLBACK_CASES] + [EPOCH_BATCH_CASE]))


def nll_grad_live(N, D, deg):
    """Which of the 4D + 3 entries have a term that is not identically zero: the slots of the degree, and the lengthscale entries from
    N = 2 on (dK_ii/d log l = 0: at N = 1 their only term vanishes, truth and S are exactly 0).  Every other entry must be exactly 0.0."""
    live = np.zeros(4 * D + 3, dtype=bool)
    live[:D] = N > 1
    live[D:D + 2] = True
    if deg >= 1:
        live[D + 2:2 * D + 3] = True
    if deg >= 2:
        live[2 * D + 3:] = True
    return live


def _row_block(N, D):
    return max(1, min(N, (1 << 20) // max(1, N * D)))


def nll_grad_truth(X, W, alpha, inv_ls, lam, w1, w20, w21, deg, be=None):
    """g_p = 1/2 sum_ij (W_ij - alpha_i alpha_j) dK_ij/dtheta_p for the 4D + 3 log-parameters of mcp_nll_grad (layout: its comment in
    include/mcpilco_hip.h; p = D + 1 is 1/2 tr(W - alpha alpha^T)), and S_p = 1/2 sum_ij (|W_ij| + |alpha_i alpha_j|) |dK_ij/dtheta_p|, from the
    float64 operands as the kernel receives them (W [N,N] general, NOT assumed symmetric).  Row blocks of W: nothing larger than about
    2^20 extended numbers lives at a time.  Every sum over j is a pairwise one along the contiguous axis and the rows are added the same
    way, so the truth's own error stays at a few 2^-64 S whatever N is (a running sum over N^2 = 2^24 terms would not)."""
    be = backend() if be is None else be
    up = be.up
    X, W, alpha, u = up(_np(X)), up(_np(W)), up(_np(alpha)).reshape(-1), up(_np(inv_ls)).reshape(-1)
    N, D = X.shape
    NP = 4 * D + 3
    lam, deg = up(float(lam)), int(deg)
    XT = np.ascontiguousarray(X.T)  # [D,N]
    u2 = (u * u)[None, :, None]
    if deg >= 1:
        w1 = up(_np(w1)).reshape(-1)
    if deg >= 2:
        w20, w21 = up(_np(w20)).reshape(-1), up(_np(w21)).reshape(-1)
    rows_g, rows_S = be.zeros((NP, N)), be.zeros((NP, N))  # [p][i]: the sums over j of row i
    b = _row_block(N, D)
    for i0 in range(0, N, b):
        I = slice(i0, min(N, i0 + b))
        Xi = X[I]  # [b,D]
        diff = Xi[:, :, None] - XT[None, :, :]  # [b,D,N]
        sq = diff * diff * u2  # ((x_ip - x_jp) / l_p)^2
        su = diff * u[None, :, None]
        kse = lam * be.exp(-(su * su).sum(1))  # [b,N]
        aa = alpha[I][:, None] * alpha[None, :]
        Wm, aWm = W[I] - aa, abs(W[I]) + abs(aa)

        def put(p, dK):  # dK [b,N] or [b,n,N] -> entries p, p + 1, ...
            dK = dK if dK.ndim == 3 else dK[:, None, :]
            n = dK.shape[1]
            rows_g[p:p + n, I] = (Wm[:, None, :] * dK).sum(2).T
            rows_S[p:p + n, I] = (aWm[:, None, :] * abs(dK)).sum(2).T

        put(0, 2 * sq * kse[:, None, :])
        put(D, kse)
        ii = np.arange(I.start, I.stop)
        rows_g[D + 1, I], rows_S[D + 1, I] = Wm[ii - i0, ii], aWm[ii - i0, ii]
        if deg >= 1:
            xx = Xi[:, :, None] * XT[None, :, :]  # [b,D,N]
            put(D + 2, 2 * w1[None, :D, None] * xx)
            put(2 * D + 2, 2 * w1[D] + 0 * kse)
        if deg >= 2:
            A, B = (xx * w20[None, :, None]).sum(1), (xx * w21[None, :, None]).sum(1)  # [b,N]
            put(2 * D + 3, 2 * w20[None, :, None] * xx * B[:, None, :])
            put(3 * D + 3, 2 * w21[None, :, None] * xx * A[:, None, :])
    return rows_g.sum(1) / 2, rows_S.sum(1) / 2


def nll_grad_float64(X, W, alpha, inv_ls, lam, w1, w20, w21, deg):
    """The same formula in float64 torch on one thread, vectorised the obvious way (row blocks, torch's own sums): a correct float64
    evaluation that shares nothing with the kernels.  Its worst r against nll_grad_truth is the floor R_ORC["nll_grad"]."""
    T = lambda a: torch.as_tensor(_np(a))
    X, W, alpha, u = T(X), T(W), T(alpha).reshape(-1), T(inv_ls).reshape(-1)
    N, D = X.shape
    lam, deg = float(lam), int(deg)
    g = torch.zeros(4 * D + 3, dtype=torch.float64)
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # (the floor is a recorded number: one summation order)
    try:
        b = _row_block(N, D)
        for i0 in range(0, N, b):
            Xi = X[i0:i0 + b]
            diff = Xi[:, None, :] - X[None, :, :]  # [b,N,D]
            sq = (diff * u) ** 2
            kse = lam * torch.exp(-sq.sum(2))
            Wm = W[i0:i0 + b] - alpha[i0:i0 + b, None] * alpha[None, :]
            Wk = Wm * kse
            g[:D] += (Wk[:, :, None] * (2.0 * sq)).sum((0, 1))
            g[D] += Wk.sum()
            g[D + 1] += torch.diagonal(Wm, offset=i0).sum()
            if deg >= 1:
                w1t = T(w1).reshape(-1)
                xx = Xi[:, None, :] * X[None, :, :]
                g[D + 2:2 * D + 2] += (Wm[:, :, None] * (2.0 * w1t[:D] * xx)).sum((0, 1))
                g[2 * D + 2] += (Wm * (2.0 * w1t[D])).sum()
            if deg >= 2:
                w20t, w21t = T(w20).reshape(-1), T(w21).reshape(-1)
                A, B = (xx * w20t).sum(2), (xx * w21t).sum(2)
                g[2 * D + 3:3 * D + 3] += ((Wm * B)[:, :, None] * (2.0 * w20t * xx)).sum((0, 1))
                g[3 * D + 3:] += ((Wm * A)[:, :, None] * (2.0 * w21t * xx)).sum((0, 1))
    finally:
        torch.set_num_threads(n)
    return 0.5 * g


def nll_kernel_operands(D, deg, ls, pw, lam=1.3):
    """float64 kernel operands of the model (lengthscales ls, lambda, raw polynomial weights pw): 1 / l, lambda and the MPK weights
    ((k - d) exp(log pw))^2 as the library's host layer forms them."""
    op = dict(D=D, deg=deg, lam=float(lam), inv_ls=1.0 / np.asarray(ls, dtype=np.float64), w1=None, w20=None, w21=None)
    if deg >= 1:
        op["w1"] = np.exp(np.log(pw[0])) ** 2
    if deg >= 2:
        lp = np.log(pw[1])
        op["w20"], op["w21"] = (2.0 * np.exp(lp[:D])) ** 2, np.exp(lp[D:]) ** 2
    return op


@functools.lru_cache(maxsize=None)
def nll_grad_case(N, D, deg, seed=0):
    """Seeded operands of one case: nll_data's inputs, targets and lengthscales, nll_poly_weights' polynomial weights, lambda 1.3,
    sigma_n 0.1; Kinv = numpy's inverse of the case's own K, symmetrised; alpha = Kinv Y.  Everything float64 numpy, made once."""
    X, Y, ls = nll_data(N, D, seed)
    op = nll_kernel_operands(D, deg, ls, nll_poly_weights(D, deg, seed))
    K = np.empty((N, N))
    b = _row_block(N, D)
    for i0 in range(0, N, b):  # (row blocks: no N x N x D array at N = 4096)
        su = (X[i0:i0 + b, None, :] - X[None, :, :]) * op["inv_ls"]
        K[i0:i0 + b] = op["lam"] * np.exp(-(su * su).sum(2))
    if deg >= 1:
        K += (X * op["w1"][:-1]) @ X.T + op["w1"][-1]
    if deg >= 2:
        K += ((X * op["w20"]) @ X.T) * ((X * op["w21"]) @ X.T)
    K += 0.1 ** 2 * np.eye(N)
    Kinv = np.linalg.inv(K)
    Kinv = np.ascontiguousarray((Kinv + Kinv.T) / 2)
    op.update(N=N, X=X, Y=Y, ls=ls, W=Kinv, alpha=(Kinv @ Y).reshape(-1))
    return op


def nll_grad_args(op):
    return (op["X"], op["W"], op["alpha"], op["inv_ls"], op["lam"], op["w1"], op["w20"], op["w21"], op["deg"])


@functools.lru_cache(maxsize=None)
def nll_grad_case_truth(case):
    return nll_grad_truth(*nll_grad_args(nll_grad_case(*case)))


def r_entries(got, truth, S, live, be=None):
    """r = |got - truth| / (2^-53 S) of the live entries (float64 array)."""
    be = backend() if be is None else be
    g = be.up(_np(got)).reshape(np.shape(truth))
    return be.down(abs(g - truth)[live] / (be.up(U53) * S[live]))
