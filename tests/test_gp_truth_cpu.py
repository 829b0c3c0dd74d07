"""CPU: pins the extended-precision reference of tests/gp_truth.py, on which the bounds of tests/test_gpu_gp_operators.py rest.

  - the float64 oracle (orc.gp_estimate_from_alpha, torch autograd for the Jacobians; torch for A G A) agrees with the truth on every
    case the GPU tests run; its worst r per quantity -- the reference's own noise floor r_orc -- is printed and must still support the
    recorded bounds: gp_truth.C = 16 x R_ORC rounded up to a power of two, so r_orc <= C / 8 leaves the floor a factor two of drift
    (another BLAS, another summation order) before the derivation of C no longer holds;
  - conditions on the inputs: truth var > 1e-8 everywhere (the kernels' NONPOS_VAR path stays out of these tests), every term sum S
    finite and positive;
  - discrimination: the truth of a subtly different model (one alpha_j zeroed; two columns of Z's Jacobian swapped; w20 and w21
    exchanged where they act asymmetrically) sits at r > 100 C from the right one, so the bound would catch such a kernel;
  - the mpmath back end (used where long double is no wider than double) gives the long-double truth on a small case;
  - the marginal likelihood: orc.marginal_nll + autograd against the extended-precision loss and gradient at the two smallest N of the
    training-epoch cases;
  - the marginal-likelihood gradient OPERATOR (tests/test_gpu_nll_grad.py): the floor of a float64 torch evaluation of the library's formula
    over every case of gt.ALL_GRAD_CASES against gt.nll_grad_truth, the conditions on S, and three subtly wrong models the bound tells apart.
"""
import numpy as np
import pytest
import torch

import gp_truth as gt
from oracle import mcpilco_oracle as orc

QUANT = ("mu", "var", "Jmu", "Jvar")


def _floor():
    worst = {q: (0.0, None) for q in QUANT}
    for case in gt.ALL_POSTERIOR_CASES:
        op, tr = gt.posterior_case(*case), gt.posterior_case_truth(case)
        got = gt.oracle_posterior(op)
        for q in QUANT:
            r = gt.r_of(got[q], *tr[q])
            if r > worst[q][0]:
                worst[q] = (r, case)
    return worst


def test_oracle_floor_of_the_posterior_supports_the_recorded_bounds():
    worst = _floor()
    for q in QUANT:
        print("r_orc[%s] = %.3f at (N, D, M, deg, mean) = %s; recorded %.3f, C = %g" % (q, worst[q][0], worst[q][1], gt.R_ORC[q], gt.C[q]))
    for q in QUANT:
        assert gt.C[q] == gt.pow2_ceil(16.0 * gt.R_ORC[q])
        assert worst[q][0] <= gt.C[q] / 8.0, q


def test_oracle_floor_of_the_sandwich_supports_the_recorded_bound():
    worst = 0.0
    for N in gt.SANDWICH_SIZES:
        A, G = gt.sandwich_case(N)
        assert float((A - A.t()).abs().max()) == 0.0 and (N == 1 or float((G - G.t()).abs().max()) > 0.1)
        tr, S = gt.sandwich_case_truth(N)
        assert np.all(np.isfinite(gt.backend().down(S))) and np.all(gt.backend().down(S) > 0)
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            got = A @ G @ A
        finally:
            torch.set_num_threads(n)
        worst = max(worst, gt.r_of(got, tr, S))
    print("r_orc[sandwich] = %.3f; recorded %.3f, C = %g" % (worst, gt.R_ORC["sandwich"], gt.C["sandwich"]))
    assert gt.C["sandwich"] == gt.pow2_ceil(16.0 * gt.R_ORC["sandwich"])
    assert worst <= gt.C["sandwich"] / 8.0


@pytest.mark.parametrize("case", gt.ALL_POSTERIOR_CASES)
def test_conditions_on_the_posterior_cases(case):
    tr = gt.posterior_case_truth(case)
    down = gt.backend().down
    assert float(down(tr["var"][0]).min()) > 1e-8
    for q in QUANT:
        S = down(tr[q][1])
        assert np.all(np.isfinite(S)) and np.all(S > 0), q
        assert np.all(np.isfinite(down(tr[q][0]))), q


@pytest.mark.parametrize("deg", gt.DEGREES)
def test_the_bound_tells_a_subtly_different_model_apart(deg):
    case = (65, 8, 13, deg, 0.0)
    op, tr = gt.posterior_case(*case), gt.posterior_case_truth(case)

    def r_between(other, quantities):
        return {q: gt.r_of(gt.backend().down(other[q][0]), *tr[q]) for q in quantities}

    # one alpha_j zeroed (a dropped term of the mean contraction: the tail of a chunk, a padded row taken for a real one)
    wrong = dict(op)
    wrong["alpha"] = op["alpha"].clone()
    wrong["alpha"][op["N"] - 1] = 0.0
    for q, r in r_between(gt.posterior_truth(wrong), ("mu", "Jmu")).items():
        print("degree %d, alpha_j zeroed: r[%s] = %.3g" % (deg, q, r))
        assert r > 100.0 * gt.C[q], q
    # two columns of the Jacobians swapped (an index slip in the d loop)
    swapped = {q: (tr[q][0][:, [1, 0] + list(range(2, op["D"]))], None) for q in ("Jmu", "Jvar")}
    for q, r in r_between(swapped, ("Jmu", "Jvar")).items():
        print("degree %d, Jacobian columns swapped: r[%s] = %.3g" % (deg, q, r))
        assert r > 100.0 * gt.C[q], q
    if deg == 2:
        # w20 and w21 exchanged asymmetrically: k is symmetric in its two factors, so exchanging both changes nothing; the wrong model
        # is the one whose FIRST factor reads w21 (a kernel that takes the wrong weight vector for one operand)
        wrong = dict(op)
        wrong["w20"] = op["w21"]
        for q, r in r_between(gt.posterior_truth(wrong), QUANT).items():
            print("degree 2, w20 := w21: r[%s] = %.3g" % (q, r))
            assert r > 100.0 * gt.C[q], q


def test_mpmath_back_end_gives_the_long_double_truth():
    wide = np.finfo(np.longdouble).nmant >= 63  # (else long double is double: the two then differ by float64 rounding, a few units of r)
    op = gt.posterior_case(15, 3, 5, 2, 0.0)
    a, b = gt.posterior_truth(op, be=gt.LongDouble), gt.posterior_truth(op, be=gt.MpMath())
    for q in QUANT:
        va, Sa = gt.LongDouble.down(a[q][0]), gt.LongDouble.down(a[q][1])
        vb, Sb = gt.MpMath.down(b[q][0]), gt.MpMath.down(b[q][1])
        # two evaluations of 64 and 113 bits: they differ by a few 2^-64 S, far below one unit of r
        assert float(np.max(np.abs(va - vb) / (gt.U53 * Sa))) < (0.01 if wide else 64.0), q
        assert float(np.max(np.abs(Sa - Sb) / Sa)) < 1e-15, q


@pytest.mark.parametrize("N", [17, 31])
def test_oracle_marginal_likelihood_against_the_extended_precision_loss(N):
    """The float64 oracle the training-epoch tests compare with sits far inside their tolerances (loss rel 1e-9, gradient entries
    1e-7 max(1, |g|max)): asserted at a hundredth of them."""
    D = 6
    X, Y, ls = gt.nll_data(N, D)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    h = orc.GPHyper(log_ls=torch.log(T(ls)), log_lambda=torch.log(T([1.3])), log_sigma_n=torch.log(T([0.1])), mean=T([0.4]), sigma_n_num=0.05)
    prm = [h.log_ls, h.log_lambda, h.log_sigma_n, h.mean]
    for q in prm:
        q.requires_grad_(True)
    loss = orc.marginal_nll(h, T(X), T(Y))
    loss.backward()
    be = gt.backend()
    tl, g_ls, g_lam, g_sn, g_mean = gt.nll_truth(X, Y, h.log_ls.detach(), float(h.log_lambda.detach()), float(h.log_sigma_n.detach()), 0.4, 0.05)
    assert np.isfinite(float(be.down(tl)))
    e_loss = abs(float(loss) - float(be.down(tl))) / abs(float(be.down(tl)))
    want = np.concatenate([be.down(g_ls).reshape(-1), [float(be.down(g_lam)), float(be.down(g_sn)), float(be.down(g_mean))]])
    got = np.concatenate([q.grad.numpy().reshape(-1) for q in prm])
    e_grad = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    print("N = %d: oracle loss rel %.2e, worst gradient error %.2e" % (N, e_loss, e_grad))
    assert e_loss < 1e-11 and e_grad < 1e-9


# ----------------------------------------------------------------------------------------------------------------------------------
# the marginal-likelihood gradient operator
# ----------------------------------------------------------------------------------------------------------------------------------
GRAD_IDS = lambda c: "N%d-D%d-deg%d" % c


def test_float64_floor_of_the_nll_gradient_supports_the_recorded_bound():
    """r_orc: gt.nll_grad_float64 (float64 torch, one thread, the same formula on the same operands) against the truth, every case."""
    worst, where = 0.0, None
    for case in gt.ALL_GRAD_CASES:
        op = gt.nll_grad_case(*case)
        g, S = gt.nll_grad_case_truth(case)
        got = gt.nll_grad_float64(*gt.nll_grad_args(op)).numpy()
        live = gt.nll_grad_live(*case)
        assert np.all(got[~live] == 0.0), case
        r = float(gt.r_entries(got, g, S, live).max())
        print("r_orc[nll_grad] (N, D, deg) = %s: %.3f" % (case, r))
        if r > worst:
            worst, where = r, case
    print("r_orc[nll_grad] = %.3f at %s; recorded %.3f, C = %g" % (worst, where, gt.R_ORC["nll_grad"], gt.C["nll_grad"]))
    assert gt.C["nll_grad"] == gt.pow2_ceil(16.0 * gt.R_ORC["nll_grad"])
    assert worst <= gt.C["nll_grad"] / 8.0


@pytest.mark.parametrize("case", gt.ALL_GRAD_CASES, ids=GRAD_IDS)
def test_conditions_on_the_nll_gradient_cases(case):
    N, D, deg = case
    op = gt.nll_grad_case(*case)
    g, S = gt.nll_grad_case_truth(case)
    down, live = gt.backend().down, gt.nll_grad_live(*case)
    g, S = down(g), down(S)
    assert g.shape == S.shape == (4 * D + 3,) and live.sum() == (D if N > 1 else 0) + 2 + (D + 1) * (deg >= 1) + 2 * D * (deg >= 2)
    assert np.all(np.isfinite(S[live])) and np.all(S[live] > 0)
    assert np.all(np.isfinite(g[live])) and np.all(np.abs(g[live]) <= S[live])
    assert np.all(g[~live] == 0.0) and np.all(S[~live] == 0.0)
    assert np.array_equal(op["W"], op["W"].T) and op["W"].shape == (N, N) and op["alpha"].shape == (N,)


def test_the_nll_gradient_bound_tells_a_subtly_different_model_apart():
    case = gt.GRAD_VARIANT_CASE
    N, D, deg = case
    assert deg == 2
    op = gt.nll_grad_case(*case)
    g, S = gt.nll_grad_case_truth(case)
    be = gt.backend()
    bound = 100.0 * gt.C["nll_grad"]
    entries = lambda a, b: np.arange(a, b)

    def r_on(wrong, idx):
        mask = np.zeros(4 * D + 3, dtype=bool)
        mask[idx] = True
        return gt.r_entries(be.down(wrong), g, S, mask)

    # one alpha_i alpha_j term dropped from Wm (an off-diagonal one: it enters every sum but the trace)
    i, j = N - 1, 0
    W = op["W"].copy()
    W[i, j] += op["alpha"][i] * op["alpha"][j]  # (W_ij - a_i a_j + a_i a_j: the float64 rounding of this sum is far below the effect)
    args = list(gt.nll_grad_args(op))
    args[1] = W
    r = r_on(gt.nll_grad_truth(*args)[0], np.r_[entries(0, D + 1), entries(D + 2, 4 * D + 3)])
    print("alpha_i alpha_j dropped at (%d, %d): r >= %.3g" % (i, j, r.min()))
    assert r.min() > bound
    # a MPK_2 factor-0 entry formed with A instead of B:  2 w20_e x_ie x_je A_ij  (the truth of the model whose second factor reads w20)
    args = list(gt.nll_grad_args(op))
    args[7] = op["w20"]
    r = r_on(gt.nll_grad_truth(*args)[0], entries(2 * D + 3, 3 * D + 3))
    print("factor 0 with A for B: r >= %.3g" % r.min())
    assert r.min() > bound
    # inv_ls where inv_ls^2 belongs:  2 dx^2 / l  in the lengthscale entries
    wrong = g.copy()
    wrong[:D] = g[:D] / be.up(op["inv_ls"])
    r = r_on(wrong, entries(0, D))
    print("inv_ls for inv_ls^2: r >= %.3g" % r.min())
    assert r.min() > bound
