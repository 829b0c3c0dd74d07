"""CPU: the truth of the tanh-MLP policy with memory (tests/mlp_hist_models.hist_truth) and the class's torch formula
(Policy.MLP_policy(history=H).forward), without a GPU:
  - with W0's history columns zero the truth IS tests/mlp_models.mlp_truth of the network on block 0's columns (asserted exact);
  - the truth is sensitive to every plausible mistake -- zero padding in place of repeating row 0, the blocks oldest first, the oldest block
    dropped: each moves the inputs and g_x0 by more than 1e-6 of their largest entry, a thousand times the GPU tests' bounds (the variants
    run on the truth, not on a device);
  - MLP_policy(history=H).forward driven over the step order is the truth's law to 1e-14, errors and the PD term included;
  - history=1 is the class as it was: the same bits, no state, ``t`` optional;
  - what the class refuses."""
import pytest
import torch

import mlp_hist_models as hm
import mlp_models as mm

DT = torch.float64
CPU = torch.device("cpu")
# (shape, N, degree, T, M, hidden, H): sampled, the model's own feature lists (arm2: P0 = 6) or f = x
SMALL = [("arm2", 37, 0, 12, 17, (5,), 2), ("arm2", 37, 2, 6, 17, (7, 3), 4), ("arm2_delta", 37, 1, 2, 5, (5,), 4)]
# the identity with the plain network is one of bits: it holds where the matrix product adds the zero columns' exact zeros behind block 0's
# sum -- these shapes; the UR5 shape's 18 features leave room for H = 1 only, where it says that the window of one block is the plain map
IDENTITY = SMALL + [("ur5", 48, 1, 6, 5, (33, 64), 1)]
WRONG = SMALL + [("arm2", 37, 1, 6, 5, (7, 3), 3)]
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())


def _inputs(shape, N, deg, T, M, hidden, H):
    c, m, _ = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    x0, _, _, _, eps, w, wu = mm.inputs_for(c, M, T, seed=T * 100 + M)
    angle, non_angle = list(c["angle"]), list(c["not_angle"])
    P0 = len(non_angle) + 2 * len(angle)
    return c, m, x0, eps, w, wu, angle, non_angle, P0, hm.network(c, hidden, H * P0, 5)


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: "-".join(str(v) for v in c))
def test_zero_history_columns_are_the_plain_network(case):
    shape, N, deg, T, M, hidden, H = case
    c, m, x0, eps, w, wu, angle, non_angle, P0, params = _inputs(*case)
    torch.set_num_threads(1)
    zeroed = [q.clone() for q in params]
    zeroed[0][:, P0:] = 0
    a = hm.hist_truth(shape, m, x0, zeroed, eps, w, wu, True, angle, non_angle, H)
    plain = [q.clone() for q in params]
    plain[0] = plain[0][:, :P0].contiguous()
    b = mm.mlp_truth(shape, m, x0, plain, eps, w, wu, True, angle, non_angle)
    assert T < 2 or a[4] > 0.0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert torch.equal(a[2][0][:, :P0], b[2][0]) and all(torch.equal(p, q) for p, q in zip(a[2][1:], b[2][1:]))


@pytest.mark.parametrize("variant", hm.VARIANTS)
@pytest.mark.parametrize("case", WRONG, ids=lambda c: "-".join(str(v) for v in c))
def test_a_wrong_window_moves_the_truth(case, variant):
    shape, N, deg, T, M, hidden, H = case
    c, m, x0, eps, w, wu, angle, non_angle, P0, params = _inputs(*case)
    torch.set_num_threads(1)
    a = hm.hist_truth(shape, m, x0, params, eps, w, wu, True, angle, non_angle, H)
    b = hm.hist_truth(shape, m, x0, params, eps, w, wu, True, angle, non_angle, H, variant=variant)
    ei, ex = rel(b[1], a[1]), rel(b[3], a[3])
    print("%s on %s: inputs %.3e g_x0 %.3e" % (variant, "-".join(str(v) for v in case), ei, ex))
    assert ei > 1e-6 and ex > 1e-6


def _class_policy(c, params, hidden, H, angle, non_angle, target=None, idx=(), res=None):
    from mc_pilco_amd.policy_learning import Policy

    kw = dict(state_dim=c["S"], input_dim=c["U"], hidden_sizes=list(hidden), angle_indices=angle or None, non_angle_indices=non_angle or None, u_max=1.0,
              flg_squash=True, weight_init=params, dtype=DT, device=CPU, history=H)
    if len(idx):
        kw.update(target_traj=target, error_indices=list(idx))
    if res is None:
        return Policy.MLP_policy(**kw)
    return Policy.Residual_MLP_policy(**kw, sqrt_Kp_gains=res["kp"], sqrt_Kd_gains=res["kd"], pd_target_traj=res["target"], pd_pos_indices=res["pos"],
                                      pd_vel_indices=res["vel"])


@pytest.mark.parametrize("H,features,idx,with_res", [(2, "lists", (), False), (4, "lists", (), False), (3, "state", (), False), (4, "positions", (3, 0), False),
                                                     (3, "lists", (1, 2), True), (1, "lists", (), False)])
def test_forward_driven_over_the_step_order_is_the_truths_law(H, features, idx, with_res):
    c = mm.SHAPES["arm2"]
    T, M, hidden = 7, 5, (7, 3)
    angle, non_angle = hm.feature_lists(c, {} if features == "lists" else {"features": features})
    P0 = len(non_angle) + 2 * len(angle) if (angle or non_angle) else c["S"]
    gen = torch.Generator().manual_seed(12)
    rows = [torch.randn(M, c["S"], dtype=DT, generator=gen) for _ in range(T)]
    params = hm.network(c, hidden, H * P0 + len(idx), 3)
    target = hm.target_for(c, T, rows[0])
    res = None
    if with_res:
        kp, kd = hm.gains_for(c["U"], 3)
        res = dict(kp=kp, kd=kd, pos=[0, 1], vel=[2, 3], target=hm.target_for(c, T, rows[0], 1.3))
    pol = _class_policy(c, params, hidden, H, angle, non_angle, target, idx, res)
    assert pol.feature_dim == H * P0 + len(idx) and pol.history == H
    with torch.no_grad():
        for sweep in range(2):  # (t == 0 resets the window: the second pass gives the first pass's values)
            for t in range(T):
                u = pol(rows[t], t=t)
                ref = hm.hist_law(rows[:t + 1], params, angle, non_angle, H, target=target, idx=idx, res=res)
                assert float((u - ref).abs().max()) < 1e-14, (sweep, t)


def test_history_one_is_the_class_as_it_was():
    c = mm.SHAPES["arm2"]
    angle, non_angle, hidden = list(c["angle"]), list(c["not_angle"]), (7, 3)
    params = mm.network(c, hidden, angle, non_angle, 3)
    x = torch.randn(9, c["S"], dtype=DT, generator=torch.Generator().manual_seed(2))
    pol = _class_policy(c, params, hidden, 1, angle, non_angle)
    assert pol.history == 1 and pol.feature_dim == 6
    with torch.no_grad():
        f = torch.cat([x[:, non_angle], torch.sin(x[:, angle]), torch.cos(x[:, angle])], dim=1)  # the class's own statements, in its order
        h = f
        for l in range(2):
            h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
        want = pol.f_squash(h @ params[-2].t() + params[-1])
        assert torch.equal(pol.features(x), f)
        assert torch.equal(pol(x), want) and torch.equal(pol(x, t=5), want) and torch.equal(pol(x, t=2), want)  # no state: any t, or none
    assert pol._window is None and pol._t_prev is None
    from mc_pilco_amd.policy_learning import Policy

    old = Policy.MLP_policy(state_dim=4, input_dim=2, hidden_sizes=[7, 3], angle_indices=angle, non_angle_indices=non_angle, weight_init=params, dtype=DT,
                            device=CPU)  # (without the keyword)
    assert old.history == 1 and torch.equal(old(x), pol(x))
    wide = Policy.MLP_policy(state_dim=40, input_dim=2, hidden_sizes=[5], dtype=DT, device=CPU)  # (a width over 32 stays legal without memory)
    assert wide.feature_dim == 40


def test_what_the_class_refuses():
    from mc_pilco_amd.policy_learning import Policy

    c = mm.SHAPES["arm2"]
    angle, non_angle = list(c["angle"]), list(c["not_angle"])
    make = lambda H, **kw: Policy.MLP_policy(**dict(dict(state_dim=4, input_dim=2, hidden_sizes=[5], angle_indices=angle, non_angle_indices=non_angle, dtype=DT,
                                                         device=CPU, history=H), **kw))
    for H in (0, -1, 5):
        with pytest.raises(ValueError, match="history"):
            make(H)
    with pytest.raises(ValueError, match="at most 32"):
        make(4, target_traj=torch.zeros(3, 4, dtype=DT), error_indices=[0, 1, 2, 3], angle_indices=[0, 1, 2, 3], non_angle_indices=None)  # 4 * 8 + 4
    with pytest.raises(ValueError, match="at most 32"):
        make(2, state_dim=17, angle_indices=None, non_angle_indices=None)  # f = x: 34
    make(2, state_dim=16, angle_indices=None, non_angle_indices=None)  # 32 exactly
    pol = make(3)
    x = torch.zeros(5, 4, dtype=DT)
    with torch.no_grad():
        with pytest.raises(ValueError, match="pass t"):
            pol(x)
        with pytest.raises(ValueError, match="holds the window"):
            pol(x, t=1)  # nothing before it
        pol(x, t=0)
        pol(x, t=1)
        with pytest.raises(ValueError, match="holds the window"):
            pol(x, t=3)  # t = 2 was skipped
        with pytest.raises(ValueError, match="holds the window"):
            pol(x, t=1)  # repeated
        pol(x, t=2)
        with pytest.raises(ValueError, match="particles"):
            pol(torch.zeros(4, 4, dtype=DT), t=3)
        pol(torch.zeros(4, 4, dtype=DT), t=0)  # t == 0 resets, whatever the count
        pol(torch.zeros(4, 4, dtype=DT), t=1)


def test_ops_refuses_memory_on_a_measurement_before_anything_else():
    """ops.rollout_mlp with a measurement model and a packed policy of history > 1 raises before it looks at a tensor or makes a launch (no
    fused measured form is built); history = 1 goes on to the usual refusals."""
    from mc_pilco_amd import ops

    class Packed:
        history, params = 2, []

    with pytest.raises(RuntimeError, match="history > 1"):
        ops.rollout_mlp(None, Packed(), None, None, 5, meas=object())
    Packed.history = 1
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.rollout_mlp(None, Packed(), None, None, 5, meas=object())
