"""GPU parity at BASELINE.json's real training-set sizes, against an independent answer (the CPU oracle on the same seeded
inputs and the same noise): N=300 SE, N=300 SE+poly(2), N=400 / D=24 / G=6 UR5-shaped -- on EVERY forward kernel variant
(1 / 2 / 4 / 16 particles per workgroup, unsharded and GP-sharded) and every backward sweep width (1 / 2 / 4).  This is where
the tail-chunk paths of phase V (Npad = 304: a 48-row tail chunk; Npad = 400: a 16-row one), the alpha padding at Npad != N and
the tile kernel's uneven block split are exercised against something that is not another variant of the same code.
Plus: BASELINE.json's configs[4] at its stated size (UR5, M=2000, T=300, N=400) through size-independent properties, and
real statistics of the in-kernel Philox noise (the mode every benchmark number is produced in).

Tolerances (fp64): the oracle factorises K itself (torch Cholesky) and the HIP path its own way, so trajectories agree to the
conditioning of K: states / inputs abs 1e-7 over 8 steps, cost rel 1e-9, gradients rel 1e-6 (tests/test_gpu_parity.py:238-243).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import mcpilco_oracle as orc

pytestmark = pytest.mark.gpu

Tt = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)

REAL = {"se300": ("c1", 48, 8), "sep2_300": ("c3", 48, 8), "ur5_400": ("c5", 40, 6), "se300_long": ("c1", 32, 150), "sep1_300": ("c2p1_script", 48, 8),
        # round 5: the training sets the launch scripts grow to (4th entry: N) -- the lean kernel beyond Npad = 384
        "se360": ("c1", 48, 8, 360), "sep2_360": ("c3", 48, 8, 360), "se450": ("c1", 48, 8, 450), "sep1_500": ("c2p1_script", 48, 8, 500),
        "se620": ("c1", 48, 8, 620), "ur5se_400": ("ur5_se", 40, 6),
        # beyond the 1024 rows the fused kernels took until round 4 (the reference factorises any N: GP_prior.py:106-110)
        "se1500": ("c1", 24, 6, 1500), "sep2_1100": ("c3", 24, 6, 1100)}


def _real(key):
    v = REAL[key]
    return v if len(v) == 4 else v + (None,)


@contextlib.contextmanager
def one_cpu_thread():
    """The oracle's answer on one CPU thread: the BLAS splits its sums by the thread count, and at the tolerances below the answer must not
    depend on how many cores the host lends torch (1 vs 8 threads moves the oracle's own states / inputs by up to 2.5e-9 at N = 300)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(nt)


@functools.lru_cache(maxsize=None)
def oracle_answer(key):
    """(cost, std, grads, states, inputs, x0, eps, masks) of the CPU oracle at the real N, small M and T, its own pretrain."""
    with one_cpu_thread():
        return _oracle_answer(key)


def _oracle_answer(key):
    from mc_pilco_amd import workloads

    name, M, Tn, Ntr = _real(key)
    pb = workloads.numpy_problem(name, N=Ntr)
    c = pb["cfg"]
    if pb["target_traj"] is not None:
        from mc_pilco_amd import synthetic as sy

        pb["target_traj"] = sy.ur5_target_traj(T=Tn, Ts=c["Ts"])
    hyp = []
    for g in range(c["G"]):
        pw = None if pb["poly"] is None else [torch.log(Tt(w)) for w in pb["poly"][g]]
        hyp.append(orc.GPHyper(torch.log(Tt(c["lengthscales"])), torch.log(Tt([c["lam"]])), torch.log(Tt([c["sigma_n"]])), poly_log_par=pw))
    caches = [orc.pretrain_gp(hyp[g], Tt(pb["Z"]), Tt(pb["Ys"][g])) for g in range(c["G"])]
    m = orc.SpeedModel(hyp, caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    pi = pb["policy"]
    pp = orc.PolicyPar(torch.log(Tt(pi["lengthscales"])).reshape(1, -1), Tt(pi["centers"]), Tt(pi["weight"]), c["u_max"], pb["policy_kind"],
                       target_traj=None if pb["target_traj"] is None else Tt(pb["target_traj"]), **pb["policy_extra"])
    if pb["system"] == "cartpole":
        cost_fn = lambda st: orc.cart_pole_cost(st, Tt(c["cost_target"]), Tt(c["cost_ls"]), c["cost_angle_index"], c["cost_pos_index"])
    else:
        tt, ls = Tt(pb["target_traj"]), Tt(c["cost_ls"])
        cost_fn = lambda st: orc.traj_cost(st, tt, ls)
    p = 0.25
    torch.manual_seed(17)
    e0, eps, masks = orc.draw_noise(M, c["S"], c["G"], c["B"], Tn, p)
    x0 = orc.sample_x0(Tt(c["x0_mean"]), Tt(c["x0_var"]), M, e0)
    oc, os_, og, ost, oin = orc.policy_grad_step(m, pp, x0, Tn, cost_fn, p, eps, masks)
    return dict(cost=float(oc), std=float(os_), grads=og, states=ost, inputs=oin, x0=x0, eps=eps, masks=masks, p=p, N=pb["Z"].shape[0],
                caches=caches, problem=pb)


@functools.lru_cache(maxsize=None)
def hip_workload(key):
    from gpu_helpers import dev
    from mc_pilco_amd import workloads

    name, M, Tn, Ntr = _real(key)
    return workloads.build(name, device=dev(), M=M, T=Tn, N=Ntr)  # pretrain (Gram -> Cholesky -> inverse -> alpha) on the device


@functools.lru_cache(maxsize=None)
def hip_workload_on_oracle_operands(key):
    """The HIP descriptors packed from the ORACLE's own pretrain (its Kinv and alpha, torch Cholesky): both sides then evaluate the
    same posterior operands and only the rollout / adjoint kernels differ."""
    from gpu_helpers import G, dev
    from mc_pilco_amd import ops, workloads

    name, M, Tn, Ntr = _real(key)
    o = oracle_answer(key)
    # (the model of `build` is replaced below: beyond the device factorisation's own size limit a smaller one is built for the rest)
    w = workloads.build(name, device=dev(), M=M, T=Tn, N=Ntr if (Ntr or 0) <= 1000 else 300)
    pb, c = o["problem"], o["problem"]["cfg"]
    gps = []
    for g in range(c["G"]):
        spec = workloads.spec_for(c, c["sigma_n"], None if pb["poly"] is None else pb["poly"][g])
        cache = o["caches"][g]
        gps.append(ops.PackedGP(spec, G(cache.X.numpy()), G(cache.alpha.numpy()), G(cache.Kinv.numpy())))
    w.model = ops.PackedModel(gps, c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    return w


ACHIEVED = {}


@pytest.mark.parametrize("pb", [1, 2, 4])
@pytest.mark.parametrize("code", [1, 2, 4, 16, 101, 102, 104, 116, 201, 202, 204])
@pytest.mark.parametrize("key", ["se300", "sep2_300", "ur5_400", "sep1_300"])
def test_rollout_kernels_alone_against_the_oracle_at_real_sizes(key, code, pb):
    """with each side factorising K itself, the real-size comparison could only hold 1e-7 (the conditioning of K).
    Here the HIP rollout runs on the oracle's OWN Kinv / alpha (N = 300, 300 + poly(2), 400 / D = 24): what differs is the rollout and
    adjoint kernels alone -- states abs 1e-9, inputs abs 2e-9 (|u| <= u_max = 10: 2e-10 relative), cost rel 1e-11, gradients rel
    1e-9, on every forward variant x backward width.  The maxima reached are printed (pytest -s) and kept in ACHIEVED; round 3, all
    variants alike: states 4e-11 .. 9e-10, inputs 3e-11 .. 1.4e-9, cost rel <= 8e-13, gradients rel <= 4e-11 -- the summation order
    of the N = 300 contractions against a Kinv of condition 5e5, not a property of any one kernel."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import ops

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    with forced_variant(code, bwd_particles=pb) as fv:
        st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
        c, s = ops.expected_cost(w.cost, st)
        c.backward()
        fv.check(sharding_optional=(key == "ur5_400"), lean_expected=(key in ("se300", "sep2_300", "sep1_300")) if code >= 200 else None)
    assert int(status.item()) == 0
    es = float((st.detach().cpu() - o["states"]).abs().max())
    eu = float((inp.detach().cpu() - o["inputs"]).abs().max())
    ec = abs(float(c) - o["cost"]) / abs(o["cost"])
    eg = max(float((q.grad.cpu().reshape(o["grads"][k].shape) - o["grads"][k]).abs().max()) / float(o["grads"][k].abs().max())
             for q, k in zip(w.params, ["log_ls", "centers", "weight"]))
    ACHIEVED[(key, code, pb)] = (es, eu, ec, eg)
    print("real-size parity %s code %d bwd %d: states %.2e inputs %.2e cost rel %.2e grad rel %.2e" % (key, code, pb, es, eu, ec, eg))
    assert es < 1e-9 and eu < 2e-9
    assert ec < 1e-11
    assert eg < 1e-9


@pytest.mark.parametrize("code", [201, 202, 204, 4])
@pytest.mark.parametrize("key", ["se360", "sep2_360", "se450", "sep1_500", "se620"])
def test_lean_kernel_beyond_npad_384_against_the_oracle(key, code):
    """Round 5: `rollout_fwd_lat_kernel` takes Npad up to 640 (SE; SE + polynomial(1) to 512, (2) to 384): beyond 24 row tiles a wave streams
    two segments of Kinv, phase K takes 4 or 5 items per thread, and the second copy of X^T in LDS is gone (phase J sums against X^T / l
    with a ones row).  N = 360 (SE, SE + poly(2): where the cart-pole scripts end), 450 (test_mcpilco4pms_cartpole.py's last trial), 500
    (degree 1, KR = 4), 620 (KR = 5, 39 row tiles) on the oracle's own operands: states abs 3e-9, inputs 6e-9 (|u| <= 10), cost rel 1e-11,
    gradients rel 1e-9.  Measured: lean 8.6e-10 .. 2.0e-9 / 2.7e-9 .. 4.6e-9, the general kernel (code 4, another summation order) 9.4e-10 ..
    1.4e-9 / 2.4e-9 .. 4.0e-9 on the same cases -- Kinv of 450 - 620 points of a smooth trajectory is worse conditioned than at N = 300,
    where 1e-9 / 2e-9 hold; cost and gradients sit at 1e-12 / 1e-10 as there."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import ops

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    assert w.model.gps[0].N == _real(key)[3]
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    with forced_variant(code) as fv:
        st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
        c, s = ops.expected_cost(w.cost, st)
        c.backward()
        fv.check(lean_expected=True if code >= 200 else None)
    assert int(status.item()) == 0
    es = float((st.detach().cpu() - o["states"]).abs().max())
    eu = float((inp.detach().cpu() - o["inputs"]).abs().max())
    ec = abs(float(c) - o["cost"]) / abs(o["cost"])
    eg = max(float((q.grad.cpu().reshape(o["grads"][k].shape) - o["grads"][k]).abs().max()) / float(o["grads"][k].abs().max())
             for q, k in zip(w.params, ["log_ls", "centers", "weight"]))
    print("beyond 384: %s code %d: states %.2e inputs %.2e cost rel %.2e grad rel %.2e" % (key, code, es, eu, ec, eg))
    assert es < 3e-9 and eu < 6e-9 and ec < 1e-11 and eg < 1e-9


@pytest.mark.parametrize("code", [0, 1, 2, 101])
@pytest.mark.parametrize("key", ["se1500", "sep2_1100"])
def test_rollout_beyond_1024_training_points(key, code):
    """N = 1500 (SE) and 1100 (SE + polynomial(2)) through the fused rollout and its adjoint: round 4 answered MCP_ERR_LIMIT beyond 1024 rows per
    GP (a table size); the small-tile kernels stream any Kinv the chunk tables hold (MCP_MAX_TRAIN = 4096), unsharded and GP-sharded.  The
    oracle's own operands; Kinv of 1500 points of a smooth trajectory is ill conditioned, so states / inputs hold abs 2e-8, cost rel 1e-10,
    gradients rel 1e-8 (printed).  Forced codes are requests here: a tile size whose operands do not fit the LDS at this N falls back to a smaller
    one (what ran is printed)."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    assert w.model.gps[0].N == _real(key)[3] > 1024
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    with forced_variant(code) as fv:
        st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
        c, s = ops.expected_cost(w.cost, st)
        c.backward()
        ran = (hipabi.lib().mcp_debug_last_particles_per_wg(), hipabi.lib().mcp_debug_last_gp_sharded())
    assert int(status.item()) == 0
    es = float((st.detach().cpu() - o["states"]).abs().max())
    eu = float((inp.detach().cpu() - o["inputs"]).abs().max())
    ec = abs(float(c) - o["cost"]) / abs(o["cost"])
    eg = max(float((q.grad.cpu().reshape(o["grads"][k].shape) - o["grads"][k]).abs().max()) / float(o["grads"][k].abs().max())
             for q, k in zip(w.params, ["log_ls", "centers", "weight"]))
    print("beyond 1024: %s code %d (ran: %d particles per workgroup, GP-sharded launches %d): states %.2e inputs %.2e cost rel %.2e grad rel %.2e" % ((key, code) + ran + (es, eu, ec, eg)))
    assert es < 2e-8 and eu < 2e-8 and ec < 1e-10 and eg < 1e-8


@pytest.mark.parametrize("code", [0, 16])
def test_long_horizon_against_the_oracle_at_n300(code):
    """T = 150, M = 32, N = 300 (SE), the oracle's own operands and noise, on the automatic dispatch (the lean GP-sharded kernel) and
    on the 16-particle tile kernel: the only place long-horizon error growth at the real N would show.  SURVEY 8c: abs 1e-6 on
    states, rel 1e-6 on gradients."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops

    key = "se300_long"
    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    assert w.T == 150 and w.model.gps[0].N == 300
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    with forced_variant(code) as fv:
        st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
        c, s = ops.expected_cost(w.cost, st)
        c.backward()
        fv.check()
        if code == 0:
            assert hipabi.lib().mcp_debug_last_fwd_lean() == 1  # what bench.py's headline runs
    assert int(status.item()) == 0
    es = float((st.detach().cpu() - o["states"]).abs().max())
    eu = float((inp.detach().cpu() - o["inputs"]).abs().max())
    print("long horizon code %d: states %.2e inputs %.2e cost rel %.2e" % (code, es, eu, abs(float(c) - o["cost"]) / abs(o["cost"])))
    assert es < 1e-6 and eu < 1e-6
    assert abs(float(c) - o["cost"]) < 1e-8 * abs(o["cost"])
    for q, k in zip(w.params, ["log_ls", "centers", "weight"]):
        g = o["grads"][k]
        assert float((q.grad.cpu().reshape(g.shape) - g).abs().max()) < 1e-6 * float(g.abs().max()), k


@pytest.mark.parametrize("name", ["c1", "c2_script", "pms_script", "c2p1_script", "c2_script+pms", "c2p1_script+pms"])
def test_lean_kernel_draws_the_same_dropout_bits_and_noise_as_the_general_one(name):
    """Philox mode (what every benchmark number runs in): the lean kernel's dropout decisions, process noise and (measurement model)
    position noise are the general kernels' -- identical counters, so the trajectories agree to rounding (different summation
    orders), far below what one flipped keep bit or a different normal would cause.  SE, SE + polynomial(2) and the measurement
    model of MC_PILCO4PMS, and their combinations (every instantiation family of the lean kernel: degree 0 / 1 / 2 x with / without the
    measurement model x 1 / 2 / 4 particles per workgroup); the cluster sizes reproduce each other bit for bit."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops, workloads

    w = workloads.build(name.split("+")[0], device=dev(), M=96, T=10)
    if name.endswith("+pms"):  # (polynomial kernel AND measurement model: the <., ., 1 / 2, true> instantiations)
        from scipy import signal

        bb, aa = signal.butter(1, 0.5)
        w.meas = ops.MeasSpec(pos=[0, 2], vel=[1, 3], std_pos=[3e-3, 3e-3], b=bb, a=aa)
    assert (w.meas is not None) == ("pms" in name)
    torch.manual_seed(4)
    x0 = w.sample_x0()
    outs = {}
    with torch.no_grad():
        for code in (4, 104, 204, 202, 201):
            with forced_variant(code) as fv:
                outs[code] = ops.rollout(w.model, w.policy, ops.NoiseSpec(seed=11, call=3), x0, w.T, w.p_drop, meas=w.meas)
                fv.check(lean_expected=True if code >= 200 else None)
    for code in (104, 204, 202, 201):
        assert int(outs[code][2].item()) == 0
        assert float((outs[code][0] - outs[4][0]).abs().max()) < 5e-9 and float((outs[code][1] - outs[4][1]).abs().max()) < 5e-9
    for code in (202, 201):  # the lean kernel does not depend on P
        assert torch.equal(outs[204][0], outs[code][0]) and torch.equal(outs[204][1], outs[code][1])


@pytest.mark.parametrize("pb", [1, 2, 4])
@pytest.mark.parametrize("code", [1, 2, 4, 16, 101, 102, 104, 116, 201, 202, 204])
@pytest.mark.parametrize("key", ["se300", "sep2_300", "ur5_400"])
def test_every_variant_against_the_oracle_at_real_training_set_sizes(key, code, pb):
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import ops

    o = oracle_answer(key)
    w = hip_workload(key)
    assert w.model.gps[0].N == o["N"] and o["N"] in (300, 400)
    nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    for q in w.params:
        q.grad = None
    with forced_variant(code, bwd_particles=pb) as fv:
        st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
        c, s = ops.expected_cost(w.cost, st)
        c.backward()
        fv.check(sharding_optional=(key == "ur5_400"))
    assert int(status.item()) == 0
    assert float((st.detach().cpu() - o["states"]).abs().max()) < 1e-7
    assert float((inp.detach().cpu() - o["inputs"]).abs().max()) < 1e-7
    assert abs(float(c) - o["cost"]) < 1e-9 * abs(o["cost"])
    assert abs(float(s) - o["std"]) < 1e-7 * max(abs(o["std"]), 1e-3)
    for q, k in zip(w.params, ["log_ls", "centers", "weight"]):
        g = o["grads"][k]
        assert float((q.grad.cpu().reshape(g.shape) - g).abs().max()) < 1e-6 * float(g.abs().max()), k


@pytest.mark.parametrize("key", ["ur5_400", "sep2_300"])
@pytest.mark.parametrize("mode", ["masks", "philox"])
def test_policy_split_over_the_cluster_of_the_gp_sharded_tile_kernel(key, mode):
    """Round 4: in the GP-sharded 16-particle kernel the members of a cluster no longer evaluate the whole policy each; member c takes its
    share of the basis functions and the partial sums W phi go round (`FwdArgs.uxch`).  Same states / inputs / cost as with the split off
    (`mcp_debug_set_policy_split(0)`: the round-3 form) up to the summation order of W phi, identical dropout bits in Philox
    mode (a wrong keep bit shows in the first digits), bitwise reproducible, and against the oracle at 1e-9 with recorded masks."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    if mode == "masks":
        nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    else:
        nz = ops.NoiseSpec(seed=11, call=2)
    L = hipabi.lib()
    out = {}
    try:
        for split in (1, 0, 1):
            L.mcp_debug_set_policy_split(1 if split else 0)
            with forced_variant(116) as fv, torch.no_grad():
                st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
                assert L.mcp_debug_last_gp_sharded() == 1, "the shape was expected to run GP-sharded"
            assert int(status.item()) == 0
            if split in out:
                assert torch.equal(out[split][0], st) and torch.equal(out[split][1], inp)  # bitwise reproducible
            out[split] = (st.clone(), inp.clone())
    finally:
        L.mcp_debug_set_policy_split(-1)
    # the first step differs by the summation order of W phi alone; later steps by what Kinv (condition 5e5) makes of it -- the same
    # distance either form keeps from the oracle
    assert float((out[1][1][0] - out[0][1][0]).abs().max()) < 1e-13
    assert float((out[1][0] - out[0][0]).abs().max()) < 2e-9 and float((out[1][1] - out[0][1]).abs().max()) < 4e-9
    assert not torch.equal(out[1][1], torch.zeros_like(out[1][1]))
    if mode == "masks":
        assert float((out[1][0].cpu() - o["states"]).abs().max()) < 1e-9 and float((out[1][1].cpu() - o["inputs"]).abs().max()) < 2e-9


ROW_SPLIT_FORMS = [(2, 0), (2, 1), (3, 1)]  # (row parts, deal of the workgroups: 0 a tile's members on one XCD, 1 row part major -- round 6)


@pytest.mark.parametrize("key", ["ur5_400", "ur5se_400"])
@pytest.mark.parametrize("mode", ["masks", "philox"])
@pytest.mark.parametrize("parts,cmap", ROW_SPLIT_FORMS)
def test_row_split_cluster_of_the_gp_sharded_tile_kernel(key, mode, parts, cmap):
    """Round 5: small swarms of the wide class (the UR5 launch script's M = 200: 13 tiles x 6 GPs on 256 CUs) run TWO workgroups per (tile, GP), one
    per half of the rows of Kinv (`FwdArgs.gsh_rs`, phases V and J over the member's own rows, the partial sums of phase F handed to the half that
    finishes the GP through `FwdArgs.rxch`).  Same states / inputs / Jacobians as one workgroup per (tile, GP) (`mcp_debug_set_row_split(0)`) up to
    the summation order over the training points, identical noise and dropout bits in Philox mode, bitwise reproducible; with recorded masks
    against the oracle at 1e-9 (states, inputs) and 1e-9 relative (gradients through the stored Jacobians).  SE + polynomial(1) and SE alone (both
    instantiations that carry the split).  Round 6: three row parts (two senders, the finishing part adds own + sender 0 + sender 1) and the
    row-part-major deal of the workgroups, each against the same one-workgroup form and the oracle."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops

    o = oracle_answer(key)
    w = hip_workload_on_oracle_operands(key)
    if mode == "masks":
        nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    else:
        nz = ops.NoiseSpec(seed=11, call=2)
    L = hipabi.lib()
    out = {}
    try:
        L.mcp_debug_set_cluster_map(cmap)
        for split in (1, 0, 1):
            L.mcp_debug_set_row_split(parts if split else 0)
            for q in w.params:
                q.grad = None
            with forced_variant(116) as fv:
                st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
                assert L.mcp_debug_last_gp_sharded() == 1, "the shape was expected to run GP-sharded"
                assert L.mcp_debug_last_row_split() == (parts if split else 0)
                c, _ = ops.expected_cost(w.cost, st)
                c.backward()
            assert int(status.item()) == 0
            res = (st.detach().clone(), inp.detach().clone(), [q.grad.clone() for q in w.params], float(c))
            if split in out:
                assert torch.equal(out[split][0], res[0]) and torch.equal(out[split][1], res[1])  # bitwise reproducible
                assert all(torch.equal(a, b) for a, b in zip(out[split][2], res[2]))
            out[split] = res
    finally:
        L.mcp_debug_set_row_split(-1)
        L.mcp_debug_set_cluster_map(-1)
    es = float((out[1][0] - out[0][0]).abs().max())
    eu = float((out[1][1] - out[0][1]).abs().max())
    eg = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(out[1][2], out[0][2]))
    print("row split (%d parts, deal %d) vs one workgroup per GP (%s, %s): states %.2e inputs %.2e grads rel %.2e" % (parts, cmap, key, mode, es, eu, eg))
    assert float((out[1][1][0] - out[0][1][0]).abs().max()) == 0.0  # the first step's inputs come before any GP
    assert es < 2e-9 and eu < 4e-9 and eg < 1e-8
    assert not torch.equal(out[1][1], torch.zeros_like(out[1][1]))
    if mode == "masks":
        assert float((out[1][0].cpu() - o["states"]).abs().max()) < 1e-9 and float((out[1][1].cpu() - o["inputs"]).abs().max()) < 2e-9
        assert abs(out[1][3] - o["cost"]) < 1e-11 * abs(o["cost"])
        for q, k in zip(out[1][2], ["log_ls", "centers", "weight"]):
            g = o["grads"][k]
            assert float((q.cpu().reshape(g.shape) - g).abs().max()) < 1e-9 * float(g.abs().max()), k


@pytest.mark.parametrize("name,N,M,T", [("ur5_script", 150, 40, 5), ("ur5_script", 448, 24, 4), ("ur5_se", 272, 200, 4), ("ur5_script", 400, 200, 3),
                                        ("ur5_script", 128, 17, 6)])
@pytest.mark.parametrize("parts,cmap", ROW_SPLIT_FORMS)
def test_row_split_cluster_block_shares(name, N, M, T, parts, cmap):
    """The row-split cluster over the block counts a training set can leave: Npad = 160 (5 blocks of 32 rows: 2 + 3), 448 (14: 7 + 7, the largest
    this class's k / v panels leave room for), 272 (8.5: 4 + 5 with a half-empty last block), 400 (12.5: 6 + 7, the launch script's 13 tiles with a ragged last one), 128
    (4: 2 + 2, one particle in the last tile).  On-device noise: the split and the one-workgroup form draw the same dropout bits and increments,
    so states, inputs and the gradients through the stored Jacobians agree to the summation order."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops, workloads

    w = workloads.build(name, device=dev(), M=M, T=T, N=N)
    assert w.model.gps[0].N == N
    torch.manual_seed(3)
    x0 = w.sample_x0()
    L = hipabi.lib()
    out = {}
    try:
        L.mcp_debug_set_cluster_map(cmap)
        for split in (1, 0):
            L.mcp_debug_set_row_split(parts if split else 0)
            for q in w.params:
                q.grad = None
            with forced_variant(116):
                st, inp, status = ops.rollout(w.model, w.policy, ops.NoiseSpec(seed=5, call=1), x0, w.T, w.p_drop)
                assert L.mcp_debug_last_gp_sharded() == 1 and L.mcp_debug_last_row_split() == (parts if split else 0)
                c, _ = ops.expected_cost(w.cost, st)
                c.backward()
            assert int(status.item()) == 0
            out[split] = (st.detach().clone(), inp.detach().clone(), [q.grad.clone() for q in w.params])
    finally:
        L.mcp_debug_set_row_split(-1)
        L.mcp_debug_set_cluster_map(-1)
    es = float((out[1][0] - out[0][0]).abs().max())
    eu = float((out[1][1] - out[0][1]).abs().max())
    eg = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(out[1][2], out[0][2]))
    print("row split vs one workgroup per GP (%s N=%d M=%d): states %.2e inputs %.2e grads rel %.2e" % (name, N, M, es, eu, eg))
    assert torch.equal(out[1][1][0], out[0][1][0])  # the first step's inputs come before any GP
    assert es < 2e-9 and eu < 4e-9 and eg < 1e-8
    assert float(out[1][1].abs().max()) > 0.0


@pytest.mark.parametrize("mode", ["masks", "philox"])
def test_eight_particles_per_backward_sweep_on_the_wide_class(mode):
    """Round 4: `rollout_bwd_kernel<24, 6, 512, 2, 8>` -- the UR5 class sweeps EIGHT particles per workgroup on large swarms (250 workgroups
    for C5's 2000 particles: one resident round instead of two).  With recorded masks the gradients are the oracle's (1e-9, as for the other
    widths); with Philox noise -- where the four lanes of a quad now draw twice per step and pass the words round -- they are those of the
    one-particle sweep on the same forward pass (a wrong keep bit anywhere changes them in the first digits)."""
    from gpu_helpers import dev, forced_variant
    from mc_pilco_amd import hipabi, ops

    o = oracle_answer("ur5_400")
    w = hip_workload_on_oracle_operands("ur5_400")
    if mode == "masks":
        nz = ops.NoiseSpec(eps=o["eps"].to(dev()).contiguous(), masks=o["masks"].to(torch.uint8).to(dev()).contiguous())
    else:
        nz = ops.NoiseSpec(seed=5, call=3)
    grads = {}
    for pb in (1, 8):
        for q in w.params:
            q.grad = None
        with forced_variant(16, bwd_particles=pb):
            st, inp, status = ops.rollout(w.model, w.policy, nz, o["x0"].to(dev()), w.T, o["p"])
            c, s = ops.expected_cost(w.cost, st)
            c.backward()
        assert int(status.item()) == 0
        grads[pb] = [q.grad.detach().cpu().clone() for q in w.params]
    for a, b in zip(grads[1], grads[8]):
        assert float((a - b).abs().max()) < 1e-11 * float(a.abs().max())
    if mode == "masks":
        for g8, k in zip(grads[8], ["log_ls", "centers", "weight"]):
            ref = o["grads"][k]
            assert float((g8.reshape(ref.shape) - ref).abs().max()) < 1e-9 * float(ref.abs().max()), k


# -------------------------------------------------------------------------------------------------------------------------
# configs[4] at its stated size
# -------------------------------------------------------------------------------------------------------------------------
def test_c5_full_size_properties():
    """UR5 shape, M=2000, T=300, N=400, 6 GPs, D=24 (BASELINE.json configs[4]) on the automatic dispatch: bitwise determinism,
    shard invariance (two half swarms with their global particle offsets reproduce the whole), status clean over all 300 steps."""
    from gpu_helpers import dev
    from mc_pilco_amd import hipabi, ops, workloads

    w = workloads.build("c5", device=dev())
    assert (w.M, w.T, w.model.gps[0].N, w.model.G, w.model.D) == (2000, 300, 400, 6, 24)
    torch.manual_seed(3)
    x0 = w.sample_x0()
    nz = lambda off=0: ops.NoiseSpec(seed=12, call=9, particle_offset=off)
    with torch.no_grad():
        a, ua, sa = ops.rollout(w.model, w.policy, nz(), x0, w.T, w.p_drop)
        assert hipabi.lib().mcp_debug_last_particles_per_wg() == 16
        b, ub, _ = ops.rollout(w.model, w.policy, nz(), x0, w.T, w.p_drop)
        assert int(sa.item()) == 0
        assert torch.equal(a, b) and torch.equal(ua, ub)
        assert bool(torch.isfinite(a).all())
        h = w.M // 2
        lo = ops.rollout(w.model, w.policy, nz(0), x0[:h].contiguous(), w.T, w.p_drop)[0]
        hi = ops.rollout(w.model, w.policy, nz(h), x0[h:].contiguous(), w.T, w.p_drop)[0]
        # (1000 particles may run with another GP split per workgroup than 2000: every GP's sums are formed by the same code
        #  in the same order whichever workgroup owns it, so the halves reproduce the whole bit for bit)
        assert torch.equal(torch.cat([lo, hi], 1), a)
        c, s = ops.expected_cost(w.cost, a)
        assert np.isfinite(float(c)) and np.isfinite(float(s))


def test_c5_adjoint_matches_finite_difference_at_full_width():
    """M=2000, N=400 on a 40-step horizon, where a central difference is accurate: directional derivative of the expected cost."""
    from gpu_helpers import dev
    from mc_pilco_amd import ops, workloads

    w = workloads.build("c5", device=dev(), T=40)
    torch.manual_seed(21)
    x0 = w.sample_x0()

    def cost_of():
        st, inp, status = ops.rollout(w.model, w.policy, ops.NoiseSpec(seed=77, call=5), x0, w.T, w.p_drop)
        return ops.expected_cost(w.cost, st)[0]

    for q in w.params:
        q.grad = None
    cost_of().backward()
    g = [q.grad.detach().clone() for q in w.params]
    gen = torch.Generator(device=dev())
    gen.manual_seed(5)
    dirs = [torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=gen) for q in w.params]
    gd = sum(float((a * b).sum()) for a, b in zip(g, dirs))
    eps = 1e-6
    with torch.no_grad():
        for q, d in zip(w.params, dirs):
            q.add_(eps * d)
        cp = float(cost_of())
        for q, d in zip(w.params, dirs):
            q.sub_(2 * eps * d)
        cm = float(cost_of())
    fd = (cp - cm) / (2 * eps)
    assert abs(fd - gd) < 1e-5 * max(abs(gd), 1e-3), (fd, gd)


# -------------------------------------------------------------------------------------------------------------------------
# the in-kernel Philox noise, statistically
# -------------------------------------------------------------------------------------------------------------------------
def _eps_of(model, pol, x0, seed, call, Tn=3):
    """Standard normals the kernel drew, recovered from the trajectories: eps = (delta - mu) / sigma with mu, sigma from the
    single-step posterior operator at each particle's own (x_t, u_t).  Returns [Tn-1, M, G]."""
    from mc_pilco_amd import ops

    with torch.no_grad():
        st, inp, status = ops.rollout(model, pol, ops.NoiseSpec(seed=seed, call=call), x0, Tn, 0.0)
        assert int(status.item()) == 0
        out = []
        for t in range(Tn - 1):
            x, u = st[t], inp[t]
            z = torch.cat([x[:, [0, 1, 3]], torch.sin(x[:, 2:3]), torch.cos(x[:, 2:3]), u], 1).contiguous()
            es = []
            for g, v in enumerate((1, 3)):
                mu, var = ops.posterior(model.gps[g], z)
                es.append(((st[t + 1][:, v] - x[:, v]) - mu.reshape(-1)) / torch.sqrt(var))
            out.append(torch.stack(es, 1))
    return torch.stack(out)


def test_philox_normals_are_standard_normal_and_independent():
    """>= 10^5 draws per stream: mean, variance, kurtosis and a Kolmogorov-Smirnov bound against N(0,1); no correlation across
    the GP index, neighbouring particles, time steps, `call`s and seeds."""
    from scipy import stats

    from conftest import load_golden
    from gpu_helpers import G, packed_model, packed_policy

    fx = load_golden("rollout_se")
    model = packed_model(fx, "se")
    pol = packed_policy(fx, "se", requires_grad=False)
    M = 65536
    x0 = G(0.05 * np.random.RandomState(0).randn(M, 4))
    e = _eps_of(model, pol, x0, seed=7, call=1).cpu().numpy()  # [2, M, 2]
    n = e.size
    assert n >= 2.5e5
    flat = e.reshape(-1)
    assert abs(flat.mean()) < 4.0 / np.sqrt(n)
    assert abs(flat.var() - 1.0) < 4.0 * np.sqrt(2.0 / n)
    assert abs(stats.kurtosis(flat, fisher=False) - 3.0) < 5.0 * np.sqrt(24.0 / n)
    assert abs(stats.skew(flat)) < 5.0 * np.sqrt(6.0 / n)
    assert stats.kstest(flat, "norm").statistic < 1.95 / np.sqrt(n)  # alpha = 0.001
    assert np.abs(flat).max() < 6.5  # Box-Muller on 52-bit uniforms reaches the tails but not absurdly
    for t in range(2):
        for g in range(2):
            col = e[t, :, g]
            assert stats.kstest(col, "norm").statistic < 1.95 / np.sqrt(col.size)

    def corr(a, b):
        return abs(float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]))

    lim = 4.5 / np.sqrt(M)
    assert corr(e[0, :, 0], e[0, :, 1]) < lim          # across GPs
    assert corr(e[0, :-1, 0], e[0, 1:, 0]) < lim       # neighbouring particles
    assert corr(e[0, :, 0], e[1, :, 0]) < lim          # across time steps
    e2 = _eps_of(model, pol, x0, seed=7, call=2).cpu().numpy()
    e3 = _eps_of(model, pol, x0, seed=8, call=1).cpu().numpy()
    assert corr(e[0], e2[0]) < lim and corr(e[0], e3[0]) < lim  # across calls and seeds
    assert not np.array_equal(e, e2)


def _keep_bits(p, M, Tn, seed, call, forced=0, B=200, offset=0):
    """Dropout keep decisions of the in-kernel generator for every (t, particle, basis), read back EXACTLY: all RBF centres sit
    far inside one huge lengthscale (phi == 1 to 1e-12), weights are powers of two (25 basis functions per input, 8 inputs = 200),
    no squashing -> u_k (1 - p) is the integer sum_j 2^j keep_j.  Returns bool [Tn, M, B] (B <= 200; ``offset``: the particle_offset)."""
    from gpu_helpers import G, dev, forced_variant, spec_from
    from mc_pilco_amd import ops

    S, U = 4, 8
    assert 176 <= B <= 200  # (every input has a basis function)
    Wm = np.zeros((U, B))
    for b in range(B):
        Wm[b // 25, b] = 2.0 ** (b % 25)
    pol = ops.PackedPolicy("plain", S, torch.log(G(np.full((1, S), 1e7))), G(np.zeros((B, S))), G(Wm), 1.0, False)
    D = S + U
    sp = spec_from(np.full(D, 1e3), 0.1)
    gp = ops.PackedGP(sp, G(np.zeros((16, D))), G(np.zeros(16)), G(1e-3 * np.eye(16)))
    model = ops.PackedModel([gp, gp], S, U, 0.05, [], list(range(S)), [1, 3], [0, 2])
    x0 = G(np.zeros((M, S)))
    with forced_variant(forced), torch.no_grad():
        st, inp, status = ops.rollout(model, pol, ops.NoiseSpec(seed=seed, call=call, particle_offset=offset), x0, Tn, p)
    assert int(status.item()) == 0
    v = (inp * (1.0 - p)).cpu().numpy()
    iv = np.rint(v).astype(np.int64)
    assert np.abs(v - iv).max() < 1e-3 and iv.min() >= 0 and iv.max() < 2 ** 25
    bits = ((iv[..., None] >> np.arange(25)) & 1).astype(bool)  # [Tn, M, U, 25]
    return bits.reshape(Tn, M, 200)[:, :, :B]


@pytest.mark.parametrize("p", [0.25, 0.1])
def test_philox_dropout_keep_rate_and_independence(p):
    """keep-rate = 1 - p overall, per basis function, per time step and per word of the 4-basis Philox block; no correlation
    between neighbouring basis functions (inside a block and across blocks), particles, steps and calls; and the 16-particle
    tile kernel and the backward-compatible variants draw the very same bits."""
    M, Tn = 4096, 4
    k = _keep_bits(p, M, Tn, seed=3, call=1)
    n = k.size
    q = 1.0 - p
    sd = np.sqrt(p * q)
    assert abs(k.mean() - q) < 4.0 * sd / np.sqrt(n)
    per_basis = k.reshape(-1, 200).mean(0)
    assert np.abs(per_basis - q).max() < 5.0 * sd / np.sqrt(M * Tn)
    per_step = k.reshape(Tn, -1).mean(1)
    assert np.abs(per_step - q).max() < 4.5 * sd / np.sqrt(M * 200)
    per_word = np.array([k[:, :, w::4].mean() for w in range(4)])
    assert np.abs(per_word - q).max() < 4.5 * sd / np.sqrt(n / 4)

    def corr(a, b):
        return abs(float(np.corrcoef(a.reshape(-1).astype(float), b.reshape(-1).astype(float))[0, 1]))

    lim = 4.5 / np.sqrt(M * Tn * 199)
    assert corr(k[:, :, :-1], k[:, :, 1:]) < lim                      # neighbouring basis functions (3 of 4 pairs share a block)
    assert corr(k[:, :, 3:-1:4], k[:, :, 4::4]) < 4.5 / np.sqrt(M * Tn * 49)  # across block boundaries only
    assert corr(k[:, :-1], k[:, 1:]) < 4.5 / np.sqrt((M - 1) * Tn * 200)      # neighbouring particles
    assert corr(k[:-1], k[1:]) < 4.5 / np.sqrt(M * (Tn - 1) * 200)            # consecutive steps
    k2 = _keep_bits(p, M, Tn, seed=3, call=2)
    assert corr(k, k2) < 4.5 / np.sqrt(n)
    for code in (1, 4, 16):
        assert np.array_equal(_keep_bits(p, 512, 2, seed=3, call=1, forced=code), k[:2, :512])
