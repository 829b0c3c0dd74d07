"""GPU: the in-kernel Philox noise against an independent truth on every form.  tests/noise_truth.py restates on the CPU what the kernels are
documented to draw (csrc/mcp_device.h:207-274, the mcp_noise comment of include/mcpilco_hip.h); tests/noise_truth_cases.py names the (seed, call,
particle offset) of every launch here and feeds the tables to the oracle; tests/test_noise_truth_cpu.py shows that each wrong generator of
``noise_truth.MUTANTS`` changes those tables and that every case meets its conditions on the oracle alone.  Every launch here is in Philox mode:
NoiseSpec(seed, call, particle_offset) and no buffers.

  a. last bit    A read-off model (x0 = 0, alpha = 0, Kinv = 0, lambda = 1: mean 0, variance kzz = 1, so the sampled velocity IS the device's normal)
                 through mcp_model_step at t = 0, 255, 256, 2^22 - 1 (M = 65536, G = 2: 2^19 draws, RARE_PARTICLE among them) and through one T = 2
                 rollout form of every kernel family, against the truth at a 64-bit significand, in ulps of the truth.
                 MEASURED on an MI355X: 2.319 ulp at the most over the 524288 draws of the steps (LASTBIT_MEASURED), 2.045 ulp over each rollout
                 form's draws, the same draw in every family; asserted: ULP_BOUND = twice the largest, rounded up to a power of two = 8.  Above
                 ULP_CEILING = 64 the device would not be evaluating the formula in double precision.  (numpy's own double evaluation of the
                 formula sits at 2.8 ulp of the same truth: tests/test_noise_truth_cpu.py.)
  b. keep bits   decoded exactly by the constructions of tests/test_gpu_realsize.py (_keep_bits) and tests/test_gpu_mlp_drop.py (decode_keep_bits),
                 equal to noise_truth.keep: p in {0.25 (threshold 2^30), 0.1, and a p whose threshold IS a drawn word}, forced 0 / 1 / 4 / 16,
                 B = 200 and 197, M = 37 (ragged tiles), the MLP's hidden shapes (16,) and (7, 16) (a block across both layers).
  c. parity, every forward form of status_models.FORMS against the oracle's rollout fed the truth's eps, masks and position noise: 1e-9 on states
                 and inputs, 2e-9 / Ts on the measured states, status 0, report == plan.
  d. parity, backward: one case per sweep instantiation (noise_truth_cases.SWEEPS) with p_drop = 0.25 against the oracle's autograd on the truth's
                 tables at the width-class bounds (cost 1e-11, gradients 1e-8 relative): the sweep's recomputed keep bits are the truth's.
  e. the other families: open loop (ragged lengths; plain and recording), PD and PD measured, the tanh MLP plain / measured / dropout / tracking
                 (measured and not), and a chain of mcp_model_step calls, forward and gradients, against their own truth functions on the tables.
  f. addressing edges on one cheap form: call = 2^32 - 1, 2^32, 2^40 + 3; seeds with a high word; call_dev carrying into the key; one total call
                 split differently; particle_offset 7, 2^32 - 2, 2^32 + 5, 2^40 - 5; two shards against the whole launch bit for bit.
  g. the class path: MC_PILCO.apply_policy twice in "philox" mode under the tanh-MLP policy with dropout, rollout k against the oracle on the
                 class's own X / alpha / Kinv fed the truth's tables at call = k.

Largest errors measured on an MI355X against the truth-fed oracle (each printed by its test; the bounds are the buffer launches' own):
  c. 90 forms: states 1.6e-14, inputs 1.5e-14, measured states 6.7e-15 (bounds 1e-9, 1e-9, 4e-8)
  d. 13 sweeps: states 1.8e-15, inputs 3.2e-15, cost 2.7e-16 relative, gradients 3.9e-15 relative (1e-9, 1e-9, 1e-11, 1e-8)
  e. open loop / step chain: states 9.4e-14, gradients 1.4e-13; PD and MLP families: states 1.1e-14, inputs 3.0e-15, measured 2.4e-15, gradients
     9.1e-15 (1e-9, 2e-9, 1e-9, 1e-9)
  f. 13 edges: states 1.8e-15, inputs 4.0e-15, measured 2.3e-15; shards and differently split calls bit for bit
  g. states 1.2e-12, inputs 8.5e-13 (1e-9, 2e-9)
  b. every decoded keep bit equal (28 launches, 3 x 37 x 200 or 197 bits each; the MLP's 3 x 37 x 16).
No launch disagreed with the truth: no defect of the generator or its addressing was found."""
import dataclasses

import numpy as np
import pytest
import torch

import noise_truth as nt
import noise_truth_cases as ntc
import status_models as sm
import width_models as wm
from forced_launch import against, launch

pytestmark = pytest.mark.gpu

BOUND, BOUND_MEAS = 1e-9, 2 * 1e-9 / wm.TS
ULP_CEILING = 64.0
LASTBIT_MEASURED = 2.319  # largest |device - truth| in ulps of the truth, tier a
ULP_BOUND = ULP_CEILING if LASTBIT_MEASURED is None else 2.0 ** np.ceil(np.log2(2.0 * LASTBIT_MEASURED))


def _nz(spec, **kw):
    from mc_pilco_amd import ops

    dev_word = None
    if spec.dev:
        dev_word = torch.tensor([spec.dev], dtype=torch.int64, device="cuda")
    return ops.NoiseSpec(seed=spec.seed, call=spec.call, particle_offset=spec.offset, call_dev=dev_word, **kw)


# ---- a. last bit ----------------------------------------------------------------------------------------------------------------------------------
def _readoff(shape="arm2"):
    """(cfg, PackedModel, sigma): arm2's layout (S 4, U 2, G 2, D 8) -- or the cart-pole's (S 4, U 1, G 2, D 6: the shape the lean kernel takes) --
    with 32 training rows, alpha = 0 and Kinv = 0; sigma = sqrt(kzz) from the oracle's kernel."""
    import open_grad_models
    import pd_models
    from gpu_helpers import G, spec_from
    from helpers import hyper
    from mc_pilco_amd import ops
    from oracle import mcpilco_oracle as orc

    c = pd_models.SHAPES["arm2"] if shape == "arm2" else open_grad_models.SHAPES["speed"]
    D = len(c["not_angle"]) + 2 * len(c["angle"]) + c["U"]
    gp = ops.PackedGP(spec_from(np.ones(D), 0.1), G(np.zeros((32, D))), G(np.zeros(32)), G(np.zeros((32, 32))))
    pm = ops.PackedModel([gp, gp], c["S"], c["U"], c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    z = orc.gp_features(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, c["U"], dtype=torch.float64), c["angle"], c["not_angle"])
    sigma = float(torch.sqrt(orc.gp_diag(hyper(np.ones(D), 0.1, 1.0, None), z))[0])
    assert sigma == 1.0  # (so that the increment sigma * eps is eps to the bit)
    return c, pm, sigma


def _ulps(name, got, spec):
    want = spec.tables(hp=True)["eps"][0]
    u = nt.ulps(got, want)
    i = np.unravel_index(int(np.argmax(u)), u.shape)
    print("%s: %d draws, largest error %.3f ulp at particle %d GP %d (truth %.17g); |normal| up to %.3f" % (
        name, u.size, u.max(), spec.offset + i[0], i[1], float(want[i]), np.abs(got).max()))
    return float(u.max())


@pytest.mark.skipif(not nt.have_longdouble(), reason="np.longdouble is a double here")
def test_last_bit_of_the_normal_through_model_step():
    from gpu_helpers import G
    from mc_pilco_amd import ops

    c, pm, _ = _readoff()
    M = ntc.LASTBIT_M
    x, u = G(np.zeros((M, 4))), G(np.zeros((M, 2)))
    worst, n = 0.0, 0
    for t in ntc.LASTBIT_STEPS:
        spec = ntc.lastbit_step_spec(t)
        with torch.no_grad():
            nx, status = ops.model_step(pm, x, u, t, noise=_nz(spec), particle_pred=True)
        assert int(status.item()) == 0
        got = nx[:, c["vel"]].cpu().numpy()
        worst, n = max(worst, _ulps("model_step t = %d" % t, got, spec)), n + got.size
        if t == 0:  # the draw that tells 32-bit uniforms apart
            i = ntc.RARE_PARTICLE - spec.offset
            assert abs(got[i, 0] - spec.tables()["eps"][0, i, 0]) < 1e-12 and got[i, 0] > 6.19
    assert n >= 2 ** 18
    print("last-bit tier, model_step: %.3f ulp at the most over %d draws (asserted %.0f)" % (worst, n, ULP_BOUND))
    assert worst <= ULP_CEILING, "the device is not evaluating Box-Muller in double precision"
    assert worst <= ULP_BOUND


ROLLOUT_FAMILIES = ["small-4", "small-sharded-104", "lean-204", "tile-16", "open", "pd", "mlp"]


@pytest.mark.skipif(not nt.have_longdouble(), reason="np.longdouble is a double here")
@pytest.mark.parametrize("fam", ROLLOUT_FAMILIES)
def test_last_bit_of_the_normal_through_a_rollout_of_every_family(fam):
    import closed_loop_family as clf
    import mlp_models
    import pd_models
    from gpu_helpers import G, forced_variant
    from mc_pilco_amd import hipabi, ops

    c, pm, _ = _readoff("arm2" if fam in ("open", "pd", "mlp") else "cartpole")
    spec = ntc.lastbit_rollout_spec(sharded="sharded" in fam or "lean" in fam)
    M = spec.M
    x0 = G(np.zeros((M, 4)))
    with torch.no_grad():
        if fam == "open":
            st, status = ops.rollout_open(pm, x0, G(np.zeros((1, M, 2))), noise=_nz(spec), particle_pred=True)
        elif fam == "pd":
            _, kp, kd, target, _, _, _ = pd_models.inputs_for(c, 1, 2, seed=1)
            st, _, status = ops.rollout_pd(pm, clf.controller(c, kp, kd, target, trainable=False).packed(), _nz(spec), x0, 2)
        elif fam == "mlp":
            pol = clf.policy(c, mlp_models.network(c, (5,), c["angle"], c["not_angle"], 1), (5,), trainable=False)
            st, _, status = ops.rollout_mlp(pm, pol.packed(), _nz(spec), x0, 2)
        else:
            code = int(fam.rsplit("-", 1)[1])
            rs = np.random.RandomState(0)
            pol = ops.PackedPolicy("angles", 4, torch.log(G(np.ones((1, 5)))), G(rs.randn(8, 5)), G(rs.randn(1, 8)), 1.0, True, angle=[2], non_angle=[0, 1, 3])
            with forced_variant(code):
                st, _, status = ops.rollout(pm, pol, _nz(spec), x0, 2, 0.0)
                d = hipabi.DISPATCH
                print("forced %d ran: particles %d GP-sharded %d lean %d" % (code, d.ran_particles, d.ran_gp_sharded, d.ran_fwd_lean))
                assert d.ran_particles == code % 100 and bool(d.ran_gp_sharded) == (code >= 100) and bool(d.ran_fwd_lean) == (code >= 200)
    assert int(status.item()) == 0
    worst = _ulps("rollout " + fam, st[1][:, c["vel"]].cpu().numpy(), spec)
    assert worst <= ULP_CEILING and worst <= ULP_BOUND


# ---- b. keep bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", ntc.KEEP_CODES)
@pytest.mark.parametrize("B", ntc.KEEP_BS)
@pytest.mark.parametrize("p", ntc.KEEP_PS, ids=["p0.25", "p0.1", "p-on-a-word"])
def test_keep_bits_of_the_rbf_policy_are_the_truths(p, B, code):
    from test_gpu_realsize import _keep_bits

    spec = ntc.keep_spec(p, B)
    got = _keep_bits(p, spec.M, spec.T, spec.seed, spec.call, forced=code, B=B)
    want = spec.tables()["masks"]
    print("p %.6f B %d forced %d: %d bits, keep rate %.4f, %d differ" % (p, B, code, want.size, want.mean(), int((got != want).sum())))
    assert got.shape == want.shape and np.array_equal(got, want)
    if p == ntc.KEEP_PS[2]:  # the word equal to the threshold is kept
        assert bool(got[0, 0, ntc.p_on_a_drawn_word()[1]])


@pytest.mark.parametrize("hidden", ntc.MLP_HIDDEN, ids=lambda h: "h" + "x".join(str(v) for v in h))
@pytest.mark.parametrize("p", ntc.KEEP_PS[:2])
def test_keep_bits_of_the_mlp_are_the_truths(p, hidden):
    """The last layer's 16 units: units 0 .. 15 of a one-layer network, units 7 .. 22 behind a layer of 7 (the block of units 4 .. 7 spans both)."""
    from test_gpu_mlp_drop import decode_keep_bits, pair

    c, m, pm = pair("arm2", 37, 1)
    spec = ntc.keep_spec(p, sum(hidden), ntc.MLP_KEEP_M, ntc.MLP_KEEP_T, ntc.MLP_KEEP_OFFSET)
    got = decode_keep_bits(pm, c, hidden, _nz(spec), p, spec.M, spec.T)
    want = spec.tables()["masks"][:, :, -16:]
    print("MLP %s p %.2f: %d bits, keep rate %.4f, %d differ" % (hidden, p, want.size, want.mean(), int((got.astype(bool) != want).sum())))
    assert np.array_equal(got.astype(bool), want)


# ---- c. parity, every forward form ------------------------------------------------------------------------------------------------------------------
def _forward_against_truth(form, c, spec, tr, out, x0=None):
    op = ntc.operands(c, spec, x0)
    st, inp, mbuf, word, rep, fp = launch(form, c, sm.packed_op(c, op, philox=_nz(spec)), True)
    if rep != (fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, fp.ran_row_split):
        out.append("the report %s is not the plan's %s" % (rep, (fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, fp.ran_row_split)))
    got = sm.plan_words(fp)
    if form.want is not None and not sm.matches(form.want, got):
        out.append("the table pins %s, the plan of this call says %s" % (form.want, got))
    if word != 0:
        out.append("status word %d" % word)
    es, eu, em = float("nan"), float("nan"), float("nan")
    if tr is not None:
        es, eu = against("states", st, tr.states, BOUND, out), against("inputs", inp, tr.inputs, BOUND, out)
        if c.pms is not None and not form.no_grad:
            if mbuf is None:
                out.append("no measured states were left by the call")
            else:
                em = against("measured", mbuf, tr.meas, BOUND_MEAS, out)
    return st, inp, mbuf, (es, eu, em), rep


@pytest.mark.parametrize("form", sm.FORMS, ids=lambda f: f.id)
def test_every_forward_form_against_the_truth_fed_oracle(form):
    c = sm.case(form.case)
    spec = ntc.spec_of(c, form.M)
    tr = ntc.truth_spec(c, spec)
    assert tr.word == 0
    out = []
    _, _, _, errs, rep = _forward_against_truth(form, c, spec, tr, out)
    print("%s (seed %#x call %d): ran %s | errs states %.2e inputs %.2e measured %.2e" % ((form.id, spec.seed, spec.call, rep) + errs))
    assert not out, "\n".join(out)


# ---- d. parity, backward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", ntc.SWEEPS, ids=lambda s: "%s-f%d-b%s%s-M%d" % (s[0], s[1], "a" if s[2] is None else s[2], "" if s[3] is None else "-pipe%d" % s[3], s[4]))
def test_backward_sweeps_against_the_oracles_autograd_on_the_truths_tables(sw):
    from test_gpu_width_classes import _abserr, _relerr, _run

    name, code, pb, pipe, M = sw
    c = wm.BY_NAME[name]
    if pb is not None:
        assert pb in wm.sweep_widths(c), (pb, wm.sweep_widths(c))
    spec = ntc.spec_of(c, M)
    ost, oin, oc, og = ntc.oracle_grad(c, M)
    st, inp, cst, pol, x0, rep = _run(c, code, pb, pipe, M, True, philox=_nz(spec))
    if code == 204:
        assert rep["fwd_lean"] == 1 and rep["bwd_lean"] == 1
    else:
        assert rep["bwd_lean"] == 0
    if pipe is not None:
        assert rep["bwd_pipe"] == pipe
    errs = [_abserr(st, ost), _abserr(inp, oin), abs(float(cst.detach()) - oc) / abs(oc), _relerr(pol.log_ls.grad, og[0]), _relerr(pol.centers.grad, og[1]),
            _relerr(pol.weight.grad, og[2])] + ([_relerr(pol.bias.grad, og[3])] if c.bias else []) + [_relerr(x0.grad, og[4])]
    print("%s forced %d sweep %s pipe %s M %d: ran %s | errs states, inputs (abs), cost, gradients (rel): %s" % (
        name, code, pb, pipe, M, rep, " ".join("%.2e" % e for e in errs)))
    assert all(float(np.abs(g).max()) > 0.0 for g in og[:3])
    assert errs[0] < 1e-9 and errs[1] < 1e-9 and errs[2] < 1e-11 and max(errs[3:]) < 1e-8


# ---- e. the other families ----------------------------------------------------------------------------------------------------------------------------
STATE_TOL, INPUT_TOL, GRAD_TOL = 1e-9, 2e-9, 1e-9  # (tests/test_gpu_pd_rollout.py, tests/test_gpu_mlp_rollout.py and their measured / dropout / tracking kin)


@pytest.mark.parametrize("fam", ["open", "step_chain"])
def test_open_loop_forms_against_their_truth(fam):
    """mcp_rollout_open (no record) and its recording form with ragged lengths; a chain of mcp_model_step calls at t = 0 .. T - 2 (autograd through
    the chain): states, dL/dx0 and dL/du (tests/test_gpu_open_rollout_grad.py: 1e-9 absolute, 1e-9 relative)."""
    import closed_loop_family as clf
    from gpu_helpers import G, relmax
    from mc_pilco_amd import ops

    c, ins, (ost, ogx, ogu, vmin) = ntc.family_truth(fam)
    _, _, pm = clf.open_pair("speed", ntc.FAM_N, ntc.FAM_DEG)
    spec = ntc.family_spec(fam)
    x0, u, w = G(ins["x0"]).requires_grad_(True), G(ins["u"]).requires_grad_(True), G(ins["w"])
    if fam == "open":
        plain, status0 = ops.rollout_open(pm, x0.detach(), u.detach(), lengths=ins["lengths"], noise=_nz(spec), particle_pred=True)
        st, status = ops.rollout_open_diff(pm, x0, u, lengths=ins["lengths"], noise=_nz(spec), particle_pred=True)
        assert int(status0.item()) == 0 and torch.equal(plain, st.detach())
    else:
        status = torch.zeros(1, dtype=torch.int32, device=x0.device)
        xs = [x0]
        for t in range(ntc.FAM_T - 1):
            xs.append(ops.model_step(pm, xs[-1], u[t], t, noise=_nz(spec), particle_pred=True, status=status)[0])
        st = torch.stack(xs)
    (w * st).sum().backward()
    assert int(status.item()) == 0
    errs = (float((st.detach().cpu() - ost).abs().max()), relmax(x0.grad, ogx), relmax(u.grad, ogu))
    print("%s (seed %#x call %d offset %d): states %.3e g_x0 %.3e g_u %.3e (min var %.3e)" % ((fam, spec.seed, spec.call, spec.offset) + errs + (vmin,)))
    assert errs[0] < STATE_TOL and errs[1] < GRAD_TOL and errs[2] < GRAD_TOL


@pytest.mark.parametrize("fam", [f for f in ntc.FAMILIES if f not in ("open", "step_chain")])
def test_closed_loop_families_against_their_truth(fam):
    """mcp_rollout_pd / _pd_meas, mcp_rollout_mlp / _mlp_meas / _mlp_drop / _mlp_track (measured and not), recording launch and sweep, through
    tests/closed_loop_family.py against the family's truth function fed the truth's tables."""
    import closed_loop_family as clf

    c, ins, truth = ntc.family_truth(fam)
    spec = ntc.family_spec(fam)
    ms = clf.meas_spec(ins["ms"])  # (no position noise buffer: Philox)
    if fam.startswith("pd"):
        family, tr = clf.PD, clf.pd_truth_of(truth)
        _, _, pm = clf.PD.pair(ntc.FAM_SHAPE, ntc.FAM_N, ntc.FAM_DEG, measured=ms is not None)
        pol, p = clf.controller(c, ins["kp"], ins["kd"], ins["target"]), None
    else:
        family, tr = clf.MLP, clf.mlp_truth_of(truth)
        _, _, pm = clf.MLP.pair(ntc.FAM_SHAPE, ntc.FAM_N, ntc.FAM_DEG, measured=True)
        p = ntc.FAM_P if ins["masks"] is not None else None
        if "track" in fam:
            from test_gpu_mlp_track import policy as track_policy

            pol = track_policy(c, ins["params"], ntc.FAM_HIDDEN, ins["target"], ins["idx"], ins["angle"], ins["non_angle"], flg_drop=True)
        else:
            pol = clf.policy(c, ins["params"], ntc.FAM_HIDDEN, ins["angle"], ins["non_angle"])
    got = family.run(pm, pol, ins["x0"], ntc.FAM_T, _nz(spec), ins["w"], ins["wu"], True, meas=ms, p_drop=p)
    clf.check_against(family, "%s (seed %#x call %d offset %d)" % (fam, spec.seed, spec.call, spec.offset), tr, got, (STATE_TOL, INPUT_TOL, GRAD_TOL))


# ---- f. addressing edges --------------------------------------------------------------------------------------------------------------------------
EDGE_FORM = next(f for f in sm.FORMS if f.case == ntc.EDGE_CASE and f.M == ntc.EDGE_M and f.code == 4 and not f.no_grad)
_EDGE_RUNS = {}


def _edge_run(name):
    """(states, inputs, measured) of the edge's launch, compared with its truth: once per process."""
    if name not in _EDGE_RUNS:
        c, spec = sm.case(ntc.EDGE_CASE), ntc.edge_spec(name)
        out = []
        st, inp, mbuf, errs, rep = _forward_against_truth(EDGE_FORM, c, spec, ntc.truth_spec(c, spec), out)
        print("edge %s (seed %#x call %d + device %d offset %d): errs states %.2e inputs %.2e measured %.2e" % (
            (name, spec.seed, spec.call, spec.dev, spec.offset) + errs))
        assert not out, "\n".join(out)
        _EDGE_RUNS[name] = (st, inp, mbuf)
    return _EDGE_RUNS[name]


@pytest.mark.parametrize("name", list(ntc.EDGES))
def test_addressing_edges_against_the_truth_fed_oracle(name):
    _edge_run(name)


@pytest.mark.parametrize("a,b", ntc.SAME_BITS)
def test_one_total_call_draws_the_same_bits_however_it_is_split(a, b):
    assert all(np.array_equal(p, q) for p, q in zip(_edge_run(a), _edge_run(b)))
    assert not np.array_equal(_edge_run("call-2^32")[0], _edge_run("call-2^32-1")[0])


@pytest.mark.parametrize("name", ["offset-2^32-2", "offset-7"])
def test_two_shards_carry_the_rows_of_the_whole_launch(name):
    """Rows [0, 3) and [3, 5) launched on their own with particle_offset advanced by 3: the whole launch's rows bit for bit (the first shard ends
    on the last particle id below 2^32), and the truth's at 1e-9."""
    c, spec = sm.case(ntc.EDGE_CASE), ntc.edge_spec(name)
    whole, tr = _edge_run(name), ntc.truth_spec(c, spec)
    x0 = wm.noise(c, spec.M)[0]
    for lo, hi in ((0, 3), (3, 5)):
        part = dataclasses.replace(spec, name="%s[%d:%d]" % (spec.name, lo, hi), M=hi - lo, offset=spec.offset + lo)
        out = []
        st, inp, mbuf, _, _ = _forward_against_truth(dataclasses.replace(EDGE_FORM, M=hi - lo), c, part, None, out, x0=x0[lo:hi])
        assert not out, "\n".join(out)
        for got, full, want in zip((st, inp, mbuf), whole, (tr.states, tr.inputs, tr.meas)):
            assert np.array_equal(got, full[:, lo:hi])
            assert float(np.abs(got - want[:, lo:hi]).max()) < (BOUND_MEAS if want is tr.meas else BOUND)


# ---- g. the class path ------------------------------------------------------------------------------------------------------------------------------
def test_class_path_rollout_k_is_the_truth_fed_oracles_at_call_k():
    """MC_PILCO.apply_policy twice with noise_mode = "philox" and seed = s under the tanh-MLP policy with dropout (the arm2 object of
    tests/closed_loop_family.py): rollout k is the oracle's on the class's own X / alpha / Kinv, fed the truth's eps and masks at call = k, the
    counter ``_rollout_noise`` advances; the two rollouts differ."""
    import closed_loop_family as clf
    import mlp_drop_models as mdm
    import mlp_models
    from helpers import hyper
    from oracle import mcpilco_oracle as orc
    from test_gpu_mlp_drop import _object

    M, T, hidden, p, seed = 16, 4, (7, 3), 0.25, (ntc.SEED_HI << 32) | 21
    c = mlp_models.SHAPES["arm2"]
    net = mlp_models.network(c, hidden, c["angle"], c["not_angle"], 40)
    obj = _object("MC_PILCO", net, hidden, M)
    obj.noise_mode, obj.seed = "philox", seed
    ml = obj.model_learning
    h = hyper(np.ones(8) * 2.0, 0.05, 1.0, None)  # (clf.arm_object: pretrained at its initial hyper-parameters)
    caches = [orc.GPCache(ml.gp_inputs_tr_list[g].cpu(), ml.alpha_list[g].cpu().reshape(-1, 1), ml.K_X_inv_list[g].cpu(), ml.m_X_list[g].cpu()) for g in range(2)]
    m = orc.SpeedModel([h, h], caches, c["Ts"], c["angle"], c["not_angle"], c["vel"], c["not_vel"])
    seen = []
    for k in (1, 2):
        torch.manual_seed(5)
        with torch.no_grad():
            st, inp = obj.apply_policy(p_dropout=p, **clf.sim_args(M, T))
        assert obj.last_feedback_fused is True and int(obj.last_status.item()) == 0 and obj._rollout_calls == k
        spec = ntc.Spec("class-path-%d" % k, seed, k, T, M, G=2, B=sum(hidden), p=p)
        eps, masks, _ = ntc.torch_tables(spec)
        w = torch.zeros(T, M, 4, dtype=torch.float64)
        tr = mdm.drop_truth("arm2", m, st[0].cpu(), net, eps, w, None, True, c["angle"], c["not_angle"], masks.to(torch.uint8), p, u_max=1.5)
        es, ei = float((st.cpu() - tr[0]).abs().max()), float((inp.cpu() - tr[1]).abs().max())
        print("class path, rollout %d (seed %#x call %d): states %.3e inputs %.3e (min var %.3e)" % (k, seed, k, es, ei, tr[-1]))
        assert tr[-1] > sm.MARGIN and es < STATE_TOL and ei < INPUT_TOL  # (kzz = lambda = 1: the margin is 1e-3 kzz)
        seen.append(st)
    assert torch.equal(seen[0][0], seen[1][0]) and float((seen[0] - seen[1]).abs().max()) > 1e-3
