"""CPU-only checks of the truth the GPU tests of the measured tanh-MLP loop compare with (tests/mlp_meas_models.mlp_meas_truth: the oracle's
step, tests/pd_meas_models.measure -- pinned to the reference by tests/test_pd_meas_cpu.py -- and tests/mlp_models.mlp_law composed under
autograd): the conditioning of every case of the table, autograd against central differences, the table's power to tell the measurement
formulas from their near misses, and the composition against tests/mlp_models.mlp_truth where the measurement changes nothing the policy reads.
Nothing here runs on a device."""
import functools

import pytest
import torch

import mlp_models as mm
from mlp_meas_models import CASES, case_id, case_inputs, loss_of, meas_model, truth_of
from pd_meas_models import pos_noise_for

DT = torch.float64


def relmax(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@functools.lru_cache(maxsize=None)
def _case(i):
    c, m, ins = case_inputs(CASES[i])
    return c, m, ins, truth_of(m, ins)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_every_case_is_well_conditioned(i):
    """What the parity bounds presuppose: positive variances, finite states of moderate size, and a gradient that is not zero in any tensor
    (a zero gradient would pass a relative bound on nothing)."""
    mode, shape, deg, N, T, M, hidden, variant, opt = CASES[i]
    c, m, ins, (st, inp, ym, grads, gx, vmin) = _case(i)
    gm = [float(g.abs().max()) for g in grads + [gx]]
    print("%s: min var %.3e |x| %.3e |u| %.3e gradient maxima %s" % (case_id(CASES[i]), vmin, float(st.abs().max()), float(inp.abs().max()),
                                                                    " ".join("%.2e" % g for g in gm)))
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(inp).all()) and bool(torch.isfinite(ym).all())
    assert float(st.abs().max()) < 20.0
    if T > 1:
        assert vmin > 0.0
    assert all(g > 0.0 for g in gm)
    assert torch.equal(ym[0], st[0])  # row 0 is measured true
    pos = ins["ms"]["pos"]
    if T > 1 and opt.get("std", 0.1):
        assert float((ym[1:, :, pos] - st[1:, :, pos]).abs().min()) > 0.0  # a measurement was simulated


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_autograd_against_central_differences(i):
    """Step 1e-6, bound 1e-5 relative with floor 1e-3 (tests/test_pd_meas_cpu.py); the first and the last entry of every parameter tensor
    and of x0."""
    c, m, ins, (_, _, _, grads, gx, _) = _case(i)
    h = 1e-6
    for k, q in enumerate(ins["params"] + [ins["x0"]]):
        g = (grads + [gx])[k].reshape(-1)
        for e in sorted({0, q.numel() - 1}):
            def moved(d):
                t = [p.clone() for p in ins["params"] + [ins["x0"]]]
                t[k].reshape(-1)[e] += d
                return loss_of(m, ins, params=t[:-1], x0=t[-1])
            fd = (moved(h) - moved(-h)) / (2 * h)
            print("%s tensor %d entry %d: fd %.9e autograd %.9e" % (case_id(CASES[i]), k, e, fd, float(g[e])))
            assert abs(fd - float(g[e])) < 1e-5 * max(abs(float(g[e])), 1e-3)


SENSITIVE = [i for i, c in enumerate(CASES) if c[4] == 12 and c[5] <= 5 and c[7] == "all" and not c[8] and c[6] != (64, 64)]


def test_the_table_tells_the_measurement_from_its_near_misses():
    """On the truth alone: a dropped b1 term, a dropped -a1 term, swapped columns of the position noise and row 0 treated like the other
    rows each move the states or the gradients of the T = 12 cases with every joint measured by more than 1e-6, 1000 x the parity bound."""
    assert len(SENSITIVE) >= 2
    smallest = float("inf")
    for defect in ("no_b1", "no_a1", "swap_columns", "row0_filtered"):
        for i in SENSITIVE:
            c, m, ins, (st, inp, ym, grads, gx, _) = _case(i)
            dst, dinp, dym, dgrads, dgx, _ = truth_of(m, ins, defect=defect)
            move = max(float((dst - st).abs().max()), max(relmax(a, b) for a, b in zip(dgrads + [dgx], grads + [gx])))
            print("%s on %s: states %.3e, largest gradient move %.3e" % (defect, case_id(CASES[i]), float((dst - st).abs().max()),
                                                                        max(relmax(a, b) for a, b in zip(dgrads + [dgx], grads + [gx]))))
            assert move > 1e-6, (defect, case_id(CASES[i]))
            smallest = min(smallest, move)
    print("smallest move: %.3e" % smallest)


def test_a_measurement_that_changes_nothing_the_policy_reads_is_the_unmeasured_truth():
    """std = 0, b = [1, 0], a = [1, 0], a policy on the positions alone (arm2: the angles): the measured positions are the true ones, the
    measured velocities are read by nobody, and the composed truth is tests/mlp_models.mlp_truth."""
    shape, N, deg, T, M, hidden = "arm2", 37, 1, 12, 5, (7, 3)
    c, m, _ = mm.build_pair(shape, N, deg, seed=mm.PAIR_SEED)
    seed = T * 100 + M
    x0, _, _, _, eps, w, wu = mm.inputs_for(c, M, T, seed=seed)
    angle, non_angle = [0, 1], []
    params = mm.network(c, hidden, angle, non_angle, seed)
    ms = dict(meas_model(shape, "all", 0.0), b=[1.0, 0.0], a=[1.0, 0.0])
    ins = dict(x0=x0, eps=eps, w=w, wu=wu, params=params, angle=angle, non_angle=non_angle, u_max=1.0, squash=True, ms=ms,
               pos_noise=pos_noise_for(T, M, 2, seed), var_scale=None, sample=True, shape=shape)
    st, inp, ym, grads, gx, vmin = truth_of(m, ins)
    torch.set_num_threads(1)
    ost, oin, ograds, ogx, ovmin = mm.mlp_truth(shape, m, x0, params, eps, w, wu, True, angle, non_angle)
    assert torch.equal(st, ost) and torch.equal(inp, oin) and vmin == ovmin
    assert torch.equal(ym[:, :, :2], st[:, :, :2]) and float((ym[1:, :, 2:] - st[1:, :, 2:]).abs().max()) > 0  # the velocities ARE measured differently
    eg = [relmax(a, b) for a, b in zip(grads + [gx], ograds + [ogx])]
    print("measured vs unmeasured truth, gradients: %s" % " ".join("%.3e" % e for e in eg))
    assert max(eg) < 1e-13 and all(float(g.abs().max()) > 0 for g in grads)
