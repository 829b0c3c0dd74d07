"""CPU: what the seven entry points of the open-loop / PD rollout family refuse, and with which code (mcp_rollout_open, _open_rec, _open_bwd,
mcp_rollout_pd, _pd_bwd, _pd_meas, _pd_meas_bwd).  A refused call returns before any HIP call, so the library answers without a GPU (as
tests/test_abi_cpu.py::test_argument_validation_without_gpu relies on); the device pointers are dummy non-NULL addresses that nothing reads.

Every expected code is written out: 0 MCP_OK, -1 MCP_ERR_ARG, -2 MCP_ERR_LIMIT.  Order of the checks in every entry: NULL pointers and
M / T / Mu (-1), the compiled limits (-2), the model (-1), the PD descriptor (U over MCP_MAX_INPUT -2, everything else -1), the measurement
(-1), then -- the sweeps only -- "nothing asked for" (0, no launch).  NOTHING here passes validation with something asked for: without a
device that would be a launch attempt.  The forward entries launch whenever they accept, so every forward call below is a refusal; the
sweeps are always called with no gradient asked for, which is also the case "a bad model is refused even when nothing is asked for"."""
import ctypes as C

import pytest

PTR = 0x1000  # stands for device memory: never dereferenced by a refused call
M, T = 5, 3
FWD = ("open", "open_rec", "pd", "pd_meas")
BWD = ("open_bwd", "pd_bwd", "pd_meas_bwd")
OPEN = ("open", "open_rec", "open_bwd")
PD = ("pd", "pd_meas", "pd_bwd", "pd_meas_bwd")
MEAS = ("pd_meas", "pd_meas_bwd")
ALL = FWD + BWD

# argument names of each entry, in call order (descriptors are passed by reference, "stream" is always NULL)
SIGS = {
    "open": ("model", "noise", "M", "T", "particle_pred", "x0", "u", "Mu", "lengths", "states", "mu", "var", "status"),
    "open_rec": ("model", "noise", "M", "T", "particle_pred", "x0", "u", "Mu", "lengths", "states", "mu", "var", "jac", "status"),
    "open_bwd": ("model", "M", "T", "states", "lengths", "jac", "g_states", "g_x0", "g_u"),
    "pd": ("model", "pd", "noise", "M", "T", "particle_pred", "x0", "states", "inputs", "jac", "mu", "var", "status"),
    "pd_meas": ("model", "pd", "meas", "noise", "M", "T", "particle_pred", "x0", "states", "inputs", "jac", "mu", "var", "status"),
    "pd_bwd": ("model", "pd", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_gains", "g_x0"),
    "pd_meas_bwd": ("model", "pd", "meas", "M", "T", "states", "inputs", "jac", "g_states", "g_inputs", "g_gains", "g_x0"),
}
# what an entry refuses to find NULL (jac: the recording form and the sweeps; the plain forward calls take jac = NULL as "no record")
REQUIRED = {
    "open": ("model", "noise", "x0", "u", "states", "status"),
    "open_rec": ("model", "noise", "x0", "u", "states", "status", "jac"),
    "open_bwd": ("model", "states", "jac", "g_states"),
    "pd": ("model", "pd", "noise", "x0", "states", "inputs", "status"),
    "pd_meas": ("model", "pd", "meas", "noise", "x0", "states", "inputs", "status"),
    "pd_bwd": ("model", "pd", "states", "inputs", "jac", "g_states"),
    "pd_meas_bwd": ("model", "pd", "meas", "states", "inputs", "jac", "g_states"),
}
OPTIONAL = ("lengths", "mu", "var", "g_x0", "g_u", "g_inputs", "g_gains")  # NULL by default: in the sweeps, nothing is asked for


def abi():
    from mc_pilco_amd import hipabi

    return hipabi


def model(U=1, **edit):
    """A valid small model: S 4, U 1, G 2, D 6 (one angle, speed integration); U = 2: two angles, D 8.  ``edit``: field = value, or
    field = (index, value) for an array, or gp_<field> / kern_<field> = value on GP 0."""
    m = abi().Model()
    m.S, m.U, m.G, m.Ts = 4, U, 2, 0.05
    ang, nang = ([2], [0, 1, 3]) if U == 1 else ([0, 1], [2, 3])
    m.n_angle, m.n_not_angle, m.D = len(ang), len(nang), len(nang) + 2 * len(ang) + U
    for i, v in enumerate(ang):
        m.angle[i] = v
    for i, v in enumerate(nang):
        m.not_angle[i] = v
    for g, (v, p) in enumerate(((1, 0), (3, 2)) if U == 1 else ((2, 0), (3, 1))):
        m.vel[g], m.not_vel[g], m.var_scale[g] = v, p, 1.0
        gp = m.gp[g]
        gp.kern.D, gp.kern.poly_deg, gp.kern.lam, gp.kern.inv_ls = m.D, 0, 1.0, PTR
        gp.N, gp.Npad, gp.Xt, gp.X, gp.alpha, gp.Kinv = 20, 32, PTR, PTR, PTR, PTR
    for k, v in edit.items():
        obj, name = (m.gp[0].kern, k[5:]) if k.startswith("kern_") else (m.gp[0], k[3:]) if k.startswith("gp_") else (m, k)
        if isinstance(v, tuple):
            getattr(obj, name)[v[0]] = v[1]
        else:
            setattr(obj, name, v)
    return m


def pd_desc(U=1, **edit):
    """A valid PD descriptor over model(U): input k reads position k and velocity 2 + k, squashed at 1."""
    p = abi().PDPolicy()
    p.U, p.squash, p.sqrt_kp, p.sqrt_kd, p.target_traj, p.target_rows = U, 1, PTR, PTR, PTR, T + 2
    for k in range(min(U, abi().MAX_INPUT)):
        p.pos[k], p.vel[k], p.u_max[k] = k, 2 + k, 1.0
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def meas_desc(**edit):
    """A valid measurement model: the pairs (0, 2) and (1, 3), the filter of tests/pd_meas_models.FILTER."""
    ms = abi().Meas()
    ms.n, ms.b0, ms.b1, ms.a0, ms.a1, ms.meas = 2, 0.42, 0.31, 1.25, -0.38, PTR
    for i in range(2):
        ms.pos[i], ms.vel[i], ms.std_pos[i] = i, 2 + i, 0.1
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(ms, k)[v[0]] = v[1]
        else:
            setattr(ms, k, v)
    return ms


def call(entry, **over):
    """The entry on valid arguments (M 5, T 3, every required buffer a dummy address, every optional one NULL) with ``over`` put in."""
    a = abi()
    args = dict(model=model(), pd=pd_desc(), meas=meas_desc(), noise=a.Noise(), M=M, T=T, particle_pred=1, Mu=M)
    args.update(over)
    vals = []
    for name in SIGS[entry]:
        if name in args:
            v = args[name]
            vals.append(C.byref(v) if isinstance(v, C.Structure) else v)
        else:
            vals.append(None if name in OPTIONAL or (name == "jac" and entry in ("open", "pd", "pd_meas")) else PTR)
    return getattr(a.lib(), "mcp_rollout_" + entry)(*vals, None)


def codes(entries, **over):
    return {e: call(e, **over) for e in entries}


def all_are(entries, code):
    return {e: code for e in entries}


def test_the_sweeps_accept_valid_arguments_with_nothing_asked_for():
    assert codes(BWD) == {"open_bwd": 0, "pd_bwd": 0, "pd_meas_bwd": 0}


@pytest.mark.parametrize("entry", ALL)
def test_null_pointers(entry):
    for name in REQUIRED[entry]:
        assert call(entry, **{name: None}) == -1, name
    if entry in PD:  # the descriptor's own device pointers
        for name in ("sqrt_kp", "sqrt_kd", "target_traj"):
            assert call(entry, pd=pd_desc(**{name: None})) == -1, name


def test_sizes():
    assert codes(ALL, M=0) == all_are(ALL, -1)
    assert codes(ALL, M=-3) == all_are(ALL, -1)
    assert codes(OPEN, T=1) == all_are(OPEN, -1)  # the open-loop three need a transition
    assert codes(PD, T=0) == all_are(PD, -1)  # the PD four take T = 1: the policy alone
    assert codes(("open", "open_rec"), Mu=3) == {"open": -1, "open_rec": -1}  # Mu is 1 or M
    assert codes(("open", "open_rec"), Mu=0) == {"open": -1, "open_rec": -1}


def test_compiled_limits():
    for edit in (dict(S=17), dict(U=9), dict(G=9), dict(D=33)):
        assert codes(ALL, model=model(**edit)) == all_are(ALL, -2), edit
    # more training points than MCP_MAX_TRAIN: the forward entries refuse; the sweeps never read a GP descriptor
    assert codes(ALL, model=model(gp_N=4097, gp_Npad=4112)) == {"open": -2, "open_rec": -2, "pd": -2, "pd_meas": -2, "open_bwd": 0, "pd_bwd": 0, "pd_meas_bwd": 0}


def test_precedence():
    assert codes(ALL, M=0, model=model(S=17)) == all_are(ALL, -1)  # sizes before limits
    assert codes(ALL, model=model(S=17, angle=(0, 9))) == all_are(ALL, -2)  # limits before the model's lists
    assert codes(PD, model=model(angle=(0, 9)), pd=pd_desc(U=9)) == all_are(PD, -1)  # the model before the PD descriptor
    assert codes(MEAS, pd=pd_desc(U=9), meas=meas_desc(a0=0.0)) == all_are(MEAS, -2)  # the PD descriptor before the measurement


# An index listed twice, on model() (angle [2], not_angle [0, 1, 3], vel [1, 3], not_vel [0, 2]): the kernels find a component's place with a
# last-match loop and let the thread of vel[g] report GP g, so each of these would leave a z slot or a mu / var row unwritten.  In order: twice
# in angle (angle [2, 2], not_angle [0]: D stays 6), twice in not_angle, twice in vel, twice in not_vel, vel[1] also not_vel[0].
REPEATED_INDEX = [dict(n_angle=2, angle=(1, 2), n_not_angle=1), dict(not_angle=(1, 0)), dict(vel=(0, 3)), dict(not_vel=(1, 0)), dict(not_vel=(0, 3))]


@pytest.mark.parametrize("edit", [dict(angle=(0, 9)), dict(angle=(0, -1)), dict(not_angle=(0, 4)), dict(vel=(0, 4)), dict(vel=(1, -1)),
                                  dict(not_vel=(0, -2)), dict(not_vel=(1, 4)), dict(n_not_angle=2), dict(n_angle=-1), dict(n_not_angle=-1),
                                  dict(S=0), dict(G=0)] + REPEATED_INDEX, ids=str)
def test_model_list_errors(edit):
    """Refused by every entry -- by the sweeps even though nothing is asked for."""
    assert codes(ALL, model=model(**edit)) == all_are(ALL, -1)


def test_an_index_in_angle_and_in_not_angle_is_allowed():
    """Both features are formed (tests/width_models.py narrow_overlap_d7, tests/layout_models.py mixed5): component 2 as the fourth plain one."""
    assert codes(BWD, model=model(n_not_angle=4, not_angle=(3, 2), D=7)) == all_are(BWD, 0)
    assert codes(BWD, model=model(not_vel=(0, -1))) == all_are(BWD, 0) and codes(BWD, model=model(not_vel=(1, -1))) == all_are(BWD, 0)


def test_not_vel_minus_one_is_a_delta_state_gp():
    assert codes(BWD, model=model(not_vel=(0, -1))) == all_are(BWD, 0)


@pytest.mark.parametrize("edit", [dict(gp_Kinv=None), dict(gp_Xt=None), dict(gp_alpha=None), dict(kern_inv_ls=None), dict(gp_Npad=40), dict(gp_N=0),
                                  dict(gp_N=33), dict(kern_poly_deg=3), dict(kern_poly_deg=-1), dict(kern_poly_deg=1), dict(kern_D=5)], ids=str)
def test_gp_operand_errors_are_the_forward_entries_alone(edit):
    """(poly_deg = 1 without w1 / aX is an operand error too.)  The sweeps run from the record: they never look at a GP."""
    assert codes(FWD, model=model(**edit)) == all_are(FWD, -1)
    assert codes(BWD, model=model(**edit)) == all_are(BWD, 0)


def test_the_sweeps_accept_a_model_without_gp_operands():
    a = abi()
    m = model()
    for g in range(a.MAX_GP):
        C.memset(C.byref(m.gp[g]), 0, C.sizeof(a.GP))
    assert codes(BWD, model=m) == all_are(BWD, 0)
    assert codes(FWD, model=m) == all_are(FWD, -1)


def test_the_record_of_the_pd_sweeps():
    """jac is required from T = 2 on; T = 1 is the policy alone and has no record."""
    for e in ("pd_bwd", "pd_meas_bwd"):
        assert call(e, T=2, jac=None) == -1
        assert call(e, T=1, jac=None) == 0


def test_pd_descriptor():
    assert codes(PD, pd=pd_desc(U=9)) == all_are(PD, -2)  # over MCP_MAX_INPUT
    assert codes(PD, pd=pd_desc(U=2)) == all_are(PD, -1)  # not the model's U
    assert codes(PD, pd=pd_desc(U=0)) == all_are(PD, -1)
    assert codes(PD, pd=pd_desc(target_rows=T - 1)) == all_are(PD, -1)
    assert codes(PD, pd=pd_desc(pos=(0, 4))) == all_are(PD, -1)
    assert codes(PD, pd=pd_desc(vel=(0, -1))) == all_are(PD, -1)
    assert codes(PD, pd=pd_desc(u_max=(0, 0.0))) == all_are(PD, -1)  # squash needs u_max > 0
    assert codes(PD, pd=pd_desc(u_max=(0, float("nan")))) == all_are(PD, -1)
    assert codes(BWD[1:], pd=pd_desc(u_max=(0, 0.0), squash=0)) == all_are(BWD[1:], 0)  # without squashing u_max is not read
    m2 = model(U=2)
    assert codes(BWD[1:], model=m2, pd=pd_desc(U=2)) == all_are(BWD[1:], 0)
    assert codes(PD, model=m2, pd=pd_desc(U=2, pos=(1, 0))) == all_are(PD, -1)  # a repeated pos
    assert codes(PD, model=m2, pd=pd_desc(U=2, vel=(1, 2))) == all_are(PD, -1)  # a repeated vel


def test_measurement():
    """The ten cases of tests/test_gpu_pd_meas.py::test_refusals_leave_the_status_word_alone, on both directions."""
    for name, over in (("meas NULL", dict(meas=None)), ("pos out of range", dict(meas=meas_desc(pos=(0, 4)))),
                       ("vel negative", dict(meas=meas_desc(vel=(1, -1)))), ("pos repeated", dict(meas=meas_desc(pos=(1, 0)))),
                       ("vel repeated", dict(meas=meas_desc(vel=(1, 2)))), ("listed as both", dict(meas=meas_desc(vel=(1, 0)))),
                       ("no meas buffer", dict(meas=meas_desc(meas=None))), ("a0 == 0", dict(meas=meas_desc(a0=0.0))),
                       ("a0 NaN", dict(meas=meas_desc(a0=float("nan")))), ("Ts <= 0", dict(model=model(Ts=0.0)))):
        assert codes(MEAS, **over) == {"pd_meas": -1, "pd_meas_bwd": -1}, name
    assert codes(MEAS, meas=meas_desc(n=3)) == {"pd_meas": -1, "pd_meas_bwd": -1}  # more pairs than S / 2
    assert codes(MEAS, meas=meas_desc(n=-1)) == {"pd_meas": -1, "pd_meas_bwd": -1}
    # Ts <= 0 is the measurement's own check: the same model passes when no pair is measured
    assert call("pd_meas_bwd", model=model(Ts=0.0), meas=abi().Meas()) == 0
    assert call("pd_meas_bwd", meas=meas_desc()) == 0


def test_packed_model_names_the_list():
    """ops.PackedModel raises ValueError with the list's name where the C entries would answer a bare MCP_ERR_ARG (before anything is
    packed: no GPU is touched)."""
    from mc_pilco_amd import ops

    good = dict(angle=[2], not_angle=[0, 1, 3], vel=[1, 3], not_vel=[0, 2])
    for name, bad in (("angle", [2, 2]), ("not_angle", [0, 0, 3]), ("vel", [3, 3]), ("not_vel", [0, 0])):
        with pytest.raises(ValueError, match="model's %s list" % name):
            ops.PackedModel([], 4, 1, 0.05, **dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="vel and not_vel lists share"):
        ops.PackedModel([], 4, 1, 0.05, **dict(good, not_vel=[3, 2]))
    # allowed: an index in angle and in not_angle, several GPs without a position -- these get as far as the (here empty) list of GPs
    for ok in (dict(good, not_angle=[0, 1, 2, 3]), dict(good, not_vel=[-1, -1])):
        with pytest.raises(IndexError):
            ops.PackedModel([], 4, 1, 0.05, **ok)
