"""The rollout dispatch without a GPU: the plan queries (mcp_rollout_fwd_plan / mcp_rollout_bwd_plan, include/mcpilco_hip_debug.h) against

  * tests/dispatch_table_mi355x.json -- what the library DECIDED on an MI355X at the commit before the dispatch became a plan
    (tools/record_dispatch_table.py: return codes and the six ``ran_*`` words of a few hundred real rollouts, automatic and forced), and
  * tests/width_models.py -- the Python restatement of the sweep's class rules; restatement and library check each other.

Descriptors are rebuilt from the recorded scalars with dummy non-null pointers: the queries test pointers for NULL and never follow them."""
import ctypes as C
import functools
import json
import os

import pytest

import width_models as wm

HERE = os.path.dirname(os.path.abspath(__file__))
DUMMY = 0x1000  # (never dereferenced)


@functools.lru_cache(maxsize=None)
def table():
    with open(os.path.join(HERE, "dispatch_table_mi355x.json")) as f:
        return json.load(f)


def make_model(s):
    from mc_pilco_amd import hipabi

    if s is None:
        return None
    m = hipabi.Model()
    m.S, m.U, m.G, m.D = s["S"], s["U"], s["G"], s["D"]
    m.n_angle, m.n_not_angle = len(s["angle"]), len(s["not_angle"])
    for i, v in enumerate(s["angle"]):
        m.angle[i] = v
    for i, v in enumerate(s["not_angle"]):
        m.not_angle[i] = v
    for g in range(s["G"]):
        m.vel[g], m.not_vel[g] = s["vel"][g], s["not_vel"][g]
        gp = m.gp[g]
        gp.N, gp.Npad, gp.kern.D, gp.kern.poly_deg = s["N"][g], s["Npad"][g], s["D"], s["poly_deg"][g]
        for f in ("Xt", "X", "alpha", "Kinv", "aX"):
            setattr(gp, f, DUMMY)
        for f in ("inv_ls", "w1", "w20", "w21"):
            setattr(gp.kern, f, DUMMY)
    return m


def make_policy(s):
    from mc_pilco_amd import hipabi

    p = hipabi.Policy()
    p.kind, p.S, p.P, p.B, p.U, p.squash = s["kind"], s["S"], s["P"], s["B"], s["U"], 1
    p.n_angle, p.n_non_angle, p.traj_len, p.p_drop = len(s["angle"]), len(s["non_angle"]), s["traj_len"], s["p_drop"]
    for i, v in enumerate(s["angle"]):
        p.angle[i] = v
    for i, v in enumerate(s["non_angle"]):
        p.non_angle[i] = v
    for f in ("log_ls", "centers", "weight", "u_max", "target_traj"):
        setattr(p, f, DUMMY)
    p.bias = DUMMY if s["bias"] else None
    p.meas.n = s["meas"]["n"]
    for i in range(p.meas.n):
        p.meas.pos[i], p.meas.vel[i] = s["meas"]["pos"][i], s["meas"]["vel"][i]
    if p.meas.n:
        p.meas.a0, p.meas.meas = 1.0, DUMMY
    return p


def make_request(words):
    from mc_pilco_amd import hipabi

    d = hipabi.Dispatch()
    for k, v in zip(table()["request_words"], words):
        setattr(d, k, v)
    return d


def query(model, policy, M, T, flags, fwd_bytes, bwd_bytes, cus, request):
    """(rc forward, forward plan, rc backward, backward plan)"""
    from mc_pilco_amd import hipabi

    L = hipabi.lib()
    fp, bp = hipabi.FwdPlan(), hipabi.BwdPlan()
    mp = None if model is None else C.byref(model)
    rf = L.mcp_rollout_fwd_plan(mp, C.byref(policy), M, T, flags, fwd_bytes, cus, C.byref(request), C.byref(fp))
    rb = L.mcp_rollout_bwd_plan(mp, C.byref(policy), M, T, flags, bwd_bytes, cus, C.byref(request), C.byref(bp))
    return rf, fp, rb, bp


def entry_query(e, cus=None):
    t = table()
    return query(make_model(t["models"][e["model"]]), make_policy(t["policies"][e["policy"]]), e["M"], e["T"], e["flags"], e["fwd_workspace_bytes"],
                 e["bwd_workspace_bytes"] or 0, t["cus"] if cus is None else cus, make_request(e["request"]))


def as_tuple(s):
    return tuple(getattr(s, f[0]) for f in s._fields_)


def test_table_is_complete():
    t = table()
    assert t["complete"] and t["cus"] > 0
    names = [e["name"] for e in t["entries"]]
    assert len(names) == len(set(names)) and len(names) >= 14 * 18 + 18 * 3
    assert t["ran_words"] == ["ran_particles", "ran_gp_sharded", "ran_fwd_lean", "ran_bwd_lean", "ran_row_split", "ran_bwd_pipe"]


def test_plans_reproduce_the_recorded_dispatch():
    """Return codes and all six report words of every entry, none skipped; two queries of the same call agree field by field."""
    t = table()
    wrong = []
    for e in t["entries"]:
        rf, fp, rb, bp = entry_query(e)
        rf2, fp2, rb2, bp2 = entry_query(e)
        assert (rf, as_tuple(fp), rb, as_tuple(bp)) == (rf2, as_tuple(fp2), rb2, as_tuple(bp2)), e["name"]
        got_rc = (rf, rb if e["rc_bwd"] is not None else None)
        ran = [fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, bp.ran_bwd_lean if e["rc_bwd"] is not None else 0, fp.ran_row_split,
               bp.ran_bwd_pipe if e["rc_bwd"] is not None else 0]
        if got_rc != (e["rc_fwd"], e["rc_bwd"]) or ran != e["ran"]:
            wrong.append((e["name"], got_rc, ran, (e["rc_fwd"], e["rc_bwd"]), e["ran"]))
    assert not wrong, "%d of %d entries differ, first: %s" % (len(wrong), len(t["entries"]), wrong[:5])


def test_no_plan_is_gp_sharded_without_a_cu_count():
    for e in table()["entries"]:
        rf, fp, _, _ = entry_query(e, cus=0)
        from mc_pilco_amd import hipabi

        assert fp.ran_gp_sharded == 0 and fp.family not in (hipabi.FWD_SMALL_SHARDED, hipabi.FWD_LEAN, hipabi.FWD_TILE_SHARDED), e["name"]
        assert fp.zero_xch == fp.zero_uxch == fp.zero_rxch == 0
        if rf == 0:
            assert fp.family in (hipabi.FWD_TILE, hipabi.FWD_SMALL)


def _pinned_shapes():
    """The two shapes of test_abi_cpu.py::test_argument_validation_without_gpu (scalars only: the size query reads nothing else)."""
    from mc_pilco_amd import hipabi

    m, p = hipabi.Model(), hipabi.Policy()
    p.P, p.B, p.U = 5, 200, 1
    yield m, p, 400, 150
    m, p = hipabi.Model(), hipabi.Policy()
    m.G, m.D = 6, 24
    for g in range(6):
        m.gp[g].Npad = 400
    p.P, p.B, p.U = 24, 8, 6
    yield m, p, 16, 5


def test_workspace_map_reproduces_the_size_query():
    """max(the forward map's total, the backward slabs) is mcp_rollout_workspace_bytes: for the two pinned shapes and for every table entry, where
    the size the parent commit's library reported (it summed the regions by hand) is the reference; the regions come in the documented order."""
    from mc_pilco_amd import hipabi

    L = hipabi.lib()
    t = table()
    cases = [(m, p, M, T, None) for m, p, M, T in _pinned_shapes()]
    cases += [(make_model(t["models"][e["model"]]), make_policy(t["policies"][e["policy"]]), e["M"], e["T"], e) for e in t["entries"]]
    for m, p, M, T, e in cases:
        mp = None if m is None else C.byref(m)
        size = L.mcp_rollout_workspace_bytes(mp, C.byref(p), M, T)
        if e is not None:
            assert size == e["fwd_workspace_bytes"] and (e["bwd_workspace_bytes"] is None or size == e["bwd_workspace_bytes"]), e["name"]
        fp = hipabi.FwdPlan()
        L.mcp_rollout_fwd_plan(mp, C.byref(p), M, T, 1, 0, 0, None, C.byref(fp))  # (the map is filled whatever the plan's fate)
        slabs = 8 * (p.P + p.B * p.P + p.U * p.B + p.U) * min(M, 1024)
        assert 0 == fp.ws_xch <= fp.ws_xj <= fp.ws_kt <= fp.ws_uxch <= fp.ws_rxch <= fp.ws_total
        assert max(fp.ws_total if m is not None else 0, slabs) == size


@pytest.mark.parametrize("c", wm.CASES, ids=lambda c: c.name)
def test_sweep_plan_agrees_with_the_python_restatement(c):
    """Every width case, every forced sweep width: the planned width is the request when ``sweep_widths`` has it, else the largest halving that it has;
    class, thread class and pipelined form are those of ``classes``."""
    from mc_pilco_amd import hipabi

    L = hipabi.lib()
    k, ok = wm.classes(c), wm.sweep_widths(c)
    s = dict(S=c.S, U=c.U, G=c.G, D=c.D, angle=list(c.angle), not_angle=list(c.not_angle), vel=list(c.vel), not_vel=list(c.not_vel), N=list(c.N),
             Npad=[(n + 15) // 16 * 16 for n in c.N], poly_deg=[c.deg] * c.G)
    ps = dict(kind={"plain": 0, "angles": 1, "traj": 2}[c.kind], S=c.S, P=c.P, B=c.B, U=c.U, angle=list(c.pol_angle), non_angle=list(c.pol_non_angle),
              traj_len=c.T, p_drop=wm.P_DROP, meas=dict(n=0 if c.pms is None else len(c.pms[0]), pos=list(c.pms[0]) if c.pms else [],
                                                        vel=list(c.pms[1]) if c.pms else []), bias=c.bias)
    m, p = make_model(s), make_policy(ps)
    M = 40
    size = L.mcp_rollout_workspace_bytes(C.byref(m), C.byref(p), M, c.T)
    assert ok and ok[0] == 1
    for pb in (1, 2, 4, 8):
        d = hipabi.Dispatch()
        d.bwd_particles = pb
        bp = hipabi.BwdPlan()
        assert L.mcp_rollout_bwd_plan(C.byref(m), C.byref(p), M, c.T, 1, size, 256, C.byref(d), C.byref(bp)) == 0
        want = pb
        while want not in ok:
            want //= 2
        assert bp.lean == 0 and bp.particles == want, (pb, bp.particles, ok)
        assert (bp.pfm, bp.um) == k["sweep"]
        nt = max(k["nt"], 64 * want)
        assert bp.maxnt == (256 if nt <= 256 else (1024 if k["sweep"][0] <= 16 else 512))
        if want == 1:
            assert bp.maxnt == k["maxnt"] and bp.pipe == int(k["pipe"]) and bp.threads == k["nt"] + 64 * bp.pipe
        else:
            assert bp.pipe == 0 and bp.threads == nt
        assert bp.slabs == (M + want - 1) // want and bp.launches == 1
