"""The status word of mcp_rollout_fwd on every forward form: each form of the table in tests/status_models.py (``FORMS``) is sent the constructions
that must raise MCP_STATUS_NONPOS_VAR, MCP_STATUS_NAN, both, or nothing (``CONS``: A exact zero variance, B negative for some particles, C a NaN
particle, D the operands of A and B in mean mode), through ``ops.rollout`` with the policy parameters requiring grad (the Jacobian record is written;
no backward), against the oracle's truth (``status_models.truth``, cached per (case, construction, M); tests/test_status_models_cpu.py shows on the
CPU that the truth meets its margins and tells a wrong kernel apart).  Per (form, construction):

  1. the status word IS the truth's word (not a superset);
  2. the finite masks of states, inputs and, under the measurement model, the measured states are the oracle's;
  3. on the finite entries the bounds of tests/test_gpu_width_classes.py hold: 1e-9 absolute on states and inputs.  The measured velocities are
     differences of two noisy positions over Ts = 0.05 through a filter with b0 + b1 <= 1: 2 x 1e-9 / Ts = 4e-8 on the measured states.
     (Construction B scales Kinv and samples with sqrt(var) as near as 1e-3 kzz to 0; the oracle against itself with the training rows of g*
     permuted -- summation order alone -- moves states and inputs by 1.8e-14 at the most over every (case, M) of the table
     (tests/test_status_models_cpu.py measures it), so 4 x that spread, 7.2e-14, is far inside 1e-9 and the project's bound stays as it is.)
  4. the form that was meant to run did run: the dispatch report (ran_particles, ran_gp_sharded, ran_fwd_lean, ran_row_split) equals the plan's
     report words, and the plan of the same call (mcp_rollout_fwd_plan on the same descriptors, request, workspace size and CU count) has the
     family, particles per workgroup, sharding, row parts, policy split, LDS staging and GPs per pass that the table pins.  Automatic dispatch pins
     nothing but report == plan.

Coverage (form -> cases; M = 5 on the 1 / 2 / 4-particle forms: one full cluster and a ragged one; M = 17 / 33 on the 16-particle forms):

  lean 201 / 202 / 204                      narrow_disjoint_d6; with the measurement model narrow_disjoint_d6_pms
  lean 201 / 204, degree 1 and 2            narrow_disjoint_d6_deg1, narrow_disjoint_d6_deg2
  small-tile 1 / 2 / 4, 101 / 102 / 104     d15_p10_g3 (G 3), u5_g5_d16 (G 5), d8_u3_pms (measurement model)
  small-tile unstaged / several GP passes   d25_s16_g8 (G 8): unstaged 5 + 3 GPs per pass; staged 2 per pass (four passes); unstaged 3 + 3 + 2 at two
                                            particles: g* = 7 is in the last pass each time
  tile kernel 16, classes 0 / 1 / 2         narrow_traj_d7, d15_p10_g3, d25_s16_g8 (M 17 and 33)
  tile kernel GP-sharded (116)              narrow_disjoint_d6, u5_g5_d16 (M 17 and 33); delta_d11_u3, speed_mixed_p9 (M 33)
  ... with the policy split, and without    d15_p10_g3 (G 3, B 257, M 17)
  ... row split 2 / 3 parts, both deals     u5_g5_d16_n128 (N = Npad = 128, degree 1, M 17, T 3); and the same launch with the split off
  D = 32 fallback                           d32_u8_pms (a forced 16 / 116 runs the 4-particle kernel, unsharded)
  delta model, var_scale != 1               delta_d11_u3 (T = 2 here: status_models.T_OVERRIDE), speed_mixed_p9 -- 4, 104, 16, 116
  automatic dispatch                        every case above at M = 5 and 17
  the states-only call (torch.no_grad())    lean 204, small-tile 4, 104, tile 16, row split 3 parts: constructions A and B

MCP_STATUS_SYNC is not raised by any test: it would take a hand-off that times out."""
import numpy as np
import pytest

import status_models as sm
import width_models as wm
from forced_launch import against as _against
from forced_launch import launch

pytestmark = pytest.mark.gpu

BOUND, BOUND_MEAS = 1e-9, 2 * 1e-9 / wm.TS


def _launch(form, c, con):
    """One rollout of (case, construction) through the form (tests/forced_launch.py)."""
    return launch(form, c, sm.packed(c, con, form.M), sm.operands(c, con, form.M)["sample"])


@pytest.mark.parametrize("form", sm.FORMS, ids=lambda f: f.id)
def test_status_word_masks_and_values_vs_oracle(form):
    c = sm.case(form.case)
    failures = []
    for con in (sm.CONS_NO_GRAD if form.no_grad else sm.CONS):
        tr = sm.truth(c, con, form.M)
        assert tr.word == sm.expected_word(con)  # (the construction's word: tests/test_status_models_cpu.py)
        st, inp, mbuf, word, rep, fp = _launch(form, c, con)
        out = []
        # 4. the form
        got = sm.plan_words(fp)
        if rep != (fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, fp.ran_row_split):
            out.append("the report %s is not the plan's %s" % (rep, (fp.ran_particles, fp.ran_gp_sharded, fp.ran_fwd_lean, fp.ran_row_split)))
        if form.want is not None and not sm.matches(form.want, got):
            out.append("the table pins %s, the plan of this call says %s" % (form.want, got))
        if form.want is None and rep[0] not in (1, 2, 4, 16):
            out.append("automatic dispatch ran %d particles per workgroup" % rep[0])
        # 1. the word
        if word != tr.word:
            out.append("status word %d, the truth's is %d" % (word, tr.word))
        # 2., 3. masks and finite entries
        es = _against("states", st, tr.states, BOUND, out)
        eu = _against("inputs", inp, tr.inputs, BOUND, out)
        em = float("nan")
        if c.pms is not None and not form.no_grad:
            if mbuf is None:
                out.append("no measured states were left by the call")
            else:
                em = _against("measured", mbuf, tr.meas, BOUND_MEAS, out)
        print("%s %s: word %d (truth %d) ran %s plan %s | errs states %.2e inputs %.2e measured %.2e | non-finite states %d of %d" % (
            form.id, con.id, word, tr.word, rep, got, es, eu, em, int((~np.isfinite(tr.states)).sum()), tr.states.size))
        failures += ["%s: %s" % (con.id, q) for q in out]
    assert not failures, "\n".join(failures)
