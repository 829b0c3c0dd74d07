"""CPU side of the status-word tests (tests/status_models.py, tests/test_gpu_status_word.py), on the oracle alone -- nothing is provoked on a device:

  * every (case, construction, M) of the form table meets the conditions of the constructions: the truth word is the one the construction names,
    every finite variance of the altered GP is at least 1e-3 kzz away from 0 at every step, the other GPs' variances stay positive by the same
    margin, construction B has a healthy and a bad particle in its first cluster and particle M - 1 bad, and on the row-split shape the bad
    particles' variance is negative only once the senders' partial sums are added;
  * the truth distinguishes what a wrong kernel would do: the flag taken from GP 0 only, particle M - 1 left out, NaN variances counted as
    non-positive -- each changes the expected word of a construction in the table;
  * the forms of the table are the ones the library's plan gives for their requests on an MI355X's 256 compute units (the plan query runs on the
    host), so that the GPU test's assertion on the report proves a form was reached, not requested."""
import numpy as np
import pytest

import status_models as sm

NAN, NONPOS = sm.STATUS_NAN, sm.STATUS_NONPOS_VAR


@pytest.mark.parametrize("name,M", sm.TRUTH_KEYS, ids=lambda v: str(v))
def test_constructions_meet_their_conditions(name, M):
    c = sm.case(name)
    line = []
    for con in sm.CONS:
        smallest = sm.check(c, con, M)
        tr, op = sm.truth(c, con, M), sm.operands(c, con, M)
        assert tr.word == sm.expected_word(con)
        assert tr.states.shape == (c.T, M, c.S) and tr.inputs.shape == (c.T, M, c.U) and tr.var.shape == (c.T - 1, M, c.G)
        if con.kind == "B":
            line.append("%s: factor %.4f, %d bad, smallest |var| / kzz %.3e" % (con.id, op["factor"], len(op["bad"]), smallest))
    print(name, "M", M, "T", c.T, "|", "; ".join(line))


def test_expected_words():
    assert [sm.expected_word(q) for q in (sm.A0, sm.AL, sm.B0, sm.BL, sm.C0, sm.CL, sm.DAL, sm.DB0, sm.DBL)] == \
        [NONPOS, NONPOS, NONPOS | NAN, NONPOS | NAN, NAN, NAN, 0, 0, 0]
    from mc_pilco_amd import hipabi

    assert (hipabi.STATUS_NAN, hipabi.STATUS_NONPOS_VAR) == (NAN, NONPOS)


SENS = [("d15_p10_g3", 5), ("u5_g5_d16", 17), ("narrow_disjoint_d6_pms", 5), ("d25_s16_g8", 33)]


@pytest.mark.parametrize("name,M", SENS, ids=lambda v: str(v))
def test_truth_is_sensitive_to_a_flag_taken_from_gp_0_only(name, M):
    """A kernel in which only the workgroup (or the pass) of GP 0 reports: the variance of g* = G - 1 goes unseen."""
    c = sm.case(name)
    tr = sm.truth(c, sm.AL, M)
    assert tr.word == NONPOS and sm.word_of(tr, gps=[0]) == 0
    tr = sm.truth(c, sm.BL, M)
    assert tr.word == NONPOS | NAN and not (sm.word_of(tr, gps=[0]) & NONPOS)
    for con in (sm.A0, sm.B0):  # (and the first GP is seen by it: the two placements tell the cases apart)
        assert sm.word_of(sm.truth(c, con, M), gps=[0]) & NONPOS


@pytest.mark.parametrize("name,M", SENS, ids=lambda v: str(v))
def test_truth_is_sensitive_to_particle_m_minus_1_left_out(name, M):
    """A validity mask that ends one particle early (or a ragged tile that drops its only real particle): in C-last the NaN sits in particle M - 1
    alone, and in B that particle is the bad one nearest the sign change."""
    c = sm.case(name)
    tr = sm.truth(c, sm.CL, M)
    assert tr.word == NAN and sm.word_of(tr, particles=range(M - 1)) == 0
    tr, op = sm.truth(c, sm.BL, M), sm.operands(c, sm.BL, M)
    assert M - 1 in op["bad"] and tr.var[0, M - 1, c.G - 1] < 0.0
    only_last = [m for m in range(M) if np.isfinite(tr.states[:, m]).all()] + [M - 1]  # (the particles that stay healthy to the end, and M - 1)
    assert len(only_last) >= 2
    assert sm.word_of(tr, particles=only_last) == NONPOS | NAN and sm.word_of(tr, particles=only_last[:-1]) == 0


@pytest.mark.parametrize("name,M", SENS, ids=lambda v: str(v))
def test_truth_is_sensitive_to_nan_variances_counted_as_non_positive(name, M):
    """`!(var > 0)` in place of `var <= 0`: a diverged particle (the retry case) would raise the reference's ValueError."""
    c = sm.case(name)
    for con in (sm.C0, sm.CL):
        tr = sm.truth(c, con, M)
        assert np.isnan(tr.var).any()
        assert tr.word == NAN and sm.word_of(tr, nan_is_nonpos=True) == NAN | NONPOS


def test_row_split_shape_needs_the_senders_sums():
    """u5_g5_d16_n128, construction B: with the finishing part's own rows of Kinv alone (rows 64 .. 127 with two and with three parts) the variance of
    every bad particle is still positive by the margin; the whole sum makes it negative."""
    c = sm.case("u5_g5_d16_n128")
    assert sm.fin_rows(c, 0, 2) == sm.fin_rows(c, 0, 3) == list(range(64, 128)) and sm.fin_rows(sm.case("u5_g5_d16"), 0) is None
    for con in (sm.B0, sm.BL):
        tr, g = sm.truth(c, con, 17), con.gstar(c)
        neg = np.isfinite(tr.var[:, :, g]) & (tr.var[:, :, g] < 0.0)
        assert neg[0].sum() >= 2
        print(con.id, "var / kzz of the bad particles: whole %s | own rows only %s" % (
            np.array2string(tr.var[:, :, g][neg] / tr.kzz[:, :, g][neg], precision=3), np.array2string(tr.var_fin[neg] / tr.kzz[:, :, g][neg], precision=3)))
        assert (tr.var_fin[neg] > sm.MARGIN * tr.kzz[:, :, g][neg]).all() and (tr.var[:, :, g][neg] < -sm.MARGIN * tr.kzz[:, :, g][neg]).all()


def test_reordering_the_training_rows_moves_b_far_less_than_the_bound():
    """The reference against itself (the training rows of g* permuted: another summation order) on construction B, where sqrt(var) near the margin
    amplifies most, over every (case, M) of the table: the spread (1.8e-14) stays orders below the 1e-9 the GPU test holds the finite entries to."""
    worst = 0.0
    for name, M in sm.TRUTH_KEYS:
        for con in (sm.B0, sm.BL):
            worst = max(worst, sm.reorder_spread(sm.case(name), con, M))
    print("largest spread of the oracle under a permutation of the training rows, construction B: %.2e" % worst)
    assert 4.0 * worst < 1e-9


@pytest.mark.parametrize("form", [f for f in sm.FORMS if not f.no_grad], ids=lambda f: f.id)
def test_forms_are_what_the_plan_gives(form):
    from mc_pilco_amd import hipabi

    c = sm.case(form.case)
    for sample in (True, False):
        fp = sm.plan(c, form.M, form.request(), sample)
        got = sm.plan_words(fp)
        if form.want is not None:
            assert sm.matches(form.want, got), (form.id, "wanted", form.want, "the plan says", got)
        else:
            assert fp.ran_particles in (1, 2, 4, 16)
        assert fp.family in (hipabi.FWD_SMALL_SHARDED, hipabi.FWD_LEAN, hipabi.FWD_TILE_SHARDED, hipabi.FWD_TILE, hipabi.FWD_SMALL)
        assert (fp.ran_fwd_lean == 1) == (fp.family == hipabi.FWD_LEAN)


def test_form_table_reaches_every_row():
    """Every family, every particle width of the small and lean kernels, both staging modes, several GP passes, the policy split, the row split in two
    and three parts under both deals -- each pinned by a ``want`` the plan test above holds against the library."""
    want = [f.want for f in sm.FORMS if f.want is not None]
    assert {(w[0], w[1]) for w in want} >= {(sm.FWD_LEAN, 1), (sm.FWD_LEAN, 2), (sm.FWD_LEAN, 4), (sm.FWD_SMALL, 1), (sm.FWD_SMALL, 2), (sm.FWD_SMALL, 4),
                                           (sm.FWD_SMALL_SHARDED, 1), (sm.FWD_SMALL_SHARDED, 2), (sm.FWD_SMALL_SHARDED, 4), (sm.FWD_TILE, 16),
                                           (sm.FWD_TILE_SHARDED, 16)}
    assert {w[3] for w in want} >= {0, 2, 3} and {w[4] for w in want} >= {0, 1} and {w[5] for w in want} >= {0, 1}
    assert any(w[0] == sm.FWD_SMALL and w[6] is not None and w[6] < sm.case(f.case).G for f, w in ((f, f.want) for f in sm.FORMS if f.want is not None))
    assert {(f.row_split, f.cluster_map) for f in sm.FORMS if f.row_split} == {(2, 0), (2, 1), (3, 0), (3, 1)}
    import width_models as wm

    tile_cases = {f.case for f in sm.FORMS if f.want is not None and f.want[0] == sm.FWD_TILE}
    assert {wm.classes(sm.case(n))["tile"] for n in tile_cases} >= {0, 1, 2}
    assert {sm.case(f.case).deg for f in sm.FORMS if f.want is not None and f.want[0] == sm.FWD_LEAN} == {0, 1, 2}
    assert any(sm.case(f.case).pms is not None for f in sm.FORMS if f.want is not None and f.want[0] == sm.FWD_LEAN)
