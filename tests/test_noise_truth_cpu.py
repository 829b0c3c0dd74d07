"""CPU: tests/noise_truth.py against the published Philox4x32-10, its addressing (injective inside the supported ranges, and the collisions just
outside that are the reason for them), its double-precision normal against the high-precision one, the sensitivity of every table set of
tests/noise_truth_cases.py to every wrong generator of ``noise_truth.MUTANTS``, and the conditions of the cases on the oracle alone.

Sensitivity, as it is read here.  A wrong generator is told apart on a table when a keep bit differs or a normal differs by more than 1e-3.  A
mutant cannot change a table it has no part in (sin for cos leaves every keep bit; a dropped high word of ``call`` leaves every launch with
call < 2^32), so ``must_differ`` states, from the mutant's definition alone, on which (table set, table) it has a part; there the table MUST
differ, every mutant has at least one such table, and the mutants of the generator's core (rounds, multipliers, key bump) have all of them.  Two
mutants move almost nothing almost everywhere and get a case built for them: > for >= needs a word EQUAL to the threshold
(noise_truth_cases.p_on_a_drawn_word), 32-bit uniforms move a normal by 1e-3 only where the first word is below ~2^5 (RARE_PARTICLE in the
last-bit tier's swarm)."""
import itertools

import numpy as np
import pytest

import noise_truth as nt
import noise_truth_cases as ntc
import status_models as sm


def _straight(counter, key):
    """Philox4x32-10 as the paper states it, one block, Python integers."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KNOWN = [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_known_answers(counter, key, want):
    assert _straight(counter, key) == want
    assert [int(q) for q in nt.philox4x32_10(counter, key)] == want


def test_vectorised_generator_is_the_straight_one():
    rs = np.random.RandomState(0)
    c, k = rs.randint(0, 2 ** 32, size=(4, 64), dtype=np.uint64), rs.randint(0, 2 ** 32, size=(2, 64), dtype=np.uint64)
    got = np.stack(nt.philox4x32_10(c, k))
    for i in range(64):
        assert [int(v) for v in got[:, i]] == _straight([int(v) for v in c[:, i]], [int(v) for v in k[:, i]])


# ---- addressing ----------------------------------------------------------------------------------------------------------------------------------
PARTICLES = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, nt.PARTICLE_LIMIT - 1]
STEPS = [0, 1, 255, 256, nt.T_LIMIT - 1]
INDICES = [0, 1, 3, 2 ** 32 - 1]
CALLS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 64 - 1]
SEEDS = [0, 1, 2 ** 32, (0xA5A5A5A5 << 32) | 7, 2 ** 64 - 1]


def _ck(seed, call, p, t, s, i):
    c, k = nt.counter_key(seed, call, p, t, s, i)
    return tuple(int(q) for q in c) + tuple(int(q) for q in k)


def test_counter_and_key_are_injective_inside_the_supported_ranges():
    """Per seed: no two (particle, t, stream, index, call) share a (counter, key).  Across seeds: none either while call < 2^32 (the high word of
    ``call`` is XORed into the key word that holds the seed's low word -- see the alias below)."""
    for seed in SEEDS:
        seen = {}
        for tup in itertools.product(CALLS, PARTICLES, STEPS, (0, 1, 2), INDICES):
            assert seen.setdefault(_ck(seed, *tup), tup) == tup, (seed, tup)
    seen = {}
    for tup in itertools.product(SEEDS, [c for c in CALLS if c < 2 ** 32], PARTICLES, STEPS, (0, 1, 2), INDICES):
        assert seen.setdefault(_ck(*tup), tup) == tup, tup


def test_collisions_just_outside_the_supported_ranges():
    """Why the ranges are what they are: each pair below is ONE (counter, key)."""
    assert _ck(5, 9, nt.PARTICLE_LIMIT, 0, 0, 0) == _ck(5, 9, 0, 1, 0, 0)  # particle id 2^40 at t = 0 is particle 0 at t = 1
    assert _ck(5, 9, 3, nt.T_LIMIT, 0, 0) == _ck(5, 9, 3, 0, 1, 0)  # t = 2^22 on the eps stream is t = 0 on the mask stream
    assert _ck(1, 0, 3, 4, 0, 0) == _ck(0, 2 ** 32, 3, 4, 0, 0)  # seeds that differ in their low word by hi32(call): one run's calls stay distinct


# ---- the normal ----------------------------------------------------------------------------------------------------------------------------------
def _extreme_words():
    """All-zero and all-one words, and the u2 nearest 1/4 and 3/4 (2 u2 = j 2^-52 with j = 2^51 -+ 1 and 3 2^51 -+ 1), each with small and large u1."""
    u2 = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (2 ** 30 - 1, 0xFFFFF000), (2 ** 30, 0), (3 * 2 ** 30 - 1, 0xFFFFF000), (3 * 2 ** 30, 0),
          (2 ** 31 - 1, 0xFFFFF000), (2 ** 31, 0)]  # (the last two: nearest 1/2, where cospi is -1 to the last bit)
    u1 = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x12345678, 0x9ABCDEF0), (19, 0x80000000)]
    w = np.array([(a, b, c, d) for (a, b) in u1 for (c, d) in u2], dtype=np.uint64)
    return tuple(w[:, i] for i in range(4))


def test_double_precision_normal_against_the_high_precision_one():
    """>= 2^16 draws plus the extreme uniforms.  Bound, from the formula's own error in double: log u1 to 1 ulp, halved by the square root and its
    rounding added (1 ulp together); the argument pi (n 2^-52) carries two roundings and pi's own, ~1.5 ulp, which cos / sin on [0, pi/4] pass on
    at a relative sensitivity <= 1, plus their own 1 ulp; the product 0.5: ~5 ulp, asserted at 8."""
    if not nt.have_longdouble():
        pytest.skip("np.longdouble is a double here")
    t, m, g = nt._grid(0, 4, 8192, 2, 2 ** 32 - 100)
    words = nt.draw(ntc.LASTBIT_SEED, 5, m, t, 0, g)
    words = tuple(np.concatenate([q.reshape(-1), e]) for q, e in zip(words, _extreme_words()))
    assert words[0].size >= 2 ** 16
    d, hp = nt.normal_of_words(words), nt.normal_hp_of_words(words)
    u = nt.ulps(d, hp)
    print("double against longdouble: max %.3f ulp over %d draws; |normal| up to %.3f" % (u.max(), u.size, np.abs(d).max()))
    assert np.isfinite(d).all() and u.max() < 8.0
    assert np.abs(d).max() < 8.6  # sqrt(-2 log 2^-53) = 8.57
    assert d[-32] > 8.5  # (all-zero words: the largest normal there is)


def test_high_precision_normal_against_mpmath():
    """The longdouble evaluation against 40-digit arithmetic on a subset and the extremes: within 2^-8 of a double's ulp."""
    mpmath = pytest.importorskip("mpmath")
    if not nt.have_longdouble():
        pytest.skip("np.longdouble is a double here")
    words = nt.draw(ntc.LASTBIT_SEED, 5, np.arange(256, dtype=np.uint64), 1, 0, 0)
    words = tuple(np.concatenate([q, e]) for q, e in zip(words, _extreme_words()))
    hp, mp = nt.normal_hp_of_words(words), nt.normal_mp_of_words(words)
    with mpmath.workdps(40):
        for a, b in zip(hp, mp):
            err = abs(mpmath.mpf(float(a)) + mpmath.mpf(float(a - np.longdouble(float(a)))) - b)  # (a, exactly: its double and the rest)
            assert err <= abs(b) * mpmath.mpf(2) ** -60, (a, b)


def test_drop_threshold():
    assert nt.drop_threshold(0.25) == 2 ** 30 and nt.drop_threshold(0.1) == 429496729 and nt.drop_threshold(0.0) == 0
    assert nt.drop_threshold(1.0) == 0xFFFFFFFF and nt.drop_threshold(1.0 - 2.0 ** -40) == 0xFFFFFFFF
    p, b = ntc.p_on_a_drawn_word()
    assert 0.2 < p < 0.4
    spec = ntc.keep_spec(p, 200)
    assert bool(spec.tables()["masks"][0, 0, b]) and not bool(spec.tables("keep_gt")["masks"][0, 0, b])


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------------------
def must_differ(mutant, spec, kind):
    """Whether the mutant, by its definition, has a part in table ``kind`` of ``spec`` (module docstring)."""
    call = nt.total_call(spec.call, spec.dev)
    normal = kind in ("eps", "pos")
    if mutant in ("rounds9", "swapped_multipliers", "no_key_bump"):
        return True
    if mutant in ("keep_word_order", "keep_index_b"):
        return kind == "masks"
    if mutant == "keep_gt":
        return kind == "masks" and spec.p == ntc.KEEP_PS[2] and spec.offset == 0
    if mutant == "t_dropped":  # (a table whose only row is drawn at t = 0 has no t in it)
        return kind in ("masks", "pos") or spec.T >= 3 or spec.t0 > 0
    if mutant == "pos_t_minus_1":
        return kind == "pos"
    if mutant == "stream_dropped":
        return kind in ("masks", "pos")
    if mutant == "call_hi_dropped":
        return call >= 2 ** 32
    if mutant == "seed_hi_dropped":
        return spec.seed >= 2 ** 32
    if mutant == "particle_hi_dropped":
        return spec.offset + spec.M > 2 ** 32
    if mutant == "call_no_carry":
        return nt.total_call(spec.call, spec.dev, "call_no_carry") != call
    if mutant == "uniform32":
        return normal and spec.t0 == 0 and spec.offset <= ntc.RARE_PARTICLE < spec.offset + spec.M and spec.seed == ntc.LASTBIT_SEED and call == ntc.LASTBIT_CALL
    if mutant == "sin_for_cos":
        return normal
    raise AssertionError(mutant)


def _differs(kind, a, b):
    return bool((a != b).any()) if kind == "masks" else float(np.abs(a - b).max()) > 1e-3


SPECS = ntc.specs()


@pytest.mark.parametrize("mutant", nt.MUTANTS)
def test_every_mutant_changes_the_tables_the_gpu_tests_use(mutant):
    told = 0
    for spec in SPECS:
        true, wrong = spec.tables(), spec.tables(mutant)
        for kind in true:
            if must_differ(mutant, spec, kind):
                assert _differs(kind, true[kind], wrong[kind]), "%s does not change %s of %s" % (mutant, kind, spec.name)
                told += 1
            elif mutant not in ("uniform32", "keep_gt"):  # (these two move something nearly everywhere, only not by the criterion)
                assert not _differs(kind, true[kind], wrong[kind]), "must_differ is wrong about %s on %s of %s" % (mutant, kind, spec.name)
    print("%s: told apart on %d tables" % (mutant, told))
    assert told >= 1


# ---- conditions ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(set(ntc.FORM_KEYS) | set(ntc.SWEEP_KEYS)), ids=lambda k: "%s-M%d" % k)
def test_conditions_of_the_width_class_cases(key):
    c = sm.case(key[0])
    print(key, "smallest variance / kzz %.3e" % ntc.check(c, ntc.spec_of(c, key[1])))


@pytest.mark.parametrize("name", list(ntc.EDGES))
def test_conditions_of_the_addressing_edges(name):
    print(name, "smallest variance / kzz %.3e" % ntc.check(sm.case(ntc.EDGE_CASE), ntc.edge_spec(name)))


def test_edges_that_must_draw_the_same_bits_do_in_the_truth():
    for a, b in ntc.SAME_BITS:
        ta, tb = ntc.edge_spec(a).tables(), ntc.edge_spec(b).tables()
        assert all(np.array_equal(ta[k], tb[k]) for k in ta), (a, b)
    assert not np.array_equal(ntc.edge_spec("call-2^32").tables()["eps"], ntc.edge_spec("call-2^32-1").tables()["eps"])


@pytest.mark.parametrize("fam", ntc.FAMILIES)
def test_conditions_of_the_other_families(fam):
    """Their truth functions return the smallest variance met (kzz >= lambda = 1 on these models) and raise nothing: finite throughout."""
    import torch

    tr = ntc.family_truth(fam)[2]
    print(fam, "smallest variance %.3e" % tr[-1])
    assert tr[-1] > ntc.VAR_FLOOR
    assert all(bool(torch.isfinite(q).all()) for q in tr[:-1] if isinstance(q, torch.Tensor))
