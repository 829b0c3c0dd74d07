"""What the in-kernel generator is documented to draw, restated on the CPU with numpy and Python integers: no project code is imported.  The GPU
tests (tests/test_gpu_noise_truth.py) feed these tables to the oracle and hold the Philox launches to the bounds the buffer launches meet;
tests/test_noise_truth_cpu.py checks this module against the published generator and shows that each wrong generator of ``MUTANTS`` changes
the tables.

Source of every statement: csrc/mcp_device.h:207-274 and the ``mcp_noise`` comment of include/mcpilco_hip.h.

  philox4x32_10   mcp_device.h:214-229.  Ten rounds of  (x, y, z, w) <- (hi(M1 z) ^ y ^ k0, lo(M1 z), hi(M0 x) ^ w ^ k1, lo(M0 x))  with
                  M0 = 0xD2511F53, M1 = 0xCD9E8D57; after each round k0 += 0x9E3779B9, k1 += 0xBB67AE85 (Salmon et al. 2011).
  the launch      :237-241.  call = (by-value call + *call_dev) mod 2^64.
  philox_draw     :243-253.  gp = particle + particle_offset (the GLOBAL particle id);
                  counter = (lo32(gp),  hi32(gp) ^ (stream << 30) ^ (t << 8),  index,  lo32(call));   key = (lo32(seed) ^ hi32(call),  hi32(seed)).
                  Streams: 0 the GP sample (eps), 1 the dropout keep bits, 2 the position measurement noise (:231-233).
  philox_normal   :256-262.  u1 = (((x << 20) | (y >> 12)) + 0.5) 2^-52, u2 likewise of (z, w): 52-bit uniforms on (0, 1);
                  normal = sqrt(-2 log u1) cospi(2 u2), index = the GP (eps) or the position pair (stream 2).
  philox_keep     :265-269.  basis / hidden unit b: word b & 3 (x, y, z, w) of the block of index b >> 2; kept iff word >= threshold.
  drop_threshold  :271-274.  floor(p 2^32), saturated at 0xFFFFFFFF.
  addressing      eps row t: step t;  masks row t: step t;  pos_noise row t - 1: step t (include/mcpilco_hip.h, mcp_meas.pos_noise).

Supported ranges (the word counter.y is shared): ``T_LIMIT`` -- t < 2^22, for t << 8 reaches the stream field at bit 30 there -- and
``PARTICLE_LIMIT`` -- a global particle id below 2^40, for its high word shares bits 8.. with t << 8: particle 2^40 at t = 0 IS particle 0 at t = 1
(tests/test_noise_truth_cpu.py shows the collision)."""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_EPS, STREAM_MASK, STREAM_POS = 0, 1, 2
T_LIMIT = 1 << 22
PARTICLE_LIMIT = 1 << 40
_M32 = np.uint64(0xFFFFFFFF)

# The wrong generators of the sensitivity test (issue list, in its order).  They exist in this truth only.
MUTANTS = ("rounds9", "swapped_multipliers", "no_key_bump", "keep_word_order", "keep_index_b", "keep_gt", "t_dropped", "pos_t_minus_1", "stream_dropped",
           "call_hi_dropped", "seed_hi_dropped", "particle_hi_dropped", "call_no_carry", "uniform32", "sin_for_cos")


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(counter, key, rounds=10, m0=M0, m1=M1, bump=True):
    """counter: four, key: two arrays of uint64 holding 32-bit words (broadcast against each other).  Returns the four output words."""
    x, y, z, w = (_u64(q) for q in counter)
    k0, k1 = (_u64(q) for q in key)
    m0, m1 = np.uint64(m0), np.uint64(m1)
    for _ in range(rounds):
        p0, p1 = m0 * x, m1 * z  # 32 x 32 -> 64 bits: exact in uint64
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & _M32
        if bump:
            k0, k1 = (k0 + np.uint64(W0)) & _M32, (k1 + np.uint64(W1)) & _M32
    return x, y, z, w


def total_call(call, call_dev=0, mutant=None):
    """The launch's call: by-value ``call`` plus the device word, mod 2^64."""
    if mutant == "call_no_carry":  # the halves added separately
        lo = ((call & 0xFFFFFFFF) + (call_dev & 0xFFFFFFFF)) & 0xFFFFFFFF
        hi = ((call >> 32) + (call_dev >> 32)) & 0xFFFFFFFF
        return (hi << 32) | lo
    return (int(call) + int(call_dev)) & (2 ** 64 - 1)


def counter_key(seed, call, particle_global, t, stream, index, mutant=None):
    """The counter (four words) and key (two) of philox_draw.  seed, call: Python integers below 2^64; the rest broadcast (uint64 arrays)."""
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    gp, t, stream, index = _u64(particle_global), _u64(t), _u64(stream), _u64(index)
    if mutant == "pos_t_minus_1":
        t = np.where(stream == np.uint64(STREAM_POS), t - np.uint64(1), t)
    gp_hi = np.uint64(0) * gp if mutant == "particle_hi_dropped" else gp >> np.uint64(32)
    tf = np.uint64(0) * t if mutant == "t_dropped" else (t << np.uint64(8)) & _M32
    sf = np.uint64(0) * stream if mutant == "stream_dropped" else (stream << np.uint64(30)) & _M32
    call_hi = 0 if mutant == "call_hi_dropped" else call >> 32
    seed_hi = 0 if mutant == "seed_hi_dropped" else seed >> 32
    c = (gp & _M32, gp_hi ^ sf ^ tf, index & _M32, np.uint64(call & 0xFFFFFFFF))
    k = (np.uint64((seed & 0xFFFFFFFF) ^ call_hi), np.uint64(seed_hi))
    return c, k


def draw(seed, call, particle_global, t, stream, index, mutant=None):
    c, k = counter_key(seed, call, particle_global, t, stream, index, mutant)
    if mutant == "rounds9":
        return philox4x32_10(c, k, rounds=9)
    if mutant == "swapped_multipliers":
        return philox4x32_10(c, k, m0=M1, m1=M0)
    if mutant == "no_key_bump":
        return philox4x32_10(c, k, bump=False)
    return philox4x32_10(c, k)


def uniform_numerators(words, mutant=None):
    """(j1, j2): the odd integers with u1 = j1 2^-53 and u2 = j2 2^-53, i.e. j = 2 (52-bit integer) + 1, as uint64."""
    x, y, z, w = words
    if mutant == "uniform32":  # the low 20 bits never filled
        a, b = x << np.uint64(20), z << np.uint64(20)
    else:
        a, b = (x << np.uint64(20)) | (y >> np.uint64(12)), (z << np.uint64(20)) | (w >> np.uint64(12))
    return (a << np.uint64(1)) | np.uint64(1), (b << np.uint64(1)) | np.uint64(1)


def normal_of_words(words, mutant=None):
    """Box-Muller in numpy double, as philox_normal forms it: the parity tier's evaluation."""
    j1, j2 = uniform_numerators(words, mutant)
    u1, u2 = j1.astype(np.float64) * 2.0 ** -53, j2.astype(np.float64) * 2.0 ** -53  # exact: j < 2^53
    r = np.sqrt(-2.0 * np.log(u1))
    return r * (np.sin(2.0 * np.pi * u2) if mutant == "sin_for_cos" else _cospi2(j2, np.float64))


def _reduce_cospi(j2):
    """cos(pi x) for x = 2 u2 = j2 2^-52 (j2 odd, below 2^53), reduced exactly in integers: returns (sign, use_sin, n) with
    cos(pi x) = sign * (sin if use_sin else cos)(pi n 2^-52) and 0 <= n 2^-52 <= 1/4.  x is never a multiple of 1/2 (j2 is odd)."""
    one = np.uint64(1) << np.uint64(52)
    j = np.where(j2 > one, (one << np.uint64(1)) - j2, j2)  # cos(pi (2 - x)) = cos(pi x): x in (0, 1)
    half = one >> np.uint64(1)
    sign = np.where(j > half, -1.0, 1.0)
    j = np.where(j > half, one - j, j)  # cos(pi x) = -cos(pi (1 - x)): x in (0, 1/2)
    quarter = half >> np.uint64(1)
    use_sin = j > quarter
    n = np.where(use_sin, half - j, j)  # cos(pi x) = sin(pi (1/2 - x))
    return sign, use_sin, n


_PI_LD = np.longdouble("3.14159265358979323846264338327950288419716939937510")


def _cospi2(j2, dtype):
    sign, use_sin, n = _reduce_cospi(j2)
    pi = _PI_LD if dtype is np.longdouble else np.pi
    a = n.astype(dtype) * dtype(2.0) ** -52 * pi
    return sign.astype(dtype) * np.where(use_sin, np.sin(a), np.cos(a))


def have_longdouble():
    """np.longdouble has the 64-bit significand of the x87 format (or more)."""
    return np.finfo(np.longdouble).nmant >= 63


def normal_hp_of_words(words):
    """The same formula at a 64-bit significand (np.longdouble): log and sqrt of the exact u1, cospi of the exactly reduced argument.  Its error
    is a few 2^-64 relative -- 2^-10 of a double's ulp.  Returns longdouble."""
    assert have_longdouble(), "np.longdouble is a double here: use normal_mp_of_words over a subset"
    j1, j2 = uniform_numerators(words)
    u1 = j1.astype(np.longdouble) * np.longdouble(2.0) ** -53
    return np.sqrt(np.longdouble(-2.0) * np.log(u1)) * _cospi2(j2, np.longdouble)


def normal_mp_of_words(words, dps=40):
    """The same with mpmath (arbitrary precision), element by element: for a subset, or where longdouble is a double.  Returns a list of mpf."""
    import mpmath

    j1, j2 = uniform_numerators(words)
    out = []
    with mpmath.workdps(dps):
        for a, b in zip(np.ravel(j1), np.ravel(j2)):
            u1, x = mpmath.mpf(int(a)) / 2 ** 53, mpmath.mpf(int(b)) / 2 ** 52
            out.append(mpmath.sqrt(-2 * mpmath.log(u1)) * mpmath.cospi(x))
    return out


def ulps(got, want_hp):
    """|got - want| in units of the double-precision ulp of ``want`` (want: longdouble)."""
    w64 = want_hp.astype(np.float64)
    return (np.abs(np.asarray(got).astype(np.longdouble) - want_hp) / np.spacing(np.abs(w64)).astype(np.longdouble)).astype(np.float64)


def normal(seed, call, particle_global, t, stream, index, mutant=None):
    return normal_of_words(draw(seed, call, particle_global, t, stream, index, mutant), mutant)


def normal_hp(seed, call, particle_global, t, stream, index):
    return normal_hp_of_words(draw(seed, call, particle_global, t, stream, index))


def drop_threshold(p):
    """floor(p 2^32) saturated at 0xFFFFFFFF, exactly: p 2^32 only changes the double's exponent."""
    f = Fraction(float(p)) * 2 ** 32
    return min(f.numerator // f.denominator, 0xFFFFFFFF)


def keep(seed, call, particle_global, t, b, p, mutant=None):
    """Keep decision of basis function / hidden unit ``b``: bool, broadcast."""
    b = _u64(b)
    idx = b if mutant == "keep_index_b" else b >> np.uint64(2)
    x, y, z, w = draw(seed, call, particle_global, t, STREAM_MASK, idx, mutant)
    order = (y, z, w, x) if mutant == "keep_word_order" else (x, y, z, w)
    sel = b & np.uint64(3)
    v = np.where(sel == 0, order[0], np.where(sel == 1, order[1], np.where(sel == 2, order[2], order[3])))
    thr = np.uint64(drop_threshold(p))
    return v > thr if mutant == "keep_gt" else v >= thr


# ---- tables in the oracle's buffer layouts ----------------------------------------------------------------------------------------------------------
def _grid(T0, T1, M, n, offset):
    t = np.arange(T0, T1, dtype=np.uint64)[:, None, None]
    m = (np.arange(M, dtype=np.uint64) + np.uint64(offset))[None, :, None]
    return t, m, np.arange(n, dtype=np.uint64)[None, None, :]


def eps_table(seed, call, T, M, G, offset=0, mutant=None, hp=False, t0=0):
    """[T - 1, M, G]: row t is what step t0 + t draws on stream 0."""
    t, m, g = _grid(t0, t0 + T - 1, M, G, offset)
    if hp:
        return normal_hp(seed, call, m, t, STREAM_EPS, g)
    return normal(seed, call, m, t, STREAM_EPS, g, mutant)


def mask_table(seed, call, T, M, B, p, offset=0, mutant=None):
    """[T, M, B] bool: the RBF policies' basis functions, or the MLP's H hidden units with layer 0's first (a block of four may span two layers)."""
    t, m, b = _grid(0, T, M, B, offset)
    return keep(seed, call, m, t, b, p, mutant)


def pos_table(seed, call, T, M, n, offset=0, mutant=None):
    """[T - 1, M, n]: row t - 1 is what step t draws on stream 2."""
    t, m, i = _grid(1, T, M, n, offset)
    return normal(seed, call, m, t, STREAM_POS, i, mutant)
