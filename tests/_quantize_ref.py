"""What the quantize tests lean on (include/bsmm_quant.h), independent of blocksparse_amd/quantize.py: the rounding as a per-element loop in
exact rational arithmetic (``fractions.Fraction`` on ``math.frexp``), per-element loops for the statistics and the exponent rule, and the
data set both tiers run: every halfway point of three small formats with its fp32 neighbours, the edges of the ranges and the specials."""
import math
from fractions import Fraction

import numpy as np

FORMATS = [(4, 3, 8), (5, 2, 16), (2, 1, 2)]          # (ebits, fbits, emax): the halfway points of these are in the data set


def fmt(ebits, fbits, emax, denorm):
    """(e_hi, s_min, e_lo, max_float as a Fraction), from the text of the header."""
    nexp = 254 if ebits == 8 else 2 ** ebits - 1
    e_hi = min(max(emax, nexp - 127), 127)
    s_min = max(e_hi - nexp + 1 - (fbits if denorm else 0), -125)
    e_lo = s_min + (fbits if denorm else 0)
    return e_hi, s_min, e_lo, (2 - Fraction(1, 2 ** fbits)) * Fraction(2) ** e_hi


def q_loop(x, ebits, fbits, emax, denorm, mode, r=0):
    """Q of one float32 value -> (result as a Python float, lo, frac)."""
    x = float(np.float32(x))
    if math.isnan(x):
        return x, None, None
    neg = math.copysign(1.0, x) < 0
    signed = lambda v: -float(v) if neg else float(v)
    e_hi, s_min, e_lo, maxf = fmt(ebits, fbits, emax, denorm)
    if math.isinf(x) or Fraction(abs(x)) >= maxf:
        return signed(maxf), None, None
    ax = Fraction(abs(x))
    m, ex = math.frexp(abs(x))                           # |x| = m * 2^ex, 0.5 <= m < 1
    e = ex - 1 if ax != 0 and ex - 1 >= -126 else -127   # zero and the fp32 subnormals count as -127
    u = Fraction(2) ** (max(e, e_lo) - fbits)
    t = ax / u
    lo = t.numerator // t.denominator
    frac = t - lo
    if mode == 0:
        up = frac >= Fraction(1, 2)
    elif mode == 1:
        up = frac > Fraction(1, 2) or (frac == Fraction(1, 2) and lo % 2 == 1)
    else:
        f32 = frac * 2 ** 32
        up = int(r) < f32.numerator // f32.denominator
    res = (lo + (1 if up else 0)) * u
    if res > maxf:
        res = maxf
    if not denorm and res < Fraction(2) ** e_lo:
        res = Fraction(0)
    return signed(res), lo, frac


def q_loop_array(x, ebits, fbits, emax, denorm, mode, r=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    r = np.zeros(x.size, dtype=np.uint32) if r is None else r
    return np.array([q_loop(v, ebits, fbits, emax, denorm, mode, w)[0] for v, w in zip(x, r)], dtype=np.float32)


def grid(ebits, fbits, emax, denorm=True):
    """The non-negative grid points as Fractions, ascending."""
    e_hi, s_min, e_lo, _ = fmt(ebits, fbits, emax, denorm)
    pts = [Fraction(0)]
    if denorm:
        pts += [m * Fraction(2) ** s_min for m in range(1, 2 ** fbits)]
    for e in range(e_lo, e_hi + 1):
        pts += [m * Fraction(2) ** (e - fbits) for m in range(2 ** fbits, 2 ** (fbits + 1))]
    return pts


def halfway_points(ebits, fbits, emax):
    g = grid(ebits, fbits, emax)
    return np.array([float((a + b) / 2) for a, b in zip(g[:-1], g[1:])], dtype=np.float32)


def dataset(seed=5):
    """float32 [a few thousand]: the halfway points of FORMATS and their fp32 neighbours, the neighbours of every max_float and of half the
    smallest step, +-0, +-inf, NaN, fp32 subnormals, and log-uniform random magnitudes; every value with both signs."""
    rng = np.random.default_rng(seed)
    vals = []
    for ebits, fbits, emax in FORMATS:
        h = halfway_points(ebits, fbits, emax)
        assert all(Fraction(float(v)) == (a + b) / 2 for v, a, b in zip(h, grid(ebits, fbits, emax)[:-1], grid(ebits, fbits, emax)[1:]))
        e_hi, s_min, e_lo, maxf = fmt(ebits, fbits, emax, True)
        edges = np.array([float(maxf), 2.0 ** (s_min - 1), 2.0 ** e_lo, 2.0 ** (e_lo - fbits - 1), 2.0 ** (fmt(ebits, fbits, emax, False)[2])], dtype=np.float32)
        for c in (h, edges):
            vals += [c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(np.inf))]
    vals.append(np.array([0.0, np.inf, np.nan, 1e-45, 3e-42, 1.1754942e-38, 1.17549435e-38, 2.0 ** -125, 2.0 ** -126, 3.4028235e38, 1.0, 65504.0], dtype=np.float32))
    vals.append((rng.normal(size=1500) * np.exp(rng.uniform(-16.0, 8.0, 1500))).astype(np.float32))
    v = np.concatenate(vals)
    return np.concatenate([v, -v])


def to_bf16(x):
    """float32 values truncated to what bf16 holds (the halfway points of FORMATS survive: they need at most 4 fraction bits)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def same_bits(got, want):
    """Bit for bit; a NaN must be a NaN where one is expected (the storage type's conversion may set its quiet bit)."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def stats_loop(x, sat_val, ftz_val):
    """The eight statistics, element by element in Python floats (float64)."""
    n = s1 = s2 = sat = ftz = nonf = 0
    vmax = 0.0
    for v in np.asarray(x, dtype=np.float64).reshape(-1):
        n += 1
        a = abs(float(v))
        if math.isnan(a) or math.isinf(a):
            nonf += 1
            sat += 1
            continue
        s1 += a
        s2 += a * a
        vmax = max(vmax, a)
        sat += a >= sat_val
        ftz += a != 0 and a < ftz_val
    mean = s1 / n
    return [mean, math.sqrt(max(s2 / n - mean * mean, 0.0)), vmax, sat / n, ftz / n, nonf, n, 0.0]


def emax_loop(x, ebits, bias_pad, mode, stdv_mul, emax):
    """The exponent rule of bsmm_quant_update_emax and the float64 value of the deciding quantity M."""
    s = stats_loop(x, 0.0, 0.0)
    M = s[0] + stdv_mul * s[1] if mode else s[2]
    if M == 0 or s[5] == s[6]:
        return emax, M
    nexp = 254 if ebits == 8 else 2 ** ebits - 1
    e = math.frexp(float(np.float32(M)))[1] - 1
    return min(max(e + bias_pad, nexp - 127), 127), M


def clear_of_a_power_of_two(M):
    """M is not within 2^-10 relative of a power of two (the float32 conversion of a float64 M cannot change its exponent then)."""
    m = math.frexp(M)[0] * 2                              # 1 <= m < 2
    return m - 1 > 2.0 ** -10 and 2 - m > 2.0 ** -10
