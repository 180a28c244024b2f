"""Input sets for the device builds of csrc/rtx_libm.h, the two x86 roundings and pow2_128 (rtx_debug_libm's ids, include/rtx.h), and the
host reference they are compared with (tests/native/libm_ref.c).  Like rayset.py and sweepset.py: generated, seeded, deterministic; here as
bit patterns (uint32), since most of what matters is no number a generator of floats would draw.

Every unary function gets
  lattice   256 exponents x 2 signs x the mantissas {0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff} and 56 random ones = 32 768
            values: +-0, every subnormal scale, +-inf, quiet and signalling NaN payloads
  stride    every 509th of all 2^32 bit patterns (8 438 049 values)
  edges     +-2048 patterns around every constant its source compares against, both signs (EDGES, read off the header)
and its own sets on top (unary_sets).  atan2f gets four sets of pairs (pair_sets).  A set has at most 2^24 values: 64 MiB each way."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

u32 = np.uint32
ACOSF, ATAN2F, EXPF, LOG2F, ATANF, F2I_RN, RSQRT, F2I_TRUNC, POW2_128 = range(9)
NAMES = ["acosf", "atan2f", "expf", "log2f", "atanf", "f2i_rn_x86", "1.0f / sqrtf", "f2i_trunc_x86", "pow2_128"]
UNARY = (ACOSF, EXPF, LOG2F, ATANF, F2I_RN, RSQRT, F2I_TRUNC, POW2_128)
PORTED = (ACOSF, ATAN2F, EXPF, LOG2F, ATANF)           # what csrc/rtx_libm.h holds, so what libm_ref.c's PORT knows
SEED = 20240607
FIXED_MANTISSAS = (0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff)
PAIR_MANTISSAS = (0, 1, 0x7fffff, 0x400000, 0x2aaaab)


def fbits(x):
    """Bit pattern(s) of float32 value(s)."""
    return np.asarray(x, np.float32).view(u32)


def _hexf(s):
    return int(fbits(float.fromhex(s)))


# the constants each function's source compares its argument (or |argument|) against, as bit patterns of the magnitude
EDGES = {
    ACOSF: (0x3f800000, 0x3f000000, 0x32800000),
    ATANF: (0x4c000000, 0x3ee00000, 0x31000000, 0x3f980000, 0x3f300000, 0x401c0000, 0x7f800000),
    # abstop > 0x42a is |x| >= 0x42b00000, abstop > 0x7f7 is inf / NaN; then the overflow, underflow and may-underflow bounds
    EXPF: (0x42b00000, 0x7f800000, _hexf("0x1.62e42ep6"), _hexf("0x1.9fe368p6"), _hexf("0x1.9d1d9ep6")),
    LOG2F: (0x3f800000, 0x00800000, 0x7f800000),
    F2I_RN: (0x4f000000,),                                 # fabsf(x) < 2147483648.0f
    F2I_TRUNC: (0x4f000000,),
    RSQRT: (0x00800000, 0x7f800000),                       # no branch of ours: where sqrt and the division change regime
    POW2_128: (),
}


@functools.lru_cache(maxsize=None)
def lattice():
    rng = np.random.default_rng(SEED)
    man = np.concatenate([np.broadcast_to(np.array(FIXED_MANTISSAS, u32), (256, 2, 8)), rng.integers(0, 1 << 23, (256, 2, 56), dtype=u32)], axis=2)
    exp = (np.arange(256, dtype=u32) << u32(23))[:, None, None]
    sign = (np.arange(2, dtype=u32) << u32(31))[None, :, None]
    out = np.ascontiguousarray((sign | exp | man).reshape(-1))
    assert out.size == 32768
    return out


@functools.lru_cache(maxsize=None)
def stride():
    return np.arange(0, 1 << 32, 509, dtype=np.uint64).astype(u32)


def around(centres, radius, both_signs=True):
    """Every pattern within `radius` of each centre (clipped to magnitudes 0 .. 0x7fffffff), with the sign bit clear and set."""
    off = np.arange(-radius, radius + 1, dtype=np.int64)
    mag = (np.asarray(centres, np.int64)[:, None] + off[None, :]).reshape(-1)
    mag = np.unique(mag[(mag >= 0) & (mag <= 0x7fffffff)]).astype(u32)
    return np.concatenate([mag, mag | u32(0x80000000)]) if both_signs else mag


def span(lo, hi):
    """Every pattern lo .. hi, both ends included."""
    return np.arange(lo, hi + 1, dtype=np.uint64).astype(u32)


def _with_neighbours(values):
    v = np.asarray(values, np.float32)
    return fbits(np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]))


@functools.lru_cache(maxsize=None)
def rounding_values():
    """f2i_rn_x86 / f2i_trunc_x86: the ties k + 0.5 and their neighbours for k in -4096 .. 4096; +-2^23 and +-2^24 (the last fractions, the
    last odd integers) with neighbours; the greatest float below 2^31, 2^31 and the float after it, both signs; 3e9."""
    k = np.arange(-4096, 4097, dtype=np.float64) + 0.5
    big = np.array([2.0 ** 23, 2.0 ** 24], np.float64)
    lim = fbits(np.array([2147483520.0, 2147483648.0], np.float32))
    lim = np.concatenate([lim, lim[1:] + u32(1)])
    return np.concatenate([_with_neighbours(k), _with_neighbours(np.concatenate([big, -big])), lim, lim | u32(0x80000000), fbits([3e9, -3e9])])


@functools.lru_cache(maxsize=None)
def log2f_table_edges():
    """+-64 patterns around the 16 boundaries 0x3f330000 + (i << 19) between the table's intervals, in five binades: the lowest and highest
    normal ones, the boundary's own and two in between."""
    base = 0x3f330000 + (np.arange(16, dtype=np.int64) << 19)
    return np.concatenate([around(base + (e << 23), 64, both_signs=False) for e in (-125, -60, 0, 60, 127)])


def unary_sets(fn):
    """name -> uint32 bit patterns (one rtx_debug_libm call each)."""
    sets = {"lattice": lattice(), "stride": stride()}
    if EDGES[fn]:
        sets["edges"] = around(EDGES[fn], 2048)
    if fn == ACOSF:
        poles = span(0x3f7f0000, 0x3f800010)
        sets["poles"] = np.concatenate([poles, poles | u32(0x80000000)])
    elif fn == EXPF:                                        # every float in [-104.5, -87] and [88, 89]: all subnormal results, the overflow bound
        sets["subnormal results and overflow"] = np.concatenate([span(0xc2ae0000, 0xc2d10000), span(0x42b00000, 0x42b20000)])
        assert sets["subnormal results and overflow"].size == 2424834
    elif fn == LOG2F:
        sets["subnormals and the first binade"] = span(0, 0x00ffffff)
        sets["around 1"] = around([0x3f800000], 65536, both_signs=False)
        sets["table boundaries"] = log2f_table_edges()
    elif fn == RSQRT:
        sets["every seventh subnormal"] = np.arange(1, 0x00800000, 7, dtype=u32)
    elif fn in (F2I_RN, F2I_TRUNC):
        sets["ties and limits"] = rounding_values()
    elif fn == POW2_128:                                    # |x| <= 2: the results cross the subnormal range near 0.5 and overflow past 2
        sets = {k: v[(v & u32(0x7fffffff)) <= u32(0x40000000)] for k, v in sets.items()}
    return sets


@functools.lru_cache(maxsize=None)
def pair_sets():
    """name -> (y bits, x bits) for atan2f(y, x)."""
    rng = np.random.default_rng(SEED + 1)
    sets = {}
    # every case of the m switch, every zero / inf / NaN combination, both k cut-offs at every scale, every quotient that underflows
    one = ((np.arange(2, dtype=u32) << u32(31))[None, :, None] | (np.arange(256, dtype=u32) << u32(23))[:, None, None] | np.array(PAIR_MANTISSAS, u32)[None, None, :]).reshape(-1)
    sets["pair lattice"] = (np.repeat(one, one.size), np.tile(one, one.size))
    assert sets["pair lattice"][0].size == 6553600
    # the four kinds tests/native/libm_check.c draws: any bit patterns, the unit square, equal exponents, x = +-1
    n = 500000
    a, b = rng.integers(0, 1 << 32, (2, 4, n), dtype=np.uint64).astype(u32)
    unit = lambda v: fbits(v.view(np.int32).astype(np.float32) * np.float32(2.0 ** -31))
    same_exp = lambda v: (v & u32(0x807fffff)) | u32(0x3f000000)
    ys = [a[0], unit(a[1]), same_exp(a[2]), unit(a[3])]
    xs = [b[0], unit(b[1]), same_exp(b[2]), (b[3] & u32(0x80000000)) | u32(0x3f800000)]
    sets["libm_check kinds"] = (np.concatenate(ys), np.concatenate(xs))
    # x == 1 exactly: the branch that hands y to atanf unchanged
    sets["x == 1"] = (lattice(), np.full(lattice().size, 0x3f800000, u32))
    # k = (iy - ix) >> 23 on both sides of the two cut-offs (k > 60, k < -60), at every scale subnormals included, every sign pair
    ey, d = np.meshgrid(np.arange(255, dtype=np.int64), np.array([-62, -61, -60, -59, -58, 58, 59, 60, 61, 62], np.int64), indexing="ij")
    ex = ey - d
    ok = (ex >= 0) & (ex <= 254)
    ey, ex = ey[ok], ex[ok]
    reps, signs = 16, np.array([0, 0x80000000], u32)
    ey = np.repeat(ey, reps * 4); ex = np.repeat(ex, reps * 4)
    sy = np.tile(np.repeat(signs, 2), ey.size // 4); sx = np.tile(np.tile(signs, 2), ex.size // 4)
    my, mx = rng.integers(0, 1 << 23, (2, ey.size), dtype=u32)
    sets["exponent band"] = (sy | (ey.astype(u32) << u32(23)) | my, sx | (ex.astype(u32) << u32(23)) | mx)
    return {k: (np.ascontiguousarray(y), np.ascontiguousarray(x)) for k, (y, x) in sets.items()}


# ---- the host reference ---------------------------------------------------------------------------------------------------------------------
class HostRef:
    """tests/native/libm_ref.c, built into `directory` and loaded with ctypes: ref(fn, a, b) -> REF bits, port(fn, a, b) -> PORT bits or None."""

    def __init__(self, directory):
        repo = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
        so = os.path.join(str(directory), "libm_ref.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(repo, "tests", "native", "libm_ref.c"), "-lm"])
        self.lib = C.CDLL(so)
        for name in ("ref_unary", "port_unary"):
            getattr(self.lib, name).argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        for name in ("ref_binary", "port_binary"):
            getattr(self.lib, name).argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]

    def _run(self, which, fn, a, b):
        a = np.ascontiguousarray(a, u32)
        out = np.zeros(a.size, u32)
        if b is None:
            rc = getattr(self.lib, which + "_unary")(fn, a.ctypes.data, out.ctypes.data, a.size)
        else:
            b = np.ascontiguousarray(b, u32)
            assert b.size == a.size
            rc = getattr(self.lib, which + "_binary")(fn, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
        return out if rc == 0 else None

    def ref(self, fn, a, b=None):
        out = self._run("ref", fn, a, b)
        assert out is not None, fn
        return out

    def port(self, fn, a, b=None):
        return self._run("port", fn, a, b)


def is_nan(bits):
    return (np.asarray(bits, u32) & u32(0x7fffffff)) > u32(0x7f800000)


def differing(got, want):
    """Indices where the bits differ and not both are NaN.  The sign of zero counts."""
    return np.flatnonzero((got != want) & ~(is_nan(got) & is_nan(want)))


def report(fn, set_name, bad, a, b, columns):
    """The failure text: the function, how many differ, the first five inputs as hex with each column's bits (columns: name -> bits or None)."""
    lines = [f"{NAMES[fn]}, set '{set_name}': {bad.size} of {a.size} inputs differ"]
    for i in bad[:5]:
        arg = f"{a[i]:08x}" + ("" if b is None else f", {b[i]:08x}")
        lines.append(f"  {NAMES[fn]}({arg}): " + "  ".join(f"{k} {'n/a' if v is None else format(v[i], '08x')}" for k, v in columns.items()))
    return "\n".join(lines)
