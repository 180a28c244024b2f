"""csrc/rtx_libm.h (the device's acosf / atanf / atan2f / expf / log2f) bit-for-bit against the host libm.
CPU part: the header compiled for the host, sampled here (the exhaustive 2^32 sweep is
tests/native/libm_check.c with stride 1: ~10 s per function on 8 cores, all five pass), and PORT == REF of tests/native/libm_ref.c on the
input sets of tests/libmset.py, the ones tests/test_gpu_libm_sweep.py puts through the device build.  GPU part: the device code."""
import os
import subprocess

import numpy as np
import pytest

import libmset
from util import REPO


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("libm") / "libm_check")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(REPO, "tests", "native", "libm_check.c"), "-lm", "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def host_ref(tmp_path_factory):
    return libmset.HostRef(tmp_path_factory.mktemp("libm_ref"))


@pytest.mark.parametrize("fn,arg", [("acosf", 13), ("atanf", 13), ("atan2f", 30000000), ("expf", 7), ("log2f", 7)])
def test_libm_ports_match_host_libm(checker, fn, arg):
    # acosf / atanf: every 13th of ALL 2^32 bit patterns (330 M values each); stride 1 is the exhaustive sweep quoted in DESIGN.md §3
    out = subprocess.run([checker, fn, str(arg)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


@pytest.mark.parametrize("fn", libmset.PORTED, ids=[libmset.NAMES[f] for f in libmset.PORTED])
def test_host_port_equals_the_reference_on_the_device_sweep_sets(host_ref, fn):
    """PORT (csrc/rtx_libm.h built for the host) == REF (the host libm) on exactly the sets the device build is swept on: the reference is
    consistent with the algorithms on the chosen inputs, and where a machine's libm differs this test says so, not the GPU one."""
    sets = {k: (v, None) for k, v in libmset.unary_sets(fn).items()} if fn != libmset.ATAN2F else libmset.pair_sets()
    assert sets
    for name, (a, b) in sets.items():
        ref, port = host_ref.ref(fn, a, b), host_ref.port(fn, a, b)
        bad = libmset.differing(port, ref)
        assert bad.size == 0, libmset.report(fn, name, bad, a, b, {"REF": ref, "PORT": port})


def test_sweep_sets_reach_what_they_are_built_for():
    """The sets are the test: their sizes, and that the atan2f pairs reach both k cut-offs, the x == 1 branch and quotients that underflow."""
    u32 = np.uint32
    lat = libmset.lattice()
    assert lat.size == 32768 == np.unique(lat >> u32(23)).size * 64 and {0x00000000, 0x80000000, 0x00000001, 0x7f800000, 0xff800000, 0x7f800001, 0x7fc00000} <= set(lat.tolist())
    assert libmset.stride().size == (1 << 32) // 509 + 1
    for fn in libmset.UNARY:
        sets = libmset.unary_sets(fn)
        assert all(0 < v.size <= 1 << 24 and v.dtype == u32 for v in sets.values()), fn
        for c in libmset.EDGES[fn]:
            assert {c - 2048, c, c + 2048, (c - 2048) | 0x80000000} <= set(sets["edges"].tolist()), (fn, hex(c))
    assert libmset.unary_sets(libmset.LOG2F)["table boundaries"].size == 5 * 16 * 129
    assert {libmset._hexf(v) for v in ("0x1.0p-1", "-0x1.8p0", "0x1.0p23", "0x1.fffffep30", "0x1.0p31", "0x1.000002p31")} <= set(libmset.rounding_values().tolist())
    pairs = libmset.pair_sets()
    assert pairs["pair lattice"][0].size == 6553600 and pairs["libm_check kinds"][0].size == 2000000
    for name, (y, x) in pairs.items():
        assert y.size == x.size <= 1 << 24, name
    y, x = (np.concatenate([p[i] for p in pairs.values()]) for i in (0, 1))
    iy, ix = (y & u32(0x7fffffff)).astype(np.int64), (x & u32(0x7fffffff)).astype(np.int64)
    live = (iy > 0) & (ix > 0) & (iy < 0x7f800000) & (ix < 0x7f800000) & (x != u32(0x3f800000))
    k = (iy - ix) >> 23
    with np.errstate(all="ignore"):
        q = np.abs(y.view(np.float32) / x.view(np.float32))
    neg = (x >> u32(31)) == 1
    for what, mask in (("k > 60", k > 60), ("k == 60", k == 60), ("k < -60, x < 0", (k < -60) & neg), ("k == -60, x < 0", (k == -60) & neg),
                       ("k < -60, x > 0", (k < -60) & ~neg), ("subnormal quotient", (q > 0) & (q < np.float32(2.0 ** -126))),
                       ("quotient rounds to zero", (q == 0) & (k > -200))):
        assert (live & mask).sum() >= 1000, what
    assert (x == u32(0x3f800000)).sum() >= 32768


@pytest.mark.gpu
def test_device_libm_matches_host(host_ref):
    import ctypes as C
    import util
    from pyrtx import api
    sc, _ = util.load_golden("cube")
    r = api.Renderer(sc)
    rng = np.random.RandomState(7)
    libm = C.CDLL("libm.so.6")
    libm.acosf.restype = C.c_float; libm.acosf.argtypes = [C.c_float]
    libm.atan2f.restype = C.c_float; libm.atan2f.argtypes = [C.c_float, C.c_float]
    x = np.concatenate([rng.uniform(-1, 1, 200000), np.array([1.0, -1.0, 0.0, 0.5, -0.5, 1e-9, 1.0000001, np.nan])]).astype(np.float32)
    dev = r.debug_libm(0, x)
    host = np.array([libm.acosf(float(v)) for v in x], np.float32)
    assert np.array_equal(dev.view(np.uint32)[~np.isnan(host)], host.view(np.uint32)[~np.isnan(host)]) and np.all(np.isnan(dev[np.isnan(host)]))
    y = rng.uniform(-2, 2, 200000).astype(np.float32); xx = rng.uniform(-2, 2, 200000).astype(np.float32)
    dev = r.debug_libm(1, y, xx)
    host = np.array([libm.atan2f(float(a), float(b)) for a, b in zip(y, xx)], np.float32)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    # expf / log2f: glibc's own table-driven algorithms incl. its fused multiply-adds -> the host's bits, specials included
    libm.expf.restype = C.c_float; libm.expf.argtypes = [C.c_float]
    libm.log2f.restype = C.c_float; libm.log2f.argtypes = [C.c_float]
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 88.7, 88.8, -103.2, -103.5, -104.0, -200.0, 1e-45, 1e-40, 1.0, -1.0, 3.4e38], np.float32)
    v = np.concatenate([rng.uniform(-110, 90, 200000).astype(np.float32), (rng.uniform(-1, 1, 100000) * 1e-3).astype(np.float32),
                        rng.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32), special])
    for fn_id, fn in ((2, libm.expf), (3, libm.log2f)):
        d = r.debug_libm(fn_id, v); h = np.array([fn(float(a)) for a in v], np.float32)
        ok = (d.view(np.uint32) == h.view(np.uint32)) | (np.isnan(d) & np.isnan(h))
        assert ok.all(), (fn_id, v[~ok][:5], d[~ok][:5], h[~ok][:5])
    # cvtss2si emulation incl. the out-of-range "indefinite" value
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3e9, -3e9, np.nan, 2147483520.0, 1e-3], np.float32)
    dev = r.debug_libm(5, v)
    assert dev.tolist()[:7] == [0.0, 2.0, 2.0, -0.0, -2.0, -2147483648.0, -2147483648.0]
    ref = host_ref.ref(libmset.F2I_RN, v.view(np.uint32))                  # cvtss2si itself: NaN -> indefinite, 2147483520 and 1e-3 exact
    assert ref.view(np.float32).tolist()[7:] == [-2147483648.0, 2147483520.0, 0.0]
    assert np.array_equal(dev.view(np.uint32), ref), (dev.tolist(), ref.view(np.float32).tolist())
