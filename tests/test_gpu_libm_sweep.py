"""The DEVICE builds of csrc/rtx_libm.h, of the two x86 roundings and of pow2_128 (csrc/rtx_math.h), swept against the host.

tests/native/libm_check.c sweeps the header exhaustively, but as gcc compiles it for the host.  What the kernels run is another compiler's
code for gfx950, and it is the host's bit for bit only under four flags of csrc/Makefile: -ffp-contract=off, -fno-fast-math,
-fhip-fp32-correctly-rounded-divide-sqrt and -fno-gpu-flush-denormals-to-zero.  Here every hook id of rtx_debug_libm runs on the input sets of
tests/libmset.py (every exponent, the subnormals, the specials, +-2048 patterns around every branch constant, the ranges where results are
subnormal, the ties of the roundings, atan2f pairs whose quotient underflows) and is compared with REF of tests/native/libm_ref.c: the host
libm, 1.0f / sqrtf, the SSE conversion instructions, seven squarings.  Equal bits or both NaN (x86 and gfx950 make different default NaNs);
the sign of zero counts; no input is left out and there is no tolerance.  On a difference the message shows the device's, REF's and PORT's
bits (PORT = the header compiled for the host): PORT != REF means the host libm moved, PORT == REF means the device build diverged.
tests/test_libm.py holds the CPU half: PORT == REF on the same sets.
Three wrong builds, tried on an MI355X and not kept, each with one flag reversed (inputs that differ, lattice set unless named):
  denormals flushed        expf 25, log2f 63, 1 / sqrtf 126 (inf for every subnormal), pow2_128 36, atan2f 146 066 of the pair lattice (NaN or a
                           zero quotient); acosf, atanf and both roundings unharmed
  contraction allowed      acosf 1, atanf 5, atan2f 2 256 of the libm_check kinds, all by one ulp; the fp64 routines unharmed
  fast divide and sqrt     acosf 6, atanf 21, 1 / sqrtf 3 257, atan2f 398 756 of the pair lattice, by one ulp"""
import numpy as np
import pytest

import libmset
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_ref(tmp_path_factory):
    return libmset.HostRef(tmp_path_factory.mktemp("libm_ref"))


@pytest.fixture(scope="module")
def renderer():
    from pyrtx import api
    sc, _ = util.load_golden("cube")
    r = api.Renderer(sc)
    yield r
    r.close()


def sweep(r, host_ref, fn, sets):
    for name, (a, b) in sets.items():
        dev = r.debug_libm(fn, a.view(np.float32), None if b is None else b.view(np.float32)).view(np.uint32)
        ref = host_ref.ref(fn, a, b)
        bad = libmset.differing(dev, ref)
        print(f"{libmset.NAMES[fn]}, set '{name}': {a.size} inputs, {bad.size} differ")
        assert bad.size == 0, libmset.report(fn, name, bad, a, b, {"device": dev, "REF": ref, "PORT": host_ref.port(fn, a, b)})


@pytest.mark.parametrize("fn", libmset.UNARY, ids=[libmset.NAMES[f] for f in libmset.UNARY])
def test_device_unary_function_equals_the_host_reference(renderer, host_ref, fn):
    sweep(renderer, host_ref, fn, {k: (v, None) for k, v in libmset.unary_sets(fn).items()})


def test_device_atan2f_equals_the_host_reference(renderer, host_ref):
    sweep(renderer, host_ref, libmset.ATAN2F, libmset.pair_sets())
