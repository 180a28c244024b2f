"""Ray queries (include/rtx.h rtx_query_closest / rtx_query_occluded): the exported symbols, the ctypes mirror of rtx_query_buffers, the
channel bits and the Python-side argument checks, without a GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from util import REPO
from test_views_cpu import _offline_renderer

NEW = ("rtx_query_closest", "rtx_query_occluded")


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


def test_query_functions_are_declared_exported_and_bound(api):
    header = open(f"{REPO}/include/rtx.h").read()
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+1\b", header)
    lib = api.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), f"{name} is not exported by the library"
        assert name in api.EXPORTS and name in api.QUERY_EXPORTS, name
        assert getattr(lib, name).argtypes, name
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.rtx_query_closest.argtypes[2] is C.c_int64 and lib.rtx_query_occluded.argtypes[2] is C.c_int64      # n is int64_t
    assert lib.rtx_abi_version() == 1


def test_query_buffers_mirror_the_header(api):
    header = open(f"{REPO}/include/rtx.h").read()
    m = re.search(r"typedef\s+struct\s+rtx_query_buffers\s*\{(.*?)\}\s*rtx_query_buffers\s*;", header, re.S)
    assert m, "rtx_query_buffers is not declared"
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    declared = re.findall(r"(float|int32_t)\s*\*\s*(\w+)\s*;", fields)
    assert [n for _, n in declared] == [n for n, _ in api.RtxQueryBuffers._fields_] == list(api.QUERY_CHANNELS)
    assert C.sizeof(api.RtxQueryBuffers) == 7 * C.sizeof(C.c_void_p)
    for (ctype, name) in declared:                                      # float channels are float32 arrays, id channels int32
        assert api.QUERY_CHANNELS[name][1] == (np.float32 if ctype == "float" else np.int32), name
    # the C side's sizeof and the chunk size: the header compiled by the host compiler
    src = (f'#include "{REPO}/include/rtx.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%zu %d %d", sizeof(rtx_query_buffers), (int)RTX_QUERY_CHUNK_RAYS, (int)RTX_QUERY_ALL); return 0; }\n')
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["cc", "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
        out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout
    assert out == f"{7 * C.sizeof(C.c_void_p)} {api.RTX_QUERY_CHUNK_RAYS} {api.RTX_QUERY_ALL}"
    assert api.RTX_QUERY_CHUNK_RAYS == 1 << 20


def test_query_bits_are_the_aov_bits_of_the_same_name(api):
    from pyrtx import ctypes_structs as cs
    header = re.sub(r"/\*.*?\*/", "", open(f"{REPO}/include/rtx.h").read(), flags=re.S)
    aov_of = {"distance": "depth"}                                       # RayHit::distance is the AOV path's depth channel
    total = 0
    for name, (bit, dtype, k) in api.QUERY_CHANNELS.items():
        assert bit == getattr(api, "RTX_QUERY_" + name.upper())
        assert int(re.search(r"\bRTX_QUERY_" + name.upper() + r"\s*=\s*(\d+)", header).group(1)) == bit
        abit, adtype, ak = cs.AOV_CHANNELS[aov_of.get(name, name)]
        assert (bit, dtype, k) == (abit, adtype, ak), name
        total |= bit
    assert total == api.RTX_QUERY_ALL == cs.RTX_AOV_ALL & ~cs.RTX_AOV_ALBEDO == 247
    assert int(re.search(r"\bRTX_QUERY_ALL\s*=\s*(\d+)", header).group(1)) == 247
    assert api.query_names(api.RTX_QUERY_ALL) == tuple(api.QUERY_CHANNELS)
    assert api.query_names(("triangle_id", "distance")) == ("distance", "triangle_id")
    for bad in (0, 8, 256, ()):
        with pytest.raises(ValueError):
            api.query_names(bad)


def test_queries_validate_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api)                                          # ctx and lib are None: a call that got through would raise AttributeError
    f32, i32 = torch.float32, torch.int32
    ok = torch.zeros((8, 6), dtype=f32)
    closest = [
        (dict(rays=np.zeros((8, 6), np.float32)), TypeError, "torch.Tensor"),         # a numpy array instead of a tensor
        (dict(rays=ok.double()), TypeError, "float32"),                               # wrong dtype
        (dict(rays=torch.zeros((8, 5), dtype=f32)), ValueError, r"\(n, 6\)"),          # (n, 5) rays
        (dict(rays=torch.zeros((8, 12), dtype=f32)[:, ::2]), ValueError, "contiguous"),
        (dict(rays=ok), ValueError, "cuda:0"),                                        # a CPU tensor
        (dict(rays=ok, channels=("distance", "albedo")), ValueError, "unknown query channel"),
        (dict(rays=ok, channels=()), ValueError, "at least one"),
        (dict(rays=ok, channels=("distance",), out={"distance": torch.zeros((7,), dtype=f32)}), ValueError, r"shape \(8,\)"),      # out of the wrong shape
        (dict(rays=ok, channels=("normal",), out={"normal": torch.zeros((8,), dtype=f32)}), ValueError, r"shape \(8, 3\)"),
        (dict(rays=ok, channels=("object_id",), out={"object_id": torch.zeros((8,), dtype=f32)}), TypeError, "int32"),             # out of the wrong dtype
        (dict(rays=ok, channels=("distance",), out={"uv": torch.zeros((8, 2), dtype=f32)}), ValueError, "not requested"),
        (dict(rays=ok, channels=("distance",), out={"distance": torch.zeros((8,), dtype=f32)}), ValueError, "cuda:0"),            # all well but the device
        (dict(rays=0x7f0000000000), ValueError, "n is needed"),                       # raw pointers without n
        (dict(rays=0x7f0000000000, n=8), ValueError, "every requested channel"),      # ... and without an address for the channel
        (dict(rays=ok, n=9), ValueError, "n must be"),                                # more rays than the tensor holds
        (dict(rays=ok, count_work=True), ValueError, "flags"),                        # a render flag that is not a query's
    ]
    for kw, exc, what in closest:
        with pytest.raises(exc, match=what):
            r.query_closest(**kw)
    seg = torch.zeros((8, 7), dtype=f32)
    occluded = [
        (dict(segments=np.zeros((8, 7), np.float32)), TypeError, "torch.Tensor"),
        (dict(segments=seg.half()), TypeError, "float32"),
        (dict(segments=ok), ValueError, r"\(n, 7\)"),                                 # (n, 6): no max distance
        (dict(segments=torch.zeros((8, 14), dtype=f32)[:, ::2]), ValueError, "contiguous"),
        (dict(segments=seg), ValueError, "cuda:0"),                                   # a CPU tensor
        (dict(segments=seg, out=torch.zeros((8,), dtype=f32)), TypeError, "int32"),
        (dict(segments=seg, out=torch.zeros((9,), dtype=i32)), ValueError, r"shape \(8,\)"),
        (dict(segments=0x7f0000000000), ValueError, "n is needed"),                   # raw pointer without n
        (dict(segments=0x7f0000000000, n=8), ValueError, "address of the result"),
        (dict(segments=seg, serial=True), ValueError, "flags"),
    ]
    for kw, exc, what in occluded:
        with pytest.raises(exc, match=what):
            r.query_occluded(**kw)
