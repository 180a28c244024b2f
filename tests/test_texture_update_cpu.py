"""Device-side texture and sky update (include/rtx.h rtx_alloc_texture / rtx_update_texture / rtx_read_texture / rtx_update_sky) without a
GPU: the exported symbols and their bindings, the format constants, the pass plan on the CPU (csrc/texmip_check.cpp under the host
sanitizers) and the Python-side argument checks."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from util import REPO
from test_views_cpu import _offline_renderer

NEW = ("rtx_alloc_texture", "rtx_update_texture", "rtx_read_texture", "rtx_update_sky")


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


def test_texture_functions_are_declared_exported_and_bound(api):
    header = open(f"{REPO}/include/rtx.h").read()
    lib = api.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), f"{name} is not exported by the library"
        assert name in api.EXPORTS and name in api.TEXTURE_EXPORTS, name
        assert getattr(lib, name).argtypes, name
        assert getattr(lib, name).restype is C.c_int, name
    assert tuple(api.TEXTURE_EXPORTS) == NEW
    assert len(lib.rtx_alloc_texture.argtypes) == 5 and len(lib.rtx_update_texture.argtypes) == 4 and len(lib.rtx_update_sky.argtypes) == 3
    assert lib.rtx_read_texture.argtypes[4] is C.c_int64                  # capacity_texels is int64_t
    assert lib.rtx_abi_version() == 1


def test_format_constants_match_the_header(api):
    src = (f'#include "{REPO}/include/rtx.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%d %d %d", (int)RTX_TEXELS_RGB_F32, (int)RTX_TEXELS_RGBA8_SRGB, (int)RTX_MAX_MIP_LEVELS); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["cc", "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
        out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout
    from pyrtx import ctypes_structs as cs
    assert out == f"{api.RTX_TEXELS_RGB_F32} {api.RTX_TEXELS_RGBA8_SRGB} {cs.RTX_MAX_MIP_LEVELS}" == "0 1 16"


def test_pass_plan_on_the_cpu_under_the_sanitizers():
    """csrc/texmip_check.cpp: every pass and tile of the plan, for every P and every shape of the GPU tests, against the plain loop."""
    out = subprocess.run(["make", "-B", "-C", os.path.join(REPO, "cpu-raytracer_amd", "csrc"), "texmip_check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "texmip_check: ok" in out.stdout


def test_update_methods_validate_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api, 64, 48)
    r._texture_shape = lambda texture_id: (16, 32) if texture_id == 3 else None      # what the library would answer after alloc_texture(3, 32, 16)
    f32 = torch.zeros((16, 32, 3), dtype=torch.float32)
    u8 = torch.zeros((16, 32, 4), dtype=torch.uint8)
    texture_cases = [
        (f32.double(), "float32"),                                                        # wrong dtype
        (f32.to(torch.int32), "float32"),
        (torch.zeros((16, 32, 4), dtype=torch.float32), "shape"),                         # [H,W,4] float32
        (torch.zeros((16, 32, 3), dtype=torch.uint8), "shape"),                           # [H,W,3] uint8
        (torch.zeros((16, 32), dtype=torch.float32), "shape"),
        (torch.zeros((32, 16, 3), dtype=torch.float32), "size of the texture"),           # not the allocated shape
        (torch.zeros((16, 16, 4), dtype=torch.uint8), "size of the texture"),
        (torch.zeros((16, 32, 6), dtype=torch.float32)[..., ::2], "contiguous"),
        (torch.zeros((16, 64, 4), dtype=torch.uint8)[:, ::2], "contiguous"),
        (f32, "cuda:0"),                                                                  # a CPU tensor
        (u8, "cuda:0"),
        (f32.numpy(), "torch.Tensor"),
    ]
    for t, match in texture_cases:
        with pytest.raises(ValueError, match=match):
            r.update_texture(3, t)
    with pytest.raises(ValueError, match="cuda:0"):
        r.update_texture(9, torch.zeros((5, 7, 3), dtype=torch.float32))                  # an id this Renderer never allocated: the library decides, after the other checks
    sky_cases = [
        (torch.zeros((8, 8, 3), dtype=torch.float64), "float32"),
        (torch.zeros((8, 8, 4), dtype=torch.uint8), "sky"),
        (torch.zeros((8, 4, 3), dtype=torch.float32), "sky"),
        (torch.zeros((8, 8, 4), dtype=torch.float32), "sky"),
        (torch.zeros((8, 8, 6), dtype=torch.float32)[..., ::2], "contiguous"),
        (torch.zeros((8, 8, 3), dtype=torch.float32), "cuda:0"),
    ]
    for t, match in sky_cases:
        with pytest.raises(ValueError, match=match):
            r.update_sky(t)
