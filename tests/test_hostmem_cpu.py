"""Who owns the device memory behind the C ABI, and what the scene a kernel receives names of it, is decided by host code alone
(cpu-raytracer_amd/csrc/rtx_hostmem.h): DevBuf, the staging ring, grow_keep, and the binding rule of the four scene tables (bind_tables /
replace_table: BLAS, materials, textures, sky).  No GPU test can make an allocation fail or see a freed table, so the rules are pinned by
csrc/hostmem_check.cpp, a stand-alone program over counting stand-ins for the HIP calls, built with the host compiler under
-fsanitize=address,undefined.  This test builds and runs it; nothing is loaded into Python and no GPU is needed."""
import os
import subprocess

import util

CSRC = os.path.join(util.REPO, "cpu-raytracer_amd", "csrc")


def test_hostmem_check_passes():
    out = subprocess.run(["make", "-B", "-C", CSRC, "hostmem_check"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "hostmem_check: ok" in out.stdout.splitlines(), out.stdout[-4000:]
    assert "FAILED" not in out.stdout
