"""Which kernels a render call launches is decided by plan_render (cpu-raytracer_amd/csrc/rtx_plan.h), a pure function of plain values with no
HIP in it.  Every traversal kernel produces the same bits, so no parity test can see a level handed to the wrong kernel: the rules and
their measured thresholds are pinned by csrc/plan_check.cpp, a stand-alone program built with the host compiler under
-fsanitize=address,undefined.  This test builds and runs it; nothing is loaded into Python and no GPU is needed."""
import os
import subprocess

import util

CSRC = os.path.join(util.REPO, "cpu-raytracer_amd", "csrc")


def test_plan_check_passes():
    out = subprocess.run(["make", "-B", "-C", CSRC, "plan_check"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "plan_check: ok" in out.stdout.splitlines(), out.stdout[-4000:]
    assert "FAILED" not in out.stdout
