import os
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "cpu-raytracer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

# torch before any test loads librtx_hip.so, as bench.py and smoke() do: the extension then binds to the HIP runtime torch has
# already loaded.  The other way round, torch brings a second HIP runtime into the process, and once torch has initialised its
# own, the extension's finds no device (rtx_create: RTX_ERR_NO_DEVICE in every in-process GPU test of a whole-suite run).
import torch  # noqa: E402,F401


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
