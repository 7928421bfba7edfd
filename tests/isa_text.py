"""The gfx950 assembly of the scorer translation unit, and of any other unit of oavif_amd/csrc, for the tests that read
the compiler's own output (test_isa_budget.py, test_march_isa_trim.py, test_build_units.py): one device-only compile per
unit and session with the device flags of oavif_amd/build.py, the text kept for whoever asks next.  CPU only: hipcc
cross-compiles without a GPU."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from oavif_amd.build import DEVICE_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oavif_amd", "csrc")


@functools.lru_cache(maxsize=None)
def unit_asm(unit: str) -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc, *DEVICE_FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                       check=True, capture_output=True)
        with open(out) as f:
            return f.read()


def scorer_asm() -> str:
    return unit_asm("ssimu2_hip.hip")
