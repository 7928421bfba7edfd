"""k_march_map_lin, the FIR map pass after a 16-bit score, in the compiler's own output: it exists,
spills nothing, touches no scratch memory, and needs no more vector registers or LDS than k_march_map of the same
compile -- so it keeps that kernel's three workgroups per CU.  CPU only (the device-only compile isa_text.py shares)."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_text  # noqa: E402

MAP = "_ZN6ssimu211k_march_mapENS_9MarchPlanENS_7MapCoefE"
MAP_LIN = "_ZN6ssimu215k_march_map_linENS_9MarchPlanENS_7MapCoefE"
KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


@pytest.fixture(scope="module")
def kernels():
    text = isa_text.scorer_asm()
    meta = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in KEYS}
    return meta, text


def _body(text, name):
    return text.split(f"\n{name}:")[1].split("s_endpgm")[0]


def test_the_kernel_exists_beside_the_8_bit_one(kernels):
    meta, text = kernels
    assert MAP in meta and MAP_LIN in meta
    assert len(_body(text, MAP_LIN)) > 1000 and len(_body(text, MAP)) > 1000


def test_it_spills_nothing_and_uses_no_scratch(kernels):
    meta, text = kernels
    k = meta[MAP_LIN]
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert "scratch_" not in _body(text, MAP_LIN)


def test_it_needs_no_more_registers_or_lds_than_the_8_bit_map_kernel(kernels):
    meta, _text = kernels
    lin, u8 = meta[MAP_LIN], meta[MAP]
    print(f"measured: k_march_map_lin {lin['vgpr_count']} VGPRs, {lin['group_segment_fixed_size']} bytes of LDS; "
          f"k_march_map {u8['vgpr_count']} VGPRs, {u8['group_segment_fixed_size']} bytes of LDS")
    assert lin["vgpr_count"] <= u8["vgpr_count"], (lin, u8)
    assert lin["group_segment_fixed_size"] <= u8["group_segment_fixed_size"], (lin, u8)
    assert u8["vgpr_count"] <= 80 and 3 * u8["group_segment_fixed_size"] <= 160 * 1024   # three workgroups per CU
