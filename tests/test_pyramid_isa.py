"""The footprint of the pair score's pyramid kernels, read from the compiler's own output (hipcc cross-compiles without
a GPU; the device-only compile of the scorer unit that isa_text.py shares).  DESIGN.md section 4, "Two scores in
flight": a pyramid workgroup runs in the slot a marching workgroup has left -- 192 registers per SIMD lane, 16 wave
slots -- and two of them fit there only at <= 48 registers and <= 12 KB of LDS each; how long it stays depends on its
VALU count, of which the 64-bit per-lane address arithmetic (v_mad_u64_u32, v_lshl_add_u64, v_mad_i64_i32: quarter
rate) was a fifth before the row addresses moved to the scalar unit."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_text  # noqa: E402

PAIR = "_ZN6ssimu215k_pyramid_bandsENS_11PyrBandArgsE"
BATCH = "_ZN6ssimu221k_pyramid_bands_batchENS_12PyrBatchArgsE"
ADDRESS_64 = ("v_mad_u64_u32", "v_lshl_add_u64", "v_mad_i64_i32")


@pytest.fixture(scope="module")
def asm():
    return isa_text.scorer_asm()


def metadata(text, name):
    blocks = [b for b in text.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+(\S+)", b).group(1) == name]
    assert len(blocks) == 1, name
    return {k: int(re.search(rf"\.{k}:\s+(\d+)", blocks[0]).group(1))
            for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}


def instructions(text, name):
    """[(mnemonic, operands)] of the kernel `name`, in program order."""
    body = text.split("\n" + name + ":")[1].split(".Lfunc_end")[0]
    out = []
    for line in body.splitlines():
        if line.startswith("\t") and not line.startswith(("\t.", "\t;")):
            parts = line.split(None, 1)
            out.append((parts[0], parts[1] if len(parts) > 1 else ""))
    return out


@pytest.mark.parametrize("name", [PAIR, BATCH])
def test_two_pyramid_workgroups_fit_a_freed_marching_slot(asm, name):
    k = metadata(asm, name)
    assert k["vgpr_count"] <= 48, k                      # four waves per SIMD in 192 registers
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= 12 * 1024, k  # two beside two marching workgroups
    assert not any(m.startswith("scratch_") for m, _ in instructions(asm, name)), name


@pytest.mark.parametrize("name", [PAIR, BATCH])
def test_pyramid_waves_issue_ahead_of_the_marching_waves(asm, name):
    """The priority is raised before the first request to memory and never lowered: a workgroup's life in the slot
    is what it costs the marching kernel beside it."""
    ins = instructions(asm, name)
    prio = [(i, ops.strip()) for i, (m, ops) in enumerate(ins) if m == "s_setprio"]
    assert [p for _, p in prio] == ["3"], prio
    assert prio[0][0] < min(i for i, (m, _) in enumerate(ins) if m.startswith(("global_", "ds_"))), prio


def test_row_addresses_are_formed_on_the_scalar_unit(asm):
    ins = instructions(asm, PAIR)
    wide = [m for m, _ in ins if m.startswith(ADDRESS_64)]
    assert len(wide) <= 24, wide                         # 96 before; the allowance is for the clamped border path alone
    # whole 4 x 4 blocks: dword loads (the border path loads bytes and shorts), all of them base + 32-bit lane offset
    frame = [(m, ops) for m, ops in ins if m.startswith("global_load_dword")]
    assert frame
    for m, ops in frame:
        assert re.fullmatch(r"v(\d+|\[\d+:\d+\]), v\d+, s\[\d+:\d+\]( offset:-?\d+)?", ops.strip()), (m, ops)
    width = {"global_load_dword": 1, "global_load_dwordx2": 2, "global_load_dwordx3": 3, "global_load_dwordx4": 4}
    assert sum(width[m] for m, _ in frame) >= 1 + 12     # the table entry and four rows of 12 bytes


def test_frame_loads_fly_under_the_table_fill(asm):
    """The table entry and the 12 dwords of the frame are requested before the first barrier (the one after the table
    fill): one memory latency for both."""
    names = [m for m, _ in instructions(asm, PAIR)]
    first_barrier = names.index("s_barrier")
    loads = [i for i, m in enumerate(names) if m.startswith("global_load_")]
    assert loads and max(loads) < first_barrier, (loads[-1], first_barrier)


def test_level_one_goes_out_in_eight_byte_stores(asm):
    names = [m for m, _ in instructions(asm, PAIR)]
    assert names.count("global_store_dwordx2") >= 6      # two rows x three channels, one pair of floats each
