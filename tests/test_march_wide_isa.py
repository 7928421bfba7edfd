"""Static budgets of the wide marching geometry, from the compiler's own assembly (CPU only; the device-only compile of
the scorer unit that isa_text.py shares with the other ISA tests).

- The kernels that leave partial sums hold the wide ring: 16 rows x 3 channels x 136 staged columns x 8 bytes, the
  sRGB table where the kernel converts 8-bit frames, and the 36 doubles of s_part; three workgroups stay below the
  160 KiB of a CU.  The kernels that write planes keep the narrow ring, as in profiles/march_wide_ab.txt.
- <= 80 VGPRs, no spills, no scratch: three workgroups of eight waves per CU.
- The converter loops pay for the halo pass and for nothing else: per six rows at most HALO_PASS_VALU more VALU than the
  parent's loops, whose counts are read from the record.  The blur loop has no more VALU than the parent's."""
import collections
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_text  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "march_wide_ab.txt")
RING = 16 * 3 * 8
LUT, S_PART = 256 * 4, 6 * 6 * 8
# mangled name -> (staged columns, holds the sRGB table)
WIDE_KERNELS = {
    "_ZN6ssimu27k_marchENS_9MarchPlanE": (136, True),
    "_ZN6ssimu215k_march_refblurENS_9MarchPlanE": (136, True),
    "_ZN6ssimu213k_march_batchENS_14MarchBatchPlanE": (136, True),
    "_ZN6ssimu221k_march_refblur_batchENS_14MarchBatchPlanE": (136, True),
    "_ZN6ssimu211k_march_linENS_9MarchPlanE": (136, False),
    "_ZN6ssimu219k_march_refblur_linENS_9MarchPlanE": (136, False),
}
K_MARCH = "_ZN6ssimu27k_marchENS_9MarchPlanE"
# One halo pass is one pixel of one frame per lane: the opsin mix (9), three cube roots (3 x 17), the bias taken off
# them (3) and the XYB sums (7) are 70; the three table indices of a u8 pixel (a shift, three extracts, three scalings)
# 7; the lane's ring slot and address (row + lane's row, mask, multiply-add, the offset's copy for the load) and the
# moves around the two uniform branches the rest.
HALO_PASS_VALU = 90


def _meta(asm, name):
    """(LDS bytes, VGPRs, spilled VGPRs, scratch bytes) from the kernel's metadata entry."""
    block = next(b for b in asm.split("  - .agpr_count:") if re.search(r"\.name:\s+%s\s" % re.escape(name), b))
    get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
    return get("group_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"), get("private_segment_fixed_size")


def _loops(asm, kernel):
    body = asm.split(kernel + ":")[1].split("s_endpgm")[0]
    found = collections.defaultdict(list)
    cur = None
    for line in body.split("\n"):
        label = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):", line)
        if label:
            head = re.search(r"=>This Inner Loop Header: Depth=1", line)
            inside = re.search(r"in Loop: Header=BB(\d+_\d+) Depth=1", line)
            cur = label.group(1)[4:] if head else (inside.group(1) if inside else None)
            continue
        s = line.strip()
        if cur and s and not s.startswith((";", ".")):
            found[cur].append(s)
    return list(found.values())


def _valu(lines):
    return sum(1 for s in lines if s.startswith("v_"))


def _record():
    """The parent's counts of k_march and every marching kernel's LDS bytes, as the record states them."""
    with open(RECORD) as f:
        text = f.read()
    m = re.search(r"^k_march\s+parent\s+converter loop VALU: 8-bit (\d+), fp32 (\d+); blur loop VALU (\d+)", text, re.M)
    lds = {k: int(v) for k, v in re.findall(r"^(k_\w+)\s+LDS parent (\d+)", text, re.M)}
    return {"u8": int(m.group(1)), "f32": int(m.group(2)), "blur": int(m.group(3))}, lds


@pytest.mark.parametrize("name", sorted(WIDE_KERNELS))
def test_wide_ring_registers_and_three_workgroups_per_cu(name):
    cols, lut = WIDE_KERNELS[name]
    lds, vgprs, spilled, scratch = _meta(isa_text.scorer_asm(), name)
    assert lds == RING * cols + (LUT if lut else 0) + S_PART
    assert 3 * lds <= 160 * 1024
    assert vgprs <= 80 and spilled == 0 and scratch == 0


def test_kernels_that_write_planes_keep_the_parent_s_lds():
    asm = isa_text.scorer_asm()
    _counts, lds = _record()
    for short, name in (("k_ref_blur", "_ZN6ssimu210k_ref_blurENS_9MarchPlanE"),
                        ("k_march_map", "_ZN6ssimu211k_march_mapENS_9MarchPlanENS_7MapCoefE"),
                        ("k_march_map_lin", "_ZN6ssimu215k_march_map_linENS_9MarchPlanENS_7MapCoefE")):
        assert _meta(asm, name)[0] == lds[short], short


def test_the_loops_pay_for_the_halo_pass_and_nothing_else():
    parent, _lds = _record()
    loops = _loops(isa_text.scorer_asm(), K_MARCH)
    conv = [v for v in loops if any(s.startswith("global_load") for s in v)]
    assert len(conv) == 2
    u8 = next(v for v in conv if any(s.startswith("ds_read_b32") for s in v))  # the loop that reads the sRGB table
    f32 = next(v for v in conv if v is not u8)
    print(f"measured: converter loops, VALU per six rows: 8-bit {_valu(u8)} (parent {parent['u8']}), "
          f"fp32 {_valu(f32)} (parent {parent['f32']})")
    assert parent["u8"] < _valu(u8) <= parent["u8"] + HALO_PASS_VALU
    assert parent["f32"] < _valu(f32) <= parent["f32"] + HALO_PASS_VALU
    blur = [v for v in loops if sum(1 for s in v if s.startswith("ds_read_b64")) >= 81]
    assert len(blur) == 1 and _valu(blur[0]) <= parent["blur"]
