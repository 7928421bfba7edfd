"""Static instruction budget of k_march's two loops, read from the compiler's own assembly (hipcc cross-compiles
without a GPU; CPU only, the device-only compile of the scorer translation unit that isa_text.py shares).

- The converter loops form no load address with VALU: the row base is uniform, so every global load takes the
  SGPR-base form with a 32-bit lane offset (global_load_dword v, v_off, s[base:base+1]); a 64-bit VALU add
  (v_lshl_add_u64, v_mad_u64_u32) costs ~4.2 cycles a wave-instruction (profiles/r06_valu_rate.txt).
- The blur loop spends at least six VALU instructions a step fewer than before the edge-difference quotient became
  one reciprocal times a product."""
import collections
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_text  # noqa: E402

KERNEL = "_ZN6ssimu27k_marchENS_9MarchPlanE"
# VALU instructions in the blur loop of k_march (nine unrolled steps) with the edge quotient computed by div_rn
BLUR_LOOP_VALU_BEFORE = 1430
STEPS_PER_LOOP = 9


@pytest.fixture(scope="module")
def loops():
    body = isa_text.scorer_asm().split(KERNEL + ":")[1].split("s_endpgm")[0]
    # instructions of each outermost loop, keyed by its header block (the compiler's loop annotations)
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
    return found


def _ops(lines):
    return collections.Counter(s.split()[0] for s in lines)


def test_converter_loops_form_no_load_address_with_valu(loops):
    conv = [v for v in loops.values() if any(s.startswith("global_load") for s in v)]
    assert len(conv) == 2, "one converter loop for 8-bit frames, one for fp32 planes"
    for v in conv:
        ops = _ops(v)
        assert ops["v_lshl_add_u64"] == 0 and ops["v_mad_u64_u32"] == 0, ops
        loads = [s for s in v if s.startswith("global_load")]
        assert all(re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\]", s) for s in loads), loads


def test_blur_step_is_at_least_six_valu_shorter(loops):
    blur = [v for v in loops.values() if _ops(v)["ds_read_b64"] >= STEPS_PER_LOOP * 9]
    assert len(blur) == 1
    valu = sum(n for op, n in _ops(blur[0]).items() if op.startswith("v_"))
    assert valu <= BLUR_LOOP_VALU_BEFORE - 6 * STEPS_PER_LOOP, valu
