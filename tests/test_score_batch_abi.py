"""Batch scoring without a GPU: the new entry points are declared, bound and exported, and the batch kernels keep the
budgets of the kernels they are forms of (one device-only compile of the scorer translation unit, as
tests/test_isa_budget.py and tests/test_march_isa_trim.py do for the single-score kernels)."""
import collections
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oavif_amd", "csrc", "ssimu2_hip.hip")

BATCH_SYMBOLS = ("ssimu2_score_batch_rgb8", "ssimu2_score_batch_against_reference", "ssimu2_score_batch_rgb8_device",
                 "ssimu2_score_batch_against_reference_device", "ssimu2_last_batch_averages")
K_MARCH = "_ZN6ssimu27k_marchENS_9MarchPlanE"
K_MARCH_BATCH = "_ZN6ssimu213k_march_batchENS_14MarchBatchPlanE"
K_REFBLUR_BATCH = "_ZN6ssimu221k_march_refblur_batchENS_14MarchBatchPlanE"


def test_batch_symbols_are_declared_bound_and_exported(hip_lib):
    from oavif_amd import Ssimu2, _lib
    header = open(os.path.join(ROOT, "include", "ssimu2_hip.h")).read()
    for name in BATCH_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    m = re.search(r"#define SSIMU2_MAX_BATCH (\d+)", header)
    assert m and int(m.group(1)) == _lib.MAX_BATCH
    for method in ("score_batch", "score_batch_against_reference", "score_batch_device",
                   "score_batch_against_reference_device", "last_batch_averages"):
        assert callable(getattr(Ssimu2, method)), method
    for name in ("ssimu2_instr_set_batch_segment_rows", "ssimu2_instr_batch_segment_rows"):
        assert name in _lib.INSTR_SYMBOLS and hasattr(_lib.instr_lib(), name), name
    zig = open(os.path.join(ROOT, "oavif_amd", "zig", "fssimu2.zig")).read()
    assert "pub fn computeSsimu2Batch(" in zig and "extern fn ssimu2_score_batch_rgb8(" in zig


def test_batch_calls_refuse_a_null_context(hip_lib):
    from oavif_amd import _lib
    out = ctypes.c_double()
    assert hip_lib.ssimu2_score_batch_rgb8(None, None, None, 1, 8, 8, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_score_batch_against_reference(None, None, 1, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_score_batch_rgb8_device(None, None, None, 192, 1, 8, 8, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_score_batch_against_reference_device(None, None, 192, 1, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_last_batch_averages(None, 0, None, None) == _lib.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    out = tmp_path_factory.mktemp("isa") / "scorer.s"
    # the flags of oavif_amd/build.py that shape device code
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-S", "--cuda-device-only", "-o", str(out), SRC], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
                                "private_segment_fixed_size")}
    return meta, text


def _body(text, kernel):
    return text.split(kernel + ":")[1].split("s_endpgm")[0]


def _loops(body):
    """Instructions of each outermost loop, keyed by its header block (the compiler's loop annotations)."""
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


def test_batch_marching_kernels_keep_the_budgets(isa):
    meta, text = isa
    for name in (K_MARCH_BATCH, K_REFBLUR_BATCH):
        k = meta[name]
        assert k["vgpr_count"] <= 80 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)                      # no scratch
        assert 3 * k["group_segment_fixed_size"] <= 160 * 1024, (name, k)            # three 8-wave workgroups per CU
        body = _body(text, name)
        assert "v_mfma" not in body and "v_pk_" not in body and "scratch_" not in body, name
    for name in ("_ZN6ssimu221k_pyramid_bands_batchENS_12PyrBatchArgsE", "_ZN6ssimu216k_finalize_batchENS_12FinalizeArgsEmPd"):
        k = meta[name]
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


def test_batch_converter_loops_form_no_load_address_with_valu(isa):
    """The item's base pointer is a blockIdx expression over kernel arguments: uniform, so the converters' loads keep
    the SGPR-base form k_march's have (tests/test_march_isa_trim.py)."""
    _meta, text = isa
    for name in (K_MARCH_BATCH, K_REFBLUR_BATCH):
        conv = [v for v in _loops(_body(text, name)).values() if any(s.startswith("global_load") for s in v)]
        # the blur loop of k_march_refblur_batch loads the cached blur(ref*ref) plane per lane: not a converter loop
        conv = [v for v in conv if _ops(v)["ds_read_b64"] < 81]
        assert len(conv) == 2, (name, "one converter loop for 8-bit frames, one for fp32 planes")
        for v in conv:
            ops = _ops(v)
            assert ops["v_lshl_add_u64"] == 0 and ops["v_mad_u64_u32"] == 0, (name, ops)
            loads = [s for s in v if s.startswith("global_load")]
            assert all(re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\]", s) for s in loads), (name, loads)


def test_batch_blur_loop_has_no_more_valu_than_k_march(isa):
    _meta, text = isa

    def blur_valu(kernel):
        blur = [v for v in _loops(_body(text, kernel)).values() if _ops(v)["ds_read_b64"] >= 81]
        assert len(blur) == 1, kernel
        return sum(n for op, n in _ops(blur[0]).items() if op.startswith("v_"))
    assert blur_valu(K_MARCH_BATCH) <= blur_valu(K_MARCH)
