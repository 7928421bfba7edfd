"""16-bit scorer input without a GPU (include/ssimu2_hip.h): the library's sRGB tables against
their restatement and the 8-bit table, the CPU references of tests/hbd_ref.py on 257*u frames, argument checks, and the
register / LDS budgets of the new kernels (one device-only compile, test_isa_budget.py's flags)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hbd_ref
import ssimu2_fp64 as ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oavif_amd", "csrc", "ssimu2_hip.hip")


@pytest.mark.parametrize("d", range(8, 17))
def test_library_table_is_the_restatement(hip_lib, d):
    from oavif_amd import scorer
    got = scorer.linear_table(d)
    exp = hbd_ref.table(d)
    assert got.dtype == np.float32 and got.shape == (1 << d,)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.all(np.diff(got) > 0) and got[0] == 0.0 and got[-1] == 1.0


def test_tables_contain_the_8bit_table(oracle):
    lut = oracle.srgb_lut()
    u = np.arange(256)
    assert np.array_equal(hbd_ref.table(8).view(np.uint32), lut.view(np.uint32))
    assert np.array_equal(hbd_ref.table(16)[257 * u].view(np.uint32), lut.view(np.uint32))


def test_table_call_refuses_bad_depths(hip_lib):
    from oavif_amd import _lib
    buf = np.zeros(1 << 16, np.float32)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for d in (0, 7, 17, 32):
        assert hip_lib.ssimu2_linear_table(d, p) == _lib.ERR_UNSUPPORTED
    assert hip_lib.ssimu2_linear_table(10, None) == _lib.ERR_INVALID_ARG


def test_null_context_arguments(hip_lib):
    from oavif_amd import _lib
    out = ctypes.c_double()
    a = np.zeros(48, np.uint16)
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    assert hip_lib.ssimu2_score_rgb16(None, p, p, 4, 4, 3, 16, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_set_reference_rgb16(None, p, 4, 4, 10) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_score_against_reference_rgb16(None, p, 10, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_score_against_reference_strided16(None, p, 24, 3, 10, ctypes.byref(out)) == _lib.ERR_INVALID_ARG


def _frames(w, h, seed):
    from oavif_amd import synth
    ref = synth.make_ref(w, h, seed=seed)
    return ref, synth.distort(ref, "blockq", 2)


@pytest.mark.parametrize("blur", ["fir", "iir"])
def test_cpu_reference_on_257u_frames_is_the_checker(oracle, blur):
    mode = oracle.BLUR_FIR if blur == "fir" else oracle.BLUR_IIR
    for k, (w, h) in enumerate([(96, 64), (67, 41), (9, 200)]):
        ref, dist = _frames(w, h, k)
        exp, avg_o, ns_o = oracle.compute_ssimu2(ref, dist, mode, return_averages=True)
        r16, d16 = ref.astype(np.uint16) * 257, dist.astype(np.uint16) * 257
        got, avg, ns = hbd_ref.compute(oracle, r16, d16, 16, mode)
        assert ns == ns_o
        assert abs(got - exp) <= 1e-4 * max(1.0, abs(exp) / 100.0), (w, h, got, exp)
        assert np.allclose(avg, np.asarray(avg_o).reshape(6, 18), rtol=2e-5, atol=1e-9)
        # an 8-bit-depth uint16 frame holding u is the same frame
        got8, avg8, _ = hbd_ref.compute(oracle, ref.astype(np.uint16), dist.astype(np.uint16), 8, mode)
        assert got8 == got and np.array_equal(avg8, avg)


@pytest.mark.parametrize("blur", ["fir", "iir"])
def test_cpu_reference_averages_are_the_kernel_order_terms_averages(oracle, blur):
    """hbd_ref.compute's averages are errmap_ref.averages(hbd_ref.terms(...)) bit for bit (what the GPU tests pass to
    gpu_cases.check_against_terms as kavg), at the frames' own depths; on 257 u frames they are the 8-bit path's
    errmap_ref.kernel_averages."""
    import errmap_ref
    mode = oracle.BLUR_FIR if blur == "fir" else oracle.BLUR_IIR
    rng = np.random.default_rng(5)
    r12 = rng.integers(0, 4096, (41, 67, 3)).astype(np.uint16)
    d10 = np.minimum(r12 // 4 + rng.integers(0, 9, r12.shape), 1023).astype(np.uint16)
    score, avg, ns = hbd_ref.compute(oracle, r12, d10, 12, mode, d_dist=10)
    tm = hbd_ref.terms(oracle, hbd_ref.linear_planes(r12, 12), hbd_ref.linear_planes(d10, 10), mode)
    assert ns == len(tm) == 4 and np.array_equal(avg, errmap_ref.averages(tm))
    assert score == oracle.score_from_averages(avg, ns) and avg[:ns].any() and not avg[ns:].any()
    ref, dist = _frames(67, 41, 3)
    _, avg16, ns16 = hbd_ref.compute(oracle, ref.astype(np.uint16) * 257, dist.astype(np.uint16) * 257, 16, mode)
    kavg, ns8 = errmap_ref.kernel_averages(oracle, ref, dist, mode)
    assert ns16 == ns8 and np.array_equal(avg16, kavg)


def test_fp64_counterpart_on_257u_frames():
    ref, dist = _frames(80, 56, 7)
    exp = ref64.evaluate(ref, dist)
    got = hbd_ref.compute_fp64(ref.astype(np.uint16) * 257, dist.astype(np.uint16) * 257, 16)
    assert got["nscales"] == exp["nscales"]
    assert np.allclose(got["averages"], exp["averages"], rtol=1e-12, atol=1e-15)
    assert abs(got["score"] - exp["score"]) <= 1e-9


def test_fp64_counterpart_with_the_frames_own_depth():
    """compute_fp64(d_dist=d) is the call without it; another d_dist reads the frame, and only the frame, at that
    depth."""
    rng = np.random.default_rng(11)
    ref = rng.integers(0, 1 << 12, (40, 56, 3)).astype(np.uint16)
    dist = np.clip(ref.astype(np.int64) + rng.integers(-40, 41, ref.shape), 0, 4095).astype(np.uint16)
    for d in (10, 12, 16):
        a, b = hbd_ref.compute_fp64(ref, dist, d), hbd_ref.compute_fp64(ref, dist, d, d_dist=d)
        assert a["score"] == b["score"] and a["nscales"] == b["nscales"]
        assert np.array_equal(a["averages"], b["averages"]) and a["weighted_sum"] == b["weighted_sum"]
    # an 8-bit reference u is the 16-bit reference 257 u (the same doubles), whatever the frame's own depth
    r8 = (ref >> 4).astype(np.uint16)
    mixed = hbd_ref.compute_fp64(r8, dist, 8, d_dist=12)
    lifted = hbd_ref.compute_fp64(r8 * np.uint16(257), dist, 16, d_dist=12)
    assert mixed["score"] == lifted["score"] and np.array_equal(mixed["averages"], lifted["averages"])
    assert mixed["score"] != hbd_ref.compute_fp64(r8 * np.uint16(257), dist, 16)["score"]


def test_uint16_levels_on_257u_frames_are_the_8bit_levels():
    """hbd_ref.reference_levels of 257*u frames (and of depth-8 uint16 frames of u) = fp64_checks.reference_levels
    of u, bit for bit; the checker-route levels equal the 8-bit pyramid of the oracle's table."""
    import fp64_checks
    from oracle import ssimu2_oracle as orc
    ref, dist = _frames(67, 45, 3)
    scales = list(range(ref64.nscales_of(67, 45)))
    exp = fp64_checks.reference_levels(ref, dist, scales)
    r16, d16 = ref.astype(np.uint16) * 257, dist.astype(np.uint16) * 257
    for got in (hbd_ref.reference_levels(r16, d16, 16, scales),
                hbd_ref.reference_levels(ref.astype(np.uint16), dist.astype(np.uint16), 8, scales),
                hbd_ref.reference_levels(r16, dist.astype(np.uint16), 16, scales, d_dist=8)):
        assert sorted(got) == scales
        for s in scales:
            for k in range(4):
                assert got[s][k].dtype == np.float64 and np.array_equal(got[s][k], exp[s][k]), (s, k)
    lin = np.ascontiguousarray(orc.srgb_lut()[ref].transpose(2, 0, 1))
    lv = hbd_ref.levels(orc, r16, 16)
    assert len(lv) == len(scales)
    for s, (lin16, xyb16) in enumerate(lv):
        if s:
            lin = orc.downsample2(lin)
        assert np.array_equal(lin16.view(np.uint32), lin.view(np.uint32)), s
        assert np.array_equal(xyb16.view(np.uint32), orc.linear_to_xyb(lin).view(np.uint32)), s


def test_every_code_frame_holds_each_code_once_per_channel():
    f = hbd_ref.every_code_frame()
    assert f.shape == (256, 256, 3) and f.dtype == np.uint16 and f.flags.c_contiguous
    codes = np.arange(1 << 16)
    for c in range(3):
        assert np.array_equal(np.sort(f[..., c].reshape(-1)), codes), c
    for a, b in ((0, 1), (0, 2), (1, 2)):   # three different orders
        assert np.count_nonzero(f[..., a] == f[..., b]) < 64, (a, b)
    assert np.array_equal(f, hbd_ref.every_code_frame())


def test_clamping_in_the_reference():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 65536, (16, 16, 3)).astype(np.uint16)
    assert np.array_equal(hbd_ref.linear_planes(a, 10), hbd_ref.linear_planes(np.minimum(a, 1023), 10))


@pytest.fixture(scope="module")
def kernels():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "scorer.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                        "-S", "--cuda-device-only", "-o", out, SRC], check=True, capture_output=True)
        text = open(out).read()
    meta = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
    return meta, text


def _hits(meta, fragment):
    hits = {k: v for k, v in meta.items() if fragment in k}
    assert hits, fragment
    return hits


def test_new_marching_kernels_keep_the_budgets(kernels):
    meta, text = kernels
    for frag in ("11k_march_linE", "19k_march_refblur_linE"):
        for name, k in _hits(meta, frag).items():
            assert k["vgpr_count"] <= 80 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
            assert 3 * k["group_segment_fixed_size"] <= 160 * 1024, (name, k)
            body = text.split(name + ":")[1].split("s_endpgm")[0]
            assert "v_mfma" not in body and "v_pk_" not in body and "scratch_" not in body, name


def test_new_pyramid_kernels_do_not_spill(kernels):
    meta, _ = kernels
    for frag in ("k_pyramid_bands16ILi3", "k_pyramid_bands16ILi4", "k_pyramid_bands_xyb16ILi3",
                 "k_pyramid_bands_xyb16ILi4"):
        for name, k in _hits(meta, frag).items():
            assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)


def _avif_or_skip():
    from oavif_amd import avif_bridge as ab
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    return ab


def _enc_opts():
    from oavif_amd import cli
    o = cli.AvifEncOptions()
    o.tenbit = False
    return o


@pytest.mark.parametrize("alpha", [False, True])
def test_decode_at_16_bits_gives_uint16_rows(alpha):
    ab = _avif_or_skip()
    from oavif_amd import synth
    ref = synth.make_ref(96, 64, 3)
    src = np.dstack([ref, np.full(ref.shape[:2], 200, np.uint8)]) if alpha else ref
    data = ab.encode(src, 8, _enc_opts(), 60)
    with ab.decode_common(data, rgb_depth=16) as f:
        ch = 4 if alpha else 3
        assert f.rgb_depth == 16 and f.channels == ch and f.depth == 8
        assert f.rows.dtype == np.uint16 and f.rows.shape == (64, f.row_bytes // 2) and f.row_bytes >= 96 * ch * 2
        px = f.tight_rgb16()
        assert px.shape == (64, 96, 3) and px.dtype == np.uint16
        with pytest.raises(ab.AvifBridgeError):
            f.tight_rgb8()
    # libavif scales 8-bit codes to 16 bits: close to 257 times the 8-bit decode
    d8 = ab.decode_rgb8(data)
    assert np.abs(px.astype(np.int64) - d8.astype(np.int64) * 257).max() <= 2 * 257
    with pytest.raises(ValueError):
        ab.decode_common(data, rgb_depth=9)


def test_default_decode_is_unchanged():
    ab = _avif_or_skip()
    from oavif_amd import synth
    ref = synth.make_ref(80, 48, 5)
    data = ab.encode(ref, 8, _enc_opts(), 50)
    with ab.decode_common(data) as f, ab.decode_common(data, rgb_depth=8) as g:
        assert f.rgb_depth == 8 and f.rows.dtype == np.uint8
        assert f.row_bytes == g.row_bytes and np.array_equal(f.rows, g.rows)
        assert np.array_equal(f.tight_rgb8(), ab.decode_rgb8(data))


def test_search_needs_the_depth_of_a_uint16_source():
    from oavif_amd import tq
    with pytest.raises(ValueError):
        tq.search_hip_frames(object(), np.zeros((8, 8, 3), np.uint16), lambda q: None)
