"""The per-pixel error map without a GPU: the numpy reference's definition against the CPU oracle, the C ABI's
declarations and argument checks, and the command-line tool's refusals."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oavif_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("w,h", [(192, 128), (96, 64), (64, 32), (24, 16)])
@pytest.mark.parametrize("mode", ["fir", "iir"])
def test_reference_map_mean_is_the_weighted_sum_of_the_oracles_averages(oracle, w, h, mode):
    blur = oracle.BLUR_FIR if mode == "fir" else oracle.BLUR_IIR
    ref = synth.make_ref(w, h, seed=w + h)
    dist = synth.distort(ref, "blockq", 2, seed=1)
    m, own, ns = errmap_ref.reference_map(oracle, ref, dist, blur)
    _score, avg, ns_o = oracle.compute_ssimu2(ref, dist, blur, return_averages=True)
    assert ns == ns_o and (w % (1 << (ns - 1)), h % (1 << (ns - 1))) == (0, 0)
    assert ns < 6 or (w, h) != (24, 16)
    _walk, total = errmap_ref.weighted_terms(oracle, avg, ns)
    assert m.shape == (h, w) and m.dtype == np.float32 and (m >= 0).all()
    assert np.mean(m, dtype=np.float64) == pytest.approx(total, rel=2e-6)
    np.testing.assert_allclose(own, avg, rtol=1e-6, atol=1e-9)


def test_reference_map_of_identical_frames_is_zero(oracle):
    ref = synth.make_ref(40, 24, seed=3)
    m, _own, ns = errmap_ref.reference_map(oracle, ref, ref, oracle.BLUR_FIR)
    assert ns == 3 and not m.any()


def test_header_declares_both_entry_points():
    text = open(os.path.join(ROOT, "include", "ssimu2_hip.h")).read()
    assert re.search(r"int ssimu2_error_map_rgb8\(ssimu2_ctx\* ctx, const uint8_t\* ref, const uint8_t\* dist, "
                     r"uint32_t w, uint32_t h,\s+uint32_t channels, float\* out_map, double\* out_score\);", text)
    assert re.search(r"int ssimu2_error_map_against_reference\(ssimu2_ctx\* ctx, const uint8_t\* dist, "
                     r"float\* out_map, double\* out_score\);", text)


def test_null_context_or_map_is_an_invalid_argument(hip_lib):
    from oavif_amd import _lib
    img = np.zeros((8, 8, 3), np.uint8)
    u8p = img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    m = np.zeros((8, 8), np.float32)
    f32p = m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    score = ctypes.c_double()
    assert hip_lib.ssimu2_error_map_rgb8(None, u8p, u8p, 8, 8, 3, f32p, ctypes.byref(score)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_error_map_rgb8(None, u8p, u8p, 8, 8, 3, None, ctypes.byref(score)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_error_map_against_reference(None, u8p, f32p, ctypes.byref(score)) == _lib.ERR_INVALID_ARG
    assert hip_lib.ssimu2_error_map_against_reference(None, u8p, None, ctypes.byref(score)) == _lib.ERR_INVALID_ARG


def _errmap(*args):
    return subprocess.run([sys.executable, "-m", "oavif_amd.errmap", *args], cwd=ROOT, capture_output=True,
                          text=True, timeout=120)


def test_errmap_help():
    r = _errmap("--help")
    assert r.returncode == 0 and "REF" in r.stdout.upper() and "--blur" in r.stdout


def test_errmap_refuses_a_missing_file(tmp_path):
    from oavif_amd.pam import write_pam
    ref = tmp_path / "ref.pam"
    ref.write_bytes(write_pam(synth.make_ref(16, 16, seed=0)))
    r = _errmap(str(ref), str(tmp_path / "missing.pam"), str(tmp_path / "out.png"))
    assert r.returncode != 0 and r.stdout == "" and "missing.pam" in r.stderr
    assert not (tmp_path / "out.png").exists()
    r = _errmap(str(ref), str(ref), str(tmp_path / "out.bmp"))
    assert r.returncode != 0 and r.stdout == ""


def test_errmap_encoders():
    from oavif_amd import errmap
    m = np.array([[0.0, 1.0, 2.0], [4.0, 3.0, 0.5]], np.float32)
    pfm = errmap.pfm_bytes(m)
    assert pfm.startswith(b"Pf\n3 2\n-1.0\n")
    assert np.array_equal(np.frombuffer(pfm[len(b"Pf\n3 2\n-1.0\n"):], "<f4").reshape(2, 3)[::-1], m)
    g, peak = errmap.to_grey8(m)
    assert peak == 4.0 and g.tolist() == [[0, 64, 128], [255, 191, 32]]
    import zlib
    png = errmap.png_bytes(g)
    assert png.startswith(b"\x89PNG\r\n\x1a\n")
    idat = png[png.index(b"IDAT") + 4:png.index(b"IEND") - 8]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(2, 4)
    assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:], g)
    assert errmap.to_grey8(np.zeros((2, 2), np.float32))[1] == 0.0
