"""The per-pixel error map without a GPU: the numpy reference's definition against the CPU oracle, the C ABI's
declarations and argument checks, and the command-line tool's refusals."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

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


def _rn32(x: Fraction) -> np.float32:
    """x correctly rounded to fp32 (to nearest, ties to even), by exact comparison with the neighbours of a value
    at most one fp32 ulp from it."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.array(v).view(np.uint32)) & 1))


def _exact_fma(a, b, c) -> np.float32:
    return _rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma_is_correctly_rounded_on_random_operands():
    """errmap_ref._fma against exact rational arithmetic: operands over 2^-30..2^30 of both signs, and sums that
    cancel (c near -a * b), where most of the product's bits decide the result."""
    rng = np.random.default_rng(2024)
    n = 3000

    def f32(k, lo, hi):
        m = rng.uniform(1.0, 2.0, k) * rng.choice([-1.0, 1.0], k)
        return (m * np.exp2(rng.integers(lo, hi, k).astype(np.float64))).astype(np.float32)

    a, b, c = f32(n, -15, 15), f32(n, -15, 15), f32(n, -30, 30)
    c[: n // 3] = -(a[: n // 3].astype(np.float64) * b[: n // 3]).astype(np.float32)   # cancellation
    c[n // 3: n // 2] = np.nextafter(c[: n // 6], np.float32(np.inf))
    got = errmap_ref._fma(a, b, c)
    exp = np.array([_exact_fma(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, exp), int(np.sum(got != exp))
    assert errmap_ref._fma(np.float32(-0.75), np.float32(0.75), 1.0) == np.float32(0.4375)


def _double_rounding_cases():
    """(a, b, c = 1) with a * b = t (1 + r), t = 2^-24 or 3 * 2^-24 and 0 < |r| * t < 2^-53: the exact sum lies within
    half an fp64 ulp of the fp32 halfway point 1 + t, so rounding it to fp64 lands on that point and the tie then goes
    to the even neighbour, which is the wrong one when r has the sign that moves the sum away from it."""
    out = []
    for t, sign in ((2.0 ** -24, 1), (3 * 2.0 ** -24, -1)):
        for k in range(1, 1 << 16):
            a = np.float32(1.0 + k * 2.0 ** -23)
            b = np.float32(t / float(a))
            r = Fraction(float(a)) * Fraction(float(b)) / Fraction(t) - 1
            if r != 0 and (r > 0) == (sign > 0) and abs(r) * Fraction(t) < Fraction(1, 2 ** 53):
                out.append((a, b, np.float32(1.0)))
                if len(out) % 8 == 0:
                    break
    return out


def test_fma_rounds_once_where_rounding_through_fp64_rounds_twice():
    cases = _double_rounding_cases()
    assert len(cases) == 16
    for a, b, c in cases:
        twice = np.float32(float(a) * float(b) + float(c))   # the fp64 sum, then fp32: two roundings
        exact = _exact_fma(a, b, c)
        assert twice != exact, (a, b)
        assert errmap_ref._fma(a, b, c) == exact, (a, b)
        assert errmap_ref._fma(np.array([a]), np.array([b]), np.array([c]))[0] == exact


def test_coefficients_restate_the_hosts_expression(oracle):
    """map_coefficients (ssimu2_hip.hip): w, or w / (a * a * a) in fp64 clamped at 3e38 and rounded once to fp32,
    0 when a == 0 -- against exact rationals of the same fp64 steps, at a == 0, around the clamp and where the cube
    underflows (the quotient is inf there, then 3e38)."""
    wts = oracle.weights()
    walk, _ = errmap_ref.weighted_terms(oracle, np.zeros((6, 18)), 6)
    w = max(wt for wt, _s, st in walk if st % 2 == 1 and wt > 0)
    clamp_a = (w / 3.0e38) ** (1.0 / 3.0)          # the L4 average whose coefficient is the clamp
    for a in [0.0, 1e-200, 1e-110, 1e-105, clamp_a * (1 - 1e-9), clamp_a, clamp_a * (1 + 1e-9), clamp_a * 1.01,
              1e-3, 0.0123456789, 0.5, 1.0]:
        got = errmap_ref.coefficient(w, a, True)
        if a == 0.0:
            exp = np.float32(0.0)
        else:
            a3 = Fraction(float(Fraction(a) * Fraction(a))) * Fraction(a)
            a3 = float(a3) if a3 else 0.0
            q = float(Fraction(w) / Fraction(a3)) if a3 and Fraction(w) / Fraction(a3) < 2 ** 1024 else np.inf
            exp = _rn32(Fraction(min(q, 3.0e38)))
        assert got == exp and got.dtype == np.float32, (a, got, exp)
        assert errmap_ref.coefficient(w, a, False) == np.float32(w)
    assert errmap_ref.coefficient(w, 1e-110, True) == np.float32(3.0e38)
    (w0, s0, st0), (w1, s1, st1) = [(wt, sc, st) for wt, sc, st in walk if st % 2 == 1 and wt > 0][:2]
    avg = np.full((6, 18), 0.25)
    avg[s0, st0], avg[s1, st1] = 0.0, 1e-110
    coef = errmap_ref.coefficients(oracle, avg, 6)
    assert coef.dtype == np.float32 and coef[s0, st0] == 0.0 and coef[s1, st1] == np.float32(3.0e38)
    assert coef[0, 0] == np.float32(wts[0]) and coef[0, 1] == np.float32(wts[3] / (0.25 * 0.25 * 0.25))


def test_compose_stays_finite_where_coefficients_reach_the_clamp(oracle):
    """Averages small enough that w / a^3 passes 3e38: 512 x 512 term planes, zero but for one pixel per plane that
    holds the smallest subnormal (d^4, art^4, det^4) or 2^-30 (d, art, det).  An L4 average is then
    (2^-149 / pixels)^(1/4) = 2.7e-13 at scale 0, and the statistics of weight above 5.9 there would get a coefficient
    beyond the clamp.  No natural pair was found that gets there; the map of these terms is finite, and its one
    non-zero scale-0 pixel is the clamped coefficients times the subnormal terms."""
    w = h = 512
    tm = []
    for s in range(6):
        t = np.zeros((3, 6, h >> s, w >> s), np.float32)
        t[:, 1::2, 3, 5] = np.float32(2.0 ** -149)
        t[:, 0::2, 3, 5] = np.float32(2.0 ** -30)
        tm.append(t)
    avg = errmap_ref.averages(tm)
    coef = errmap_ref.coefficients(oracle, avg, 6)
    clamped = np.argwhere(coef == np.float32(3.0e38))
    assert len(clamped) >= 2 and (clamped[:, 0] == 0).all() and (clamped[:, 1] % 2 == 1).all(), clamped
    walk, _ = errmap_ref.weighted_terms(oracle, avg, 6)
    for wt, s, st in walk:
        unclamped = wt / avg[s, st] ** 3 if st % 2 == 1 else wt
        assert (unclamped > 3.0e38) == (coef[s, st] == np.float32(3.0e38)), (s, st, unclamped)
    assert np.isfinite(coef).all() and coef.max() == np.float32(3.0e38)
    m = errmap_ref.compose(tm, coef, w, h)
    assert m.dtype == np.float32 and np.isfinite(m).all() and (m >= 0).all()
    exp = sum(float(coef[0, errmap_ref.stat_of(c, k)]) * float(tm[0][c, k, 3, 5]) for c in range(3) for k in range(6))
    assert exp > 2 * 3.0e38 * 2.0 ** -149 and m[3, 5] == pytest.approx(exp, rel=1e-6)
    assert np.count_nonzero(m) == sum(4 ** s for s in range(6))   # one pixel per scale, 2^s x 2^s map pixels each


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
