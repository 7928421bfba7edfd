"""The one body of the rule a full-depth error map (16-bit, RGBA, YUV frames; include/ssimu2_hip_map.h, DESIGN.md section
15) is held by, shared by tests/test_gpu_map_hbd.py, tests/test_gpu_map_grid.py and the 16-bit part of
tests/test_gpu_long_frames.py.  Importing this module needs no GPU.

The reference is numpy alone, built from the helpers the 8-bit map is held with: scale-0 linear planes
(hbd_ref.linear_planes, or the composite table for RGBA codes) -> errmap_ref.terms_lin -> errmap_ref.coefficients of the
DEVICE's averages (as gpu_cases.check_map takes them) -> errmap_ref.compose.  The comparison rule is check_map's, restated
in hold_map because check_map itself builds its reference from 8-bit frames: the recursive modes bit for bit; FIR per
pixel within gpu_cases.MAP_K * 2^-24 of the reference pixel and 0 exactly where the reference is 0; the mean to
errmap_ref.MEAN_RTOL."""
import numpy as np

import errmap_ref
import gpu_cases
import hbd_ref


def results(s, score):
    avg, ns = s.last_averages()
    return score, avg, ns


def assert_bits(got, exp, what):
    assert got[2] == exp[2], (what, got[2], exp[2])
    gpu_cases.bits_equal(got[0], got[1], exp[0], exp[1], what)


def hold_map(orc, m, exp, blur, what):
    """gpu_cases.check_map's rule for a device map `m` against the reference map `exp`.  -> the FIR map's largest
    deviation in units of 2^-24 (0 in the recursive modes)."""
    assert m.shape == exp.shape and m.dtype == exp.dtype == np.float32, what
    mean_e = exp.mean(dtype=np.float64)
    rel_mean = abs(m.mean(dtype=np.float64) - mean_e) / max(mean_e, 1e-30)
    assert rel_mean <= errmap_ref.MEAN_RTOL, (what, rel_mean)
    if blur != orc.BLUR_FIR:
        bad = m.view(np.uint32) != exp.view(np.uint32)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        return 0.0
    assert np.array_equal(m == 0, exp == 0), (what, int(np.sum((m == 0) != (exp == 0))))
    units = np.abs(m.astype(np.float64) - exp) / np.maximum(exp.astype(np.float64), 2.0 ** -126) * 2.0 ** 24
    worst = float(units.max()) if units.size else 0.0
    print(f"measured: {what}: FIR map {worst:.2f} units of 2^-24 (K = {gpu_cases.MAP_K})")
    assert worst <= gpu_cases.MAP_K, (what, worst, np.unravel_index(int(np.argmax(units)), units.shape))
    return worst


def reference_map(orc, lin_ref, lin_dist, blur, avg):
    """The numpy map of two frames given as scale-0 linear planes, its coefficients from the averages `avg`."""
    _c, h, w = lin_ref.shape
    tm = errmap_ref.terms_lin(orc, lin_ref, lin_dist, blur)
    return errmap_ref.compose(tm, errmap_ref.coefficients(orc, avg, len(tm)), w, h), len(tm)


def check_pair_hbd(orc, s, mode, ref, dist, d, what):
    """Case 1: the pair map against numpy; its score and averages are compute_ssimu2_hbd's bits."""
    blur = gpu_cases.MODES[mode][1]
    plain = results(s, s.compute_ssimu2_hbd(ref, dist, d))
    score, m = s.error_map_hbd(ref, dist, d)
    got = results(s, score)
    assert_bits(got, plain, what)
    exp, ns = reference_map(orc, hbd_ref.linear_planes(ref, d), hbd_ref.linear_planes(dist, d), blur, got[1])
    assert ns == got[2], what
    if ns == 0:
        assert score == 100.0 and not m.any(), what
    assert np.isfinite(m).all(), what
    return hold_map(orc, m, exp, blur, what), score, m
