"""tests/fir_sums.py without a GPU: the vectorised restatement of k_march's summing order against the plain loop a lane
runs, the kernel-order averages against the exact means of the same terms (the bound the suite held the FIR averages
to before), and what the tighter bound buys: faults in the summing that the order-of-an-fp64-sum bound sees, and which
of them the rounding bound lets pass."""
import os
import sys

import numpy as np
import pytest

from oavif_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import fir_sums  # noqa: E402
import gpu_cases  # noqa: E402

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("w,h", [(13, 9), (121, 40)])
@pytest.mark.parametrize("seg", [1, 8, 37, 1000])
def test_vectorised_sum_equals_the_scalar_loop(w, h, seg):
    """Ragged planes, segments of one row, of rows that do not divide the plane, and longer than the plane.  The terms
    span 2^-40 .. 1 so that nearly every add rounds."""
    rng = np.random.default_rng(w * 1000 + seg)
    t = (rng.uniform(0.0, 1.0, (h, w)) * np.exp2(rng.integers(-40, 1, (h, w)))).astype(F32)
    t[rng.uniform(size=(h, w)) < 0.2] = 0.0
    got, exp = fir_sums.accumulators(t, seg), fir_sums.accumulators_scalar(t, seg)
    assert got.shape == exp.shape == ((h + seg - 1) // seg, w) and got.dtype == F32
    assert np.array_equal(_bits(got), _bits(exp))
    if seg >= h:      # one segment: against the running fp32 sum down the whole column
        run = np.zeros(w, F32)
        for y in range(h):
            run = run + t[y]
        assert np.array_equal(_bits(got[0]), _bits(run))
    if seg == 1:      # one row each: the accumulators are the terms
        assert np.array_equal(_bits(got), _bits(t))
    assert fir_sums.mean_of(got, w * h) == pytest.approx(float(t.astype(np.float64).mean()), rel=1e-6)


def test_the_bound_and_the_segment_rows_at_known_frames():
    """1921 x 1083 at 37 rows: N = 1921 * 30 accumulators, (N + 4) * 2^-53 = 6.4e-12, against 2.4e-6 before."""
    assert gpu_cases.march_seg_rows(1921, 1083, 0) == 37
    assert fir_sums.rtol(1921, 1083, 37) == (1921 * 30 + 4) * 2.0 ** -53
    assert 6.3e-12 < fir_sums.rtol(1921, 1083, 37) < 6.5e-12 and 2.3e-6 < gpu_cases.fir_rtol(1921, 1083, 0) < 2.5e-6
    assert gpu_cases.seg_rows(1000, 700) == [13] * 6 and gpu_cases.seg_rows(1921, 1083) == [37] * 6
    assert gpu_cases.seg_rows(3840, 2160) == [135] + [48] * 5
    assert gpu_cases.seg_rows(509, 131, gpu_cases.batch_seg_rows) == [96] + [48] * 5
    assert gpu_cases.override_rows(47, 160) == [47] + [160] * 5


SCORED = [s for s in gpu_cases.SIZES if min(s) >= 8]


@pytest.mark.parametrize("w,h", SCORED, ids=[f"{w}x{h}" for w, h in SCORED])
def test_kernel_order_averages_agree_with_the_exact_means(oracle, w, h):
    """The old derivation and the new one: averages 0..5 summed in the kernel's order lie within gpu_cases.fir_rtol of
    errmap_ref.kernel_averages' exact means, are 0 exactly where those are, and come from the same pass."""
    ref = synth.make_ref(w, h, 17 * w + h)
    dist = synth.distort(ref, "noise", 2, seed=w + 3 * h)
    rows = gpu_cases.seg_rows(w, h)
    kavg, ns, kord = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=rows)
    plain, ns_p = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR)
    assert ns == ns_p >= 1 and np.array_equal(kavg, plain) and kord.shape == (6, 6)
    assert not kord[ns:].any()
    worst = 0.0
    for s in range(ns):
        exp = kavg[s, :6]
        assert np.array_equal(kord[s] == 0, exp == 0)
        dev = np.abs(kord[s] - exp) / np.where(exp == 0, 1.0, exp)
        worst = max(worst, float(dev.max()) / gpu_cases.fir_rtol(w, h, s))
        assert (dev <= gpu_cases.fir_rtol(w, h, s)).all(), (s, dev, gpu_cases.fir_rtol(w, h, s))
    print(f"measured: {w}x{h}: kernel order against exact means {worst:.3e} of fir_rtol")


def test_the_other_routes_return_the_same_kernel_order_averages(oracle):
    """errmap_ref.averages and reference_map hand out kernel_averages' (6, 6), and an override's rows enter."""
    ref = synth.make_ref(121, 40, 5)
    dist = synth.distort(ref, "blockq", 2, seed=6)
    rows = gpu_cases.seg_rows(121, 40)
    _kavg, ns, kord = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=rows)
    tm = errmap_ref.terms(oracle, ref, dist, oracle.BLUR_FIR)
    avg_t, kord_t = errmap_ref.averages(tm, rows)
    m, own, ns_m, kord_m = errmap_ref.reference_map(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=rows)
    m0, own0, _ns0 = errmap_ref.reference_map(oracle, ref, dist, oracle.BLUR_FIR)
    assert ns == ns_m == len(tm) and np.array_equal(kord, kord_t) and np.array_equal(kord, kord_m)
    assert np.array_equal(own, own0) and np.array_equal(own, avg_t) and np.array_equal(_bits(m), _bits(m0))
    _a, _n, other = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=gpu_cases.override_rows(8, 9))
    assert not np.array_equal(other[:ns], kord[:ns])


def _shares(d, d4):
    """Per term, how far leaving it out moves the worse of the two averages, relatively (an L4 average moves by a
    quarter of its sum's share)."""
    d, d4 = d.astype(np.float64), d4.astype(np.float64)
    return np.maximum(d / d.sum(), d4 / d4.sum() / 4)


def _strip_rows(x, w):
    """(h, w) per-term values -> (h, nstrips) sums over each row of each 120-column strip."""
    h, nstrips = x.shape[0], (w + gpu_cases.MW - 1) // gpu_cases.MW
    pad = np.zeros((h, nstrips * gpu_cases.MW))
    pad[:, :w] = x
    return pad.reshape(h, nstrips, gpu_cases.MW).sum(2)


def _loudest_below(shares, limit):
    """Index of the largest entry of `shares` below `limit`."""
    flat = np.where(shares < limit, shares, -1.0).ravel()
    assert flat.max() > 0
    return np.unravel_index(int(np.argmax(flat)), shares.shape)


@pytest.mark.parametrize("w,h", [(1000, 700), (1921, 1083)])
def test_faults_the_rounding_bound_lets_pass(oracle, w, h):
    """The Y channel's d and d^4 terms at scale 0 of a seeded blockq-2 pair, summed in the kernel's order -- and then
    with a fault in the summing: one term dropped, one row of one strip added twice, every term once but in segments
    of seg - 1 rows.  Every fault moves the d or the d^4 average by more than fir_sums.rtol: the kernel-order check
    sees it.  gpu_cases.fir_rtol, the bound the suite held these averages to before, is (seg + 3) * 2^-24 of the sum
    whatever the frame: 2.4e-6 at 1921 x 1083 (37 rows), 9.5e-7 at 1000 x 700 (13 rows), where a median term is
    1 / pixels = 4.8e-7 and 1.4e-6 of the sum and a full strip row 120 / pixels = 5.8e-5 and 1.7e-4.  So what it lets
    pass is: the regrouping at both sizes; a median term at 1921 x 1083 but not quite at 1000 x 700; a busy strip row
    at neither, a quiet one at both (the last strip is 1 and 40 columns wide).  Each kind of fault is therefore run
    twice where that matters -- the median term and a mid-frame row of strip 3, and the loudest term and strip row
    whose share of the sums is below half of fir_rtol -- and the second must lie between the two bounds."""
    ref = synth.make_ref(w, h, seed=3)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    lin1, lin2 = (oracle.srgb_lut()[f].transpose(2, 0, 1).copy() for f in (ref, dist))
    t = errmap_ref.channel_terms(oracle, oracle.linear_to_xyb(lin1)[1], oracle.linear_to_xyb(lin2)[1], oracle.BLUR_FIR)
    d, d4 = t[0], t[1]
    seg = gpu_cases.march_seg_rows(w, h, 0)
    new, old = fir_sums.rtol(w, h, seg), gpu_cases.fir_rtol(w, h, 0)
    base = fir_sums.means(d, d4, seg)
    shares = _shares(d, d4)

    def moved(got):
        return max(abs(g - b) / b for g, b in zip(got, base))

    def without_term(y, x):
        dz, d4z = d.copy(), d4.copy()
        dz[y, x] = d4z[y, x] = 0.0
        return moved(fir_sums.means(dz, d4z, seg))

    def strip_row_twice(y, strip):
        x0, out = strip * gpu_cases.MW, []
        for plane in (d, d4):
            acc = fir_sums.accumulators(plane, seg)
            acc[y // seg, x0:x0 + gpu_cases.MW] = acc[y // seg, x0:x0 + gpu_cases.MW] + plane[y, x0:x0 + gpu_cases.MW]
            out.append(fir_sums.mean_of(acc, w * h))
        return moved((out[0], out[1] ** 0.25))

    nz = np.flatnonzero(d.ravel() > 0)
    median = np.unravel_index(int(nz[np.argsort(d.ravel()[nz])[nz.size // 2]]), d.shape)
    faults = [
        # (name, relative move of the worse average, must the rounding bound let it pass?)
        ("one median term zeroed", without_term(*median), (w, h) == (1921, 1083)),
        ("the loudest term below half of fir_rtol zeroed", without_term(*_loudest_below(shares, old / 2)), True),
        ("a mid-frame row of strip 3 added twice", strip_row_twice((h // 2 // seg) * seg + seg // 2, 3), False),
        ("the loudest strip row below half of fir_rtol added twice",
         strip_row_twice(*_loudest_below(_strip_rows(shares, w), old / 2)), True),
        ("seg - 1 rows per segment", moved(fir_sums.means(d, d4, seg - 1)), True),
    ]
    for name, dev, passes_the_old_bound in faults:
        print(f"measured: {w}x{h} {name}: {dev:.3e} = {dev / new:.1f} of the kernel-order bound, "
              f"{dev / old:.2e} of fir_rtol")
        assert dev > new, (name, dev, new)
        assert (dev < old) == passes_the_old_bound, (name, dev, old)
