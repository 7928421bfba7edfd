"""CPU only.  How far does the fp32 checker (oracle/ssimu2_oracle.c) sit from the fp64 reference
(tests/ssimu2_fp64.py), stage by stage and score by score, in each blur mode?  The bounds of tests/fp64_checks.py
are this tool's maxima times a margin.

Stages: the sRGB table (all 256 codes), linear_to_xyb (all 2^24 colours), downsample2, blur_plane in FIR / EXACT
(random and XYB planes) and in the two recursive orders (lines of 16 .. 4096).  Scores: random cases (sizes 1..600
per side, the five content kinds of tests/gpu_cases.py plus synth.make_ref, four distortion kinds, strengths 1..3)
and 1080p / 4K pairs, each in FIR, EXACT, IIR and IIR_FMA.  The recursive modes are also reported by frame size.

Usage: cpu_fp64_campaign.py [N_CASES] [--no-large] [--no-stages] [--seed S] [--hbd-maps]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import fp64_checks as fc  # noqa: E402
import ssimu2_fp64 as R  # noqa: E402
from gpu_cases import content  # noqa: E402
from oavif_amd import synth  # noqa: E402
from oracle import ssimu2_oracle as orc  # noqa: E402

MODES = {"fir": orc.BLUR_FIR, "exact": orc.BLUR_EXACT, "recursive": orc.BLUR_IIR, "recursive_fma": orc.BLUR_IIR_FMA}
KINDS = ["make_ref", "gradient", "primaries", "checker", "text", "noise"]
DISTORTIONS = ["blockq", "noise", "blur", "band"]


def ulps(got32, exp64):
    exp64 = np.asarray(exp64, np.float64)
    sp = np.spacing(np.abs(exp64).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got32, np.float64) - exp64) / sp))


def stage_campaign():
    out = {}
    lut = orc.srgb_lut()
    out["srgb_lut mismatches"] = int(np.count_nonzero(lut != R.srgb_to_linear(np.arange(256)).astype(np.float32)))
    worst = np.zeros(3)
    v = np.arange(1 << 24, dtype=np.uint32)
    for lo in range(0, 1 << 24, 1 << 20):
        c = v[lo:lo + (1 << 20)]
        rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255]).reshape(3, 1, -1)
        got = orc.linear_to_xyb(lut[rgb])
        exp = R.to_xyb(R.srgb_to_linear(rgb))
        worst = np.maximum(worst, np.abs(got.astype(np.float64) - exp).max(axis=(1, 2)))
    out["xyb abs X/Y/B"] = worst.tolist()
    rng = np.random.default_rng(1)
    ds = 0.0
    for h, w in [(1, 1), (1, 7), (7, 1), (2, 2), (9, 13), (64, 64), (129, 67), (333, 217)]:
        p = rng.random((3, h, w)).astype(np.float32)
        ds = max(ds, ulps(orc.downsample2(p), R.downsample2(p.astype(np.float64))))
    out["downsample2 ulps"] = ds
    planes = []
    for h, w in [(1, 1), (2, 9), (9, 2), (13, 11), (64, 64), (333, 217), (200, 700)]:
        planes.append(rng.random((h, w)).astype(np.float32))
        img = synth.make_ref(w, h, h + w)
        xyb = orc.linear_to_xyb(orc.srgb_lut()[img].transpose(2, 0, 1))
        planes += [xyb[c] for c in range(3)] + [xyb[1] * xyb[1]]
    out["blur fir rel"] = max(float(np.abs(orc.blur_plane(p, orc.BLUR_FIR) - R.blur(p)).max() / np.abs(p).max())
                              for p in planes)
    # the product planes p * p as the score forms them (blur_plane has no fp64 form: OR_BLUR_EXACT blurs products)
    for name, mode in (("fir", orc.BLUR_FIR), ("exact", orc.BLUR_EXACT)):
        out[f"blur_product {name} rel"] = max(
            float(np.abs(orc.blur_product(p, p, mode) - R.blur(p.astype(np.float64) ** 2)).max() / np.square(p).max())
            for p in planes)
    for name, mode in (("recursive", orc.BLUR_IIR), ("recursive_fma", orc.BLUR_IIR_FMA)):
        per = {}
        for n in (16, 64, 256, 1024, 4096):
            r = 0.0
            for shape in ((32, n), (n, 32)):
                for p in (rng.random(shape).astype(np.float32), (0.3 + 0.1 * rng.random(shape)).astype(np.float32)):
                    r = max(r, float(np.abs(orc.blur_plane(p, mode) - R.blur(p)).max() / np.abs(p).max()))
            per[n] = r / np.sqrt(n)
        out[f"blur {name} rel / sqrt(line)"] = per
    return out


PLANE_SIZES = [(121, 9), (333, 217), (1921, 1083), (3840, 2160)]


def plane_campaign():
    """The checker's intermediate planes (bit for bit the instrumented build's debug downloads) against the
    reference's, on the frames of tests/test_gpu_fp64_reference.py: pyramid levels in ulps, XYB absolute, the FIR
    blur of ref * ref and the recursive planes (both passes) relative to the plane's peak; the recursive ones also
    divided by sqrt(w + h)."""
    out = {}
    for w, h in PLANE_SIZES:
        ref = synth.make_ref(w, h, 5 * w + h)
        dist = synth.distort(ref, "blockq", 2, seed=4)
        ns = R.nscales_of(w, h)
        lv = fc.reference_levels(ref, dist, list(range(ns)))
        lut = orc.srgb_lut()
        lin = [np.ascontiguousarray(lut[f].transpose(2, 0, 1)) for f in (ref, dist)]
        r = {"lin ulps": 0.0, "xyb abs": 0.0, "fir blur rel": 0.0, "recursive V rel - per sqrt(w+h)": 0.0}
        for s in range(ns):
            if s:
                lin = [orc.downsample2(x) for x in lin]
                r["lin ulps"] = max(r["lin ulps"], fc.lin_ulps(lin[0], lv[s][0]), fc.lin_ulps(lin[1], lv[s][1]))
            x1, x2 = orc.linear_to_xyb(lin[0]), orc.linear_to_xyb(lin[1])
            r["xyb abs"] = max(r["xyb abs"], fc.abs_dev(x1, lv[s][2]))
            e1 = lv[s][2]
            for c in range(3):
                r["fir blur rel"] = max(r["fir blur rel"],
                                        fc.rel_dev(orc.blur_product(x1[c], x1[c], orc.BLUR_FIR), R.blur(e1[c] ** 2)))
            if s == 0:
                exp = fc.rg_reference(lv[0][2], lv[0][3], vertical=True)
                got = []
                for c in range(3):
                    a, b = x1[c], x2[c]
                    got += [orc.blur_plane(src, orc.BLUR_IIR) for src in (a, b, a * a, b * b, a * b)]
                dev = max(fc.rel_dev(g, e) for g, e in zip(got, exp))
                r["recursive V rel - per sqrt(w+h)"] = (dev - fc.RG_REL0) / np.sqrt(w + h)
        out[f"{w}x{h}"] = r
        print(f"  planes {w}x{h} done", file=sys.stderr)
    return out


def map_campaign():
    """tests/errmap_ref.py's fp32 map (bit for bit the device map) against the fp64 map of section 9, on the frames
    of tests/test_gpu_fp64_reference.py: per pixel relative to the peak, and the mean against sum w_i |a_i| where every
    scale tiles the frame."""
    import errmap_ref
    out = {}
    for w, h in ((128, 96), (131, 173), (640, 352)):
        ref = synth.make_ref(w, h, w * h)
        dist = synth.distort(ref, "blockq", 2, seed=7)
        m64, e = R.error_map(ref, dist)
        ns = e["nscales"]
        tiles = w % (1 << (ns - 1)) == 0 and h % (1 << (ns - 1)) == 0
        for mode, blur in (("fir", orc.BLUR_FIR), ("recursive", orc.BLUR_IIR)):
            avg = orc.compute_ssimu2(ref, dist, blur, return_averages=True)[1]
            m, _own, _ns = errmap_ref.reference_map(orc, ref, dist, blur, avg=avg)
            r = {"pixel / peak": float(np.abs(m - m64).max() / m64.max())}
            if tiles:
                r["mean rel"] = abs(m.mean(dtype=np.float64) - e["weighted_sum"]) / e["weighted_sum"]
            out[f"{w}x{h} {mode}"] = r
    return out


def hbd_map_cases():
    """fc.MAP_HBD_CASES (the frames of the tests) and a dozen more content16 pairs at depths 9..16, sizes up to
    640 x 352, every other one a multiple of 32 both ways so that the mean is measured too: -> [(w, h, depth, seed or
    None)]."""
    rng = np.random.default_rng(1016)
    more = []
    for i in range(12):
        w, h = int(rng.integers(8, 641)), int(rng.integers(8, 353))
        if i % 2 == 0:
            w, h = max(32, w // 32 * 32), max(32, h // 32 * 32)
        more.append((w, h, 9 + i % 8, 500 + i))
    return [c + (None,) for c in fc.MAP_HBD_CASES] + more


def hbd_map_campaign():
    """The fp32 map of 9- to 16-bit frames (hbd_ref.error_map_fp32: bit for bit the device map in the recursive modes,
    within MAP_K * 2^-24 of it in FIR) against hbd_ref.error_map_fp64, in fc.map_deviation's measures.  -> (per case,
    {(measure, mode): maximum}); fc.MAP_PIXEL_REL_HBD / MAP_MEAN_REL_HBD are the maxima times 2."""
    import hbd_ref
    out, worst = {}, {}
    for w, h, d, seed in hbd_map_cases():
        ref, dist = fc.map_hbd_pair(w, h, d, seed)
        m64, e = hbd_ref.error_map_fp64(ref, dist, d)
        for mode, blur in (("fir", orc.BLUR_FIR), ("recursive", orc.BLUR_IIR)):
            r = fc.map_deviation(hbd_ref.error_map_fp32(orc, ref, dist, d, blur)[0], m64, e)
            out[f"{w}x{h} {d}-bit {mode}"] = {k: v for k, v in r.items() if v is not None}
            for k, v in r.items():
                if v is not None:
                    worst[k, mode] = max(worst.get((k, mode), 0.0), v)
        print(f"  16-bit map {w}x{h} {d}-bit done", file=sys.stderr)
    return out, worst


def random_case(rng, i):
    w, h = (int(x) for x in rng.integers(1, 601, 2))
    kind = KINDS[i % len(KINDS)]
    ref = synth.make_ref(w, h, 1000 + i) if kind == "make_ref" else content(kind, w, h, 1000 + i)
    dk = DISTORTIONS[int(rng.integers(0, len(DISTORTIONS)))]
    st = int(rng.integers(1, 4))
    return f"{w}x{h} {kind} {dk}{st}", ref, synth.distort(ref, dk, st, seed=i)


def large_cases():
    for w, h in ((1920, 1080), (3840, 2160)):
        ref = synth.make_ref(w, h, w + h)
        for dk, st in (("blockq", 1), ("noise", 1), ("blur", 2)):
            yield f"{w}x{h} make_ref {dk}{st}", ref, synth.distort(ref, dk, st, seed=3)


def score_campaign(cases):
    worst = {}     # (mode, content class, size class, measure) -> (value, case)

    def note(key, val, what):
        if val > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (val, what)

    for what, ref, dist in cases:
        t = time.time()
        exp = R.evaluate(ref, dist)
        h, w, _ = ref.shape
        big = w * h >= 1920 * 1080
        natural = "make_ref" in what
        for mode, blur in MODES.items():
            s, avg, ns = orc.compute_ssimu2(ref, dist, blur, omp=big, return_averages=True)
            dev = fc.deviation(s, avg, ns, exp)
            cls = "1080p+" if big else ("small" if w * h <= fc.IIR_MAX_PIXELS else "medium")
            key = (mode, "natural" if natural else "synthetic", cls)
            if not dev["nscales_ok"]:
                note(key + ("nscales mismatch",), 1.0, what)
                continue
            note(key + ("term",), dev["term"], what)
            note(key + ("avg abs",), dev["avg_abs"], what)
            if exp["score"] > fc.NEAR_100:
                note(key + ("sum (near 100)",), dev["sum"], what)
            else:
                note(key + ("score",), dev["score"], what)
        print(f"  {what}: reference {exp['score']:.4f}  ({time.time() - t:.1f} s)", file=sys.stderr)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", type=int, nargs="?", default=200)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--hbd-maps", action="store_true", help="only the 16-bit error-map section")
    a = ap.parse_args()
    orc.build()
    if not a.no_stages and not a.hbd_maps:
        print("== stages: checker vs fp64 reference")
        for k, v in stage_campaign().items():
            print(f"  {k}: {v}")
        print("== planes: checker (= device) vs fp64 reference")
        for k, v in plane_campaign().items():
            print(f"  {k}: " + ", ".join(f"{m} {x:.3g}" for m, x in v.items()))
        print("== error map: fp32 map vs fp64 map")
        for k, v in map_campaign().items():
            print(f"  {k}: " + ", ".join(f"{m} {x:.3g}" for m, x in v.items()))
    if not a.no_stages or a.hbd_maps:
        print("== error map, 16-bit: fp32 map vs fp64 map")
        per_case, worst = hbd_map_campaign()
        for k, v in per_case.items():
            print(f"  {k}: " + ", ".join(f"{m} {x:.3g}" for m, x in v.items()))
        for (meas, mode), x in sorted(worst.items()):
            print(f"  maximum {meas} {mode}: {x:.3e}")
    if a.hbd_maps:
        return
    rng = np.random.default_rng(a.seed)
    cases = [random_case(rng, i) for i in range(a.cases)]
    if not a.no_large:
        cases += list(large_cases())
    print(f"== scores: {len(cases)} cases; largest deviation per mode, content class (natural: synth.make_ref; "
          f"synthetic: the five kinds of gpu_cases.content), size class and measure "
          f"(small: <= {fc.IIR_MAX_PIXELS} px, medium: below 1080p)")
    for (mode, kind, cls, meas), (val, what) in sorted(score_campaign(cases).items()):
        print(f"  {mode:14s} {kind:9s} {cls:7s} {meas:15s} {val:.3e}  [{what}]")


if __name__ == "__main__":
    main()
