"""Every scorer entry point against the checker in all three blur modes (-m gpu only).

The search path scores in SSIMU2_BLUR_RECURSIVE: libavif's RGB(A) rows through the strided hand-off against a
cached reference, often on several contexts.  Here each mode of the table in tests/gpu_cases.py is held to the
checker's evaluation of the same blur at the sizes where the kernels change shape (no scale, scale-count
transitions, FIR strip edges, recursive tile / batch edges, ragged, very tall and very wide), and every other entry
point -- cached reference, strided RGB(A) rows, device pointers, enqueue / wait, error maps -- must return the pair
score's bits.  Then extreme frames and content kinds, production-sized frames through the strided hand-off,
fan-out over contexts, and one long-lived context driven through sizes, modes and entry points against fresh
contexts.

Tolerances against the checker are those of tests/test_gpu_recursive.py (score 1e-4, relative beyond 100 points;
averages rtol 2e-5) and 5e-4 for frames that score far below 0 (test_extreme_frames).  Beyond them the pair scores are
held to the kernel-order terms (gpu_cases.check_against_terms: k_finalize to 1e-11, the averages to 1e-9 in the
recursive modes and to the FIR sums' derived bound), at production size too, and the error map pixel by pixel
(gpu_cases.check_map: bit for bit in the recursive modes, MAP_K * 2^-24 in FIR).
"""
import json
import os
import struct
import sys

import numpy as np
import pytest

from oavif_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_cases import (ATOL_AVG, MODES, RTOL_AVG, SIZES, TOL_FAR_BELOW_ZERO, check_against_terms,  # noqa: E402
                       check_fir_sums, check_map, content_pairs as _content_pairs, contexts_fixture, decoded_like,
                       extreme_pairs as _extreme_pairs, flat_pairs as _flat_pairs, march_seg_rows, pseudo_codec,
                       score_tol, seg_rows)
import errmap_ref  # noqa: E402

pytestmark = pytest.mark.gpu

RECURSIVE_MODES = ["recursive", "recursive_fma"]

_CHECKER = {}   # (mode, case) -> the checker's (score, averages, nscales)


def _bits(x: float) -> bytes:
    return struct.pack("<d", x)


def _checker(oracle, mode, case, ref, dist):
    key = (mode, case)
    if key not in _CHECKER:
        _CHECKER[key] = oracle.compute_ssimu2(ref, dist, MODES[mode][1], return_averages=True)
    return _CHECKER[key]


def _check_score(got, avg, ns, exp, avg_o, ns_o, what, tol=None):
    assert ns == ns_o, what
    assert np.allclose(avg, avg_o, rtol=RTOL_AVG, atol=ATOL_AVG), (what, np.abs(avg - avg_o).max())
    tol = score_tol(exp) if tol is None else tol
    assert abs(got - exp) <= tol, (what, got, exp)


def _on_device(*frames):
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(f)).cuda().contiguous() for f in frames]
    torch.cuda.synchronize()
    return ts


ctxs = contexts_fixture()   # one long-lived context per mode


# ---- 1. sizes x modes x entry points ----------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_entry_point_matches_the_checker(ctxs, oracle, mode, w, h):
    """(a) the pair score against the checker in that mode; (b) every other entry point returns its bits and its
    averages; (c) the error map against the numpy reference, the against-reference map bit for bit the pair map."""
    s = ctxs[mode]
    ref = synth.make_ref(w, h, 17 * w + h)
    dist = synth.distort(ref, "noise", 2, seed=w + 3 * h)
    got = s.compute_ssimu2(ref, dist)
    avg, ns = s.last_averages()
    exp, avg_o, ns_o = _checker(oracle, mode, (w, h), ref, dist)
    _check_score(got, avg, ns, exp, avg_o, ns_o, f"{mode} {w}x{h}")

    def same(what, score):
        a, n = s.last_averages()
        assert _bits(score) == _bits(got), (what, score, got)
        assert n == ns and np.array_equal(a.view(np.uint64), avg.view(np.uint64)), what

    s.set_reference(ref)
    same("score_against_reference", s.score_against_reference(dist))
    # RGBA rows without padding take k_unpack_rgb<true> when w % 4 == 0
    for channels, pad in ((4, 0), (4, 3), (3, 5)):
        buf, view = decoded_like(dist, channels, pad, seed=w * h + pad)
        same(f"strided {channels} ch + {pad}", s.score_decoded_against_reference(view))
        same(f"strided flat {channels} ch + {pad}",
             s.score_decoded_against_reference(buf.reshape(-1), row_bytes=buf.shape[1], channels=channels))

    t_ref, t_dist = _on_device(ref, dist)
    same("score_device", s.score_device(t_ref.data_ptr(), t_dist.data_ptr(), w, h))
    s.enqueue_device(t_ref.data_ptr(), t_dist.data_ptr(), w, h)
    same("enqueue_device", s.wait())
    s.set_reference_device(t_ref.data_ptr(), w, h)
    s.enqueue_against_reference_device(t_dist.data_ptr())
    same("enqueue_against_reference_device", s.wait())

    pair_score, pair_map = s.error_map(ref, dist)
    same("error_map", pair_score)
    s.set_reference(ref)
    ref_score, ref_map = s.error_map_against_reference(dist)
    same("error_map_against_reference", ref_score)
    assert np.array_equal(ref_map.view(np.uint32), pair_map.view(np.uint32))
    _worst, own = check_map(oracle, pair_map, avg, ns, ref, dist, MODES[mode][1], f"{mode} {w}x{h}")
    check_against_terms(oracle, got, avg, ns, ref, dist, mode, f"{mode} {w}x{h}", kavg=own)
    if min(w, h) < 8:   # no scale to score
        assert got == 100.0 and not pair_map.any()


# ---- 2. extreme frames and content kinds in the recursive modes --------------------------------------------------

GROUPS = ["extreme", "flat", "content-gradient", "content-primaries", "content-checker", "content-text",
          "content-noise"]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", RECURSIVE_MODES)
def test_extreme_frames_and_content_in_the_recursive_modes(ctxs, oracle, mode, group):
    s = ctxs[mode]
    pairs = {"extreme": _extreme_pairs, "flat": _flat_pairs}.get(group, lambda: _content_pairs(group[8:]))()
    for i, (ref, dist) in enumerate(pairs):
        got = s.compute_ssimu2(ref, dist)
        avg, ns = s.last_averages()
        exp, avg_o, ns_o = _checker(oracle, mode, (group, i), ref, dist)
        tol = TOL_FAR_BELOW_ZERO if exp < 0 else score_tol(exp)
        _check_score(got, avg, ns, exp, avg_o, ns_o, f"{mode} {group} {i}", tol)
        check_against_terms(oracle, got, avg, ns, ref, dist, mode, f"{mode} {group} {i}")
        if np.array_equal(ref, dist):
            assert got == 100.0
        s.set_reference(ref)
        assert _bits(s.score_against_reference(dist)) == _bits(got)


@pytest.mark.parametrize("mode", ["recursive", "fir"])
def test_a_4k_pair_against_the_kernel_order_terms(ctxs, oracle, mode):
    """One 3840 x 2160 pair in the search default and in FIR: the averages over 8.3 M terms per statistic within
    RTOL_RECURSIVE (the whole fp64 summation bound) or the FIR sums' bound at a 135-row segment, k_finalize to
    FINALIZE_TOL.  In FIR the d and d^4 averages are also held to the same terms summed in k_march's order
    (gpu_cases.check_fir_sums: 32 strips x 16 segments)."""
    s = ctxs[mode]
    ref = synth.make_ref(3840, 2160, seed=21)
    dist = synth.distort(ref, "blockq", 2, seed=22)
    got = s.compute_ssimu2(ref, dist)
    avg, ns = s.last_averages()
    assert ns == 6
    if mode != "fir":
        check_against_terms(oracle, got, avg, ns, ref, dist, mode, f"{mode} 3840x2160")
        return
    assert march_seg_rows(3840, 2160, 0) == 135
    rows = seg_rows(3840, 2160)
    kavg, ns_r, kord = errmap_ref.kernel_averages(oracle, ref, dist, MODES[mode][1], seg_rows=rows)
    assert ns_r == ns
    check_against_terms(oracle, got, avg, ns, ref, dist, mode, f"{mode} 3840x2160", kavg=kavg)
    check_fir_sums(avg, ns, 3840, 2160, kord, rows, f"{mode} 3840x2160")


# ---- 3. frames shaped like production: RGBA rows against a cached reference --------------------------------------

def _anchor_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "large_anchors.json")
    with open(path) as f:
        return [c for c in json.load(f)["cases"] if c["w"] * c["h"] <= 3840 * 2160]


def _anchor_frames(case):
    w, h = case["w"], case["h"]
    ref = synth.make_ref(w, h, case["seed"])
    crc = int(np.bitwise_xor.reduce(ref.reshape(-1).astype(np.uint32) * np.arange(1, ref.size + 1, dtype=np.uint32)
                                    & 0xFFFFFFFF))
    assert crc == case["ref_crc"], "synth.make_ref no longer regenerates the fixture's frame"
    return ref, synth.distort(ref, case["kind"], case["strength"], seed=case["seed"])


@pytest.mark.parametrize("case", _anchor_cases(), ids=lambda c: f"{c['w']}x{c['h']}-{c['kind']}{c['strength']}")
@pytest.mark.parametrize("mode", RECURSIVE_MODES)
def test_production_frames_through_the_strided_handoff(ctxs, mode, case):
    """set_reference, then libavif-like RGBA rows (row_bytes 4w and 4w + 64): the tight against-reference bits, which
    are the pair score's, within 1e-4 of the committed checker score of that recursion."""
    s = ctxs[mode]
    ref, dist = _anchor_frames(case)
    pair = s.compute_ssimu2(ref, dist)
    s.set_reference(ref)
    tight = s.score_against_reference(dist)
    avg, ns = s.last_averages()
    assert _bits(tight) == _bits(pair)
    for pad in (0, 64):
        _buf, view = decoded_like(dist, 4, pad, seed=case["seed"] + pad)
        assert _bits(s.score_decoded_against_reference(view)) == _bits(tight), pad
        a, n = s.last_averages()
        assert n == ns and np.array_equal(a.view(np.uint64), avg.view(np.uint64)), pad
    exp = case["score_iir" if mode == "recursive" else "score_iir_fma"]
    assert abs(tight - exp) <= 1e-4, (tight, exp)


# ---- 4. fan-out over contexts in the recursive modes --------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(960, 540), (641, 359)])
@pytest.mark.parametrize("mode", RECURSIVE_MODES)
def test_probe_fanout_in_the_recursive_modes(ctxs, mode, w, h):
    import oavif_amd
    s = ctxs[mode]
    ref = synth.make_ref(w, h, 81)
    dists = [synth.distort(ref, k, st, seed=st) for k, st in
             [("blockq", 0), ("blockq", 2), ("noise", 1), ("noise", 3), ("blur", 1), ("band", 2), ("blur", 3)]]
    seq = [s.compute_ssimu2(ref, d) for d in dists]
    t_ref, *t_d = _on_device(ref, *dists)
    fan_ctxs = [oavif_amd.Ssimu2(0, blur=MODES[mode][0]) for _ in range(3)]
    try:
        fan = oavif_amd.score_many(fan_ctxs, t_ref.data_ptr(), [t.data_ptr() for t in t_d], w, h)
    finally:
        for c in fan_ctxs:
            c.close()
    assert [_bits(x) for x in fan] == [_bits(x) for x in seq]


@pytest.mark.parametrize("w,h,tgt,fan", [(1920, 1080, 80.0, 4), (1920, 1080, 65.0, 6), (7680, 4320, 80.0, 4)])
def test_speculative_search_in_recursive_mode_equals_sequential(hip_lib, w, h, tgt, fan):
    """test_speculative_search_over_streams_equals_sequential with every context in the search path's default mode."""
    import oavif_amd
    from oavif_amd import tq
    ref = synth.make_ref(w, h, 77)
    codec = pseudo_codec(ref)
    with oavif_amd.Ssimu2(0, blur=_lib.BLUR_RECURSIVE) as scorer:
        seq = tq.search_hip(scorer, ref, codec, score_tgt=tgt)
    spec = [oavif_amd.Ssimu2(0, blur=_lib.BLUR_RECURSIVE) for _ in range(fan)]
    try:
        res, stats, sizes = tq.search_speculative_hip(spec, ref, codec, score_tgt=tgt)
    finally:
        for c in spec:
            c.close()
    assert (res.q, res.score, res.num_pass, res.buf_q) == (seq.q, seq.score, seq.num_pass, seq.buf_q)
    assert res.history == seq.history
    assert res.last_avif_size == seq.last_avif_size == 1000 + 10 * seq.buf_q
    assert stats.waves + stats.cache_hits == seq.num_pass and stats.waves <= seq.num_pass
    assert stats.probes_issued == len(sizes) <= stats.waves * fan


# ---- 5. history independence ------------------------------------------------------------------------------------

MODE_ORDER = ["fir", "recursive", "recursive_fma"]
HSIZES = {"S": (64, 64), "L": (1920, 1080), "T": (33, 17), "N": (7, 7)}

# (op, size, frame, layout).  "blur" k switches to MODE_ORDER[(start + k) % 3]; the six switches cover every ordered
# pair of modes from any start.  "gone": score_against_reference must raise ERR_NO_REFERENCE.  Every other step is
# compared with the same call on a fresh context (after set_reference / set_reference_device where it needs one).
SCRIPT = [
    ("pair", "S", 1), ("ref", "S"), ("against", "S", 1), ("strided", "S", 2, (4, 64)), ("map_against", "S", 1),
    ("pair", "L", 1), ("gone",),                              # a pair score that grows the buffers
    ("ref", "L"), ("strided", "L", 2, (4, 0)), ("against", "L", 1),   # a larger staging buffer than before
    ("blur", 1), ("gone",),
    ("ref_dev", "L"), ("dev_against", "L", 2), ("strided", "L", 1, (3, 5)),   # a smaller one
    ("map", "T", 1), ("gone",),                               # shrink
    ("score_dev", "L", 2),
    ("blur", 2),                                              # recursive <-> recursive_fma from start fir
    ("ref", "T"), ("against", "T", 2), ("strided", "T", 1, (4, 3)),
    ("blur", 1), ("gone",),
    ("ref", "S"), ("map_against", "S", 2),
    ("pair", "N", 1), ("map", "N", 2), ("ref", "N"), ("strided", "N", 1, (4, 0)),   # below 8 x 8
    ("blur", 0), ("gone",),
    ("enqueue_dev", "T", 1), ("map", "L", 1),
    ("ref", "S"), ("blur", 2), ("gone",),
    ("ref", "S"), ("against", "S", 1),
    ("blur", 0), ("gone",),
    ("pair", "L", 2), ("ref_dev", "S"), ("dev_against", "S", 2),
]

_HFRAMES = {}
_FRESH = {}


def _hframe(size, k):
    """frame k of a size: 0 the reference, 1 and 2 two distortions of it (host array, device tensor)."""
    if (size, k) not in _HFRAMES:
        w, h = HSIZES[size]
        ref = synth.make_ref(w, h, 5 * w + h)
        f = ref if k == 0 else synth.distort(ref, "blockq" if k == 1 else "noise", 2, seed=k)
        _HFRAMES[(size, k)] = (f, _on_device(f)[0])
    return _HFRAMES[(size, k)]


def _call(s, step, have_ref):
    """Run one step on `s` -> (score, averages, nscales, map or None).  `have_ref`: False on a fresh context, which
    gets the reference the step needs first."""
    op, size = step[0], step[1]
    w, h = HSIZES[size]
    ref, t_ref = _hframe(size, 0)
    dist, t_dist = _hframe(size, step[2])
    m = None
    if op in ("against", "strided", "map_against") and not have_ref:
        s.set_reference(ref)
    if op == "dev_against" and not have_ref:
        s.set_reference_device(t_ref.data_ptr(), w, h)
    if op == "pair":
        score = s.compute_ssimu2(ref, dist)
    elif op == "against":
        score = s.score_against_reference(dist)
    elif op == "strided":
        _buf, view = decoded_like(dist, *step[3], seed=w + h)
        score = s.score_decoded_against_reference(view)
    elif op == "map":
        score, m = s.error_map(ref, dist)
    elif op == "map_against":
        score, m = s.error_map_against_reference(dist)
    elif op == "score_dev":
        score = s.score_device(t_ref.data_ptr(), t_dist.data_ptr(), w, h)
    elif op == "enqueue_dev":
        s.enqueue_device(t_ref.data_ptr(), t_dist.data_ptr(), w, h)
        score = s.wait()
    elif op == "dev_against":
        s.enqueue_against_reference_device(t_dist.data_ptr())
        score = s.wait()
    else:
        raise AssertionError(op)
    avg, ns = s.last_averages()
    return score, avg, ns, m


def _fresh(mode, step):
    key = (mode,) + step
    if key not in _FRESH:
        from oavif_amd import Ssimu2
        with Ssimu2(0, blur=MODES[mode][0]) as s:
            _FRESH[key] = _call(s, step, False)
    return _FRESH[key]


@pytest.mark.parametrize("start", MODE_ORDER)
def test_one_context_through_sizes_modes_and_entry_points_equals_fresh_contexts(hip_lib, start):
    """One long-lived context grows (64 x 64 -> 1080p) and shrinks (-> 33 x 17 -> 7 x 7), switches among the three
    modes and interleaves pair scores, cached-reference scores, strided scores, device entry points and error maps:
    every score, every last_averages() and every map is bit for bit what a fresh context returns for that one call,
    and the cached reference is gone where the ABI drops it (a pair score, buffer growth, any set_blur)."""
    from oavif_amd import Ssimu2, Ssimu2Error
    k0 = MODE_ORDER.index(start)
    mode = start
    ref_size = None
    with Ssimu2(0, blur=MODES[start][0]) as s:
        for i, step in enumerate(SCRIPT):
            op = step[0]
            what = (start, i, mode) + step
            if op == "blur":
                mode = MODE_ORDER[(k0 + step[1]) % 3]
                s.set_blur(MODES[mode][0])
                continue
            if op == "gone":
                assert ref_size is not None, what
                with pytest.raises(Ssimu2Error) as ei:
                    s.score_against_reference(_hframe(ref_size, 1)[0])
                assert ei.value.code == _lib.ERR_NO_REFERENCE, what
                continue
            if op in ("ref", "ref_dev"):
                ref, t_ref = _hframe(step[1], 0)
                if op == "ref":
                    s.set_reference(ref)
                else:
                    s.set_reference_device(t_ref.data_ptr(), *HSIZES[step[1]])
                ref_size = step[1]
                continue
            if op in ("against", "strided", "map_against", "dev_against"):
                assert step[1] == ref_size, what
            score, avg, ns, m = _call(s, step, True)
            f_score, f_avg, f_ns, f_m = _fresh(mode, step)
            assert _bits(score) == _bits(f_score), (what, score, f_score)
            assert ns == f_ns and np.array_equal(avg.view(np.uint64), f_avg.view(np.uint64)), what
            if m is not None:
                assert np.array_equal(m.view(np.uint32), f_m.view(np.uint32)), what
