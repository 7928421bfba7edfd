"""One long-lived context against fresh ones across every entry-point family (-m gpu only).

The kernels are held to the checker elsewhere; what decides which kernel runs on which buffer is the host state of a
context: a dozen lazily grown allocations, each with a capacity and a validity rule of its own, and the flags have_ref,
ref_hbd, pending and cache_ref_blur.  A stale plane or a capacity that survived a free does not show on a fresh context,
so here the committed plans of tests/ctx_walk.py (300 steps each, coverage asserted by tests/test_ctx_walk_plan.py) drive
one context through 8-bit, 16-bit, strided, map, device, enqueue and batch calls, reference changes, mode switches and
refusals.  Every scoring step must have the bits of the same single call on a fresh context (score, all 108 averages,
the scale count, the map, every item of a batch), every refusal the code the model predicts.  The table of fresh
results is itself held to the checker with the existing helpers (test_fresh_results_match_the_checker), so agreeing
with a fresh context means being right.  No bound of its own: bit for bit, or the bounds of tests/gpu_cases.py,
tests/hbd_ref.py and tests/fp64_checks.py.

Measured on the MI355X: the 30 tests of this module take 6.3 s (the suite before it: 475 tests in 278 s); a 300-step walk
0.1 to 0.8 s including its 90 to 150 fresh contexts (about 1 ms each), the four walks side by side 0.1 s; the slowest case
is test_fresh_results_match_the_checker[fir-G], 1.0 s, most of it the CPU references.
"""
import threading

import numpy as np
import pytest

import ctx_walk as cw
import errmap_ref
import fp64_checks
import gpu_cases
import hbd_ref
from oavif_amd import Ssimu2, Ssimu2Error, _lib

pytestmark = pytest.mark.gpu

FRESH = cw.FreshTable()     # serial results of fresh contexts, shared by every test of the module
S = cw.Step


def run_plan(p, fresh=FRESH):
    with Ssimu2(0, instrumented=p[2], blur=gpu_cases.MODES[p[1]][0]) as s:
        return cw.walk(s, cw.committed_plan(p), p[1], p[2], fresh)


@pytest.mark.parametrize("p", cw.PLANS, ids=cw.plan_id)
def test_walk_equals_fresh_contexts(hip_lib, p):
    before = FRESH.created
    counts = run_plan(p)
    print(f"measured: {cw.plan_id(p)}: {counts}, {FRESH.created - before} fresh contexts")
    assert counts["steps"] == cw.PLAN_LENGTH and counts["scored"] > cw.PLAN_LENGTH // 3


# ---- the fresh table against the references ----------------------------------------------------------------------------
def fresh_result(mode, st, ref=None):
    model = cw.CtxModel(mode)
    model.ref = ref
    return FRESH.get(model, st)


@pytest.mark.parametrize("size", cw.SIZE_ORDER)
@pytest.mark.parametrize("mode", cw.MODE_NAMES)
def test_fresh_results_match_the_checker(hip_lib, oracle, mode, size):
    """One check per operation kind with the existing helpers; the other 8-bit entry points must return the pair
    score's bits (as tests/test_gpu_mode_matrix.py holds them on its own grid)."""
    w, h = cw.SIZES[size]
    blur = gpu_cases.MODES[mode][1]
    what = f"{mode} {size} {w}x{h}"
    ref, dist = cw.frame8(size, 0), cw.frame8(size, 1)
    # 8-bit scores and maps
    pair = fresh_result(mode, S("compute", size=size, k=1))
    mp = fresh_result(mode, S("error_map", size=size, k=1))
    _worst, own = gpu_cases.check_map(oracle, mp.map, mp.avg, mp.ns, ref, dist, blur, what)
    gpu_cases.check_against_terms(oracle, pair.score, pair.avg, pair.ns, ref, dist, mode, what, kavg=own)
    for kind in ("8h", "8d"):
        r8 = cw.Ref(size, kind, 8, True)
        for st in (S("score_device", size=size, k=1), S("enqueue_device", size=size, k=1),
                   S("score_against", size=size, k=1), S("enqueue_against_device", size=size, k=1),
                   S("score_decoded", size=size, k=1, layout=cw.LAYOUTS8[1])):
            got = fresh_result(mode, st, r8 if cw.FAMILY[st.op] in cw.AGAINST_FAMILIES else None)
            cw.same_result(got, pair, (what, st.op, kind))
    cw.same_result(mp._replace(map=None), pair, (what, "error_map's score"))
    cw.same_result(fresh_result(mode, S("error_map_against", size=size, k=1), cw.Ref(size, "8h", 8, True)), mp,
                   (what, "error_map_against"))
    # 16-bit scores: a pair at depth 12, and the mixed pair (reference at depth 12, frame at depth 10)
    d_ref, d_dist = cw.MIXED
    r16 = cw.frame16(size, 0, d_ref)
    for st, r, d16, dd in ((S("compute_hbd", size=size, k=1, depth=d_ref), None, cw.frame16(size, 1, d_ref), d_ref),
                           (S("score_against_hbd", size=size, k=1, depth=d_dist), cw.Ref(size, "16", d_ref, True),
                            cw.frame16(size, 1, d_dist), d_dist)):
        got = fresh_result(mode, st, r)
        exp, avg_r, ns_r = hbd_ref.compute(oracle, r16, d16, d_ref, blur, d_dist=dd)
        assert got.ns == ns_r, (what, st.op)
        assert abs(got.score - exp) <= gpu_cases.score_tol(exp), (what, st.op, got.score, exp)
        assert np.allclose(got.avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), (what, st.op)
        # fp64_checks has no bound for the recursive modes beyond IIR_MAX_PIXELS (the recursion's own noise)
        if mode == "fir" or w * h <= fp64_checks.IIR_MAX_PIXELS:
            fp64_checks.check(got.score, got.avg, got.ns, hbd_ref.compute_fp64(r16, d16, d_ref, d_dist=dd), mode,
                              (what, st.op), "synthetic")
        gpu_cases.check_against_terms(oracle, got.score, got.avg, got.ns, r16, d16, mode, f"{what} {st.op}", kavg=avg_r)
    strided = fresh_result(mode, S("score_decoded_hbd", size=size, k=1, layout=cw.LAYOUTS16[2], depth=d_dist),
                           cw.Ref(size, "16", d_ref, True))
    cw.same_result(strided, got, (what, "score_decoded_hbd"))
    # batch items (FIR only)
    if mode != "fir":
        return
    n = 3
    refs, dists = cw.batch_pairs(size, n)
    against = cw.batch_dists(size, n)
    r8 = cw.Ref(size, "8h", 8, True)
    forms = [(S("score_batch", size=size, n=n), None, list(zip(refs, dists))),
             (S("score_batch_device", size=size, n=n), None, list(zip(refs, dists))),
             (S("score_batch_against", size=size, n=n), r8, [(ref, d) for d in against]),
             (S("score_batch_against_device", size=size, n=n), r8._replace(kind="8d"), [(ref, d) for d in against])]
    kavgs = {}
    for st, r, pairs in forms:
        got = fresh_result(mode, st, r)
        for i, (a, b) in enumerate(pairs):
            key = (id(a), id(b))
            if key not in kavgs:
                kavgs[key] = errmap_ref.kernel_averages(oracle, a, b, oracle.BLUR_FIR)
            kavg, ns_r = kavgs[key]
            avg, ns = got.items[i]
            assert ns == ns_r, (what, st.op, i)
            gpu_cases.check_item_against_terms(oracle, got.score[i], avg, ns, a, b, f"{what} {st.op} item {i}", kavg=kavg)


# ---- four contexts side by side ------------------------------------------------------------------------------------------
SIDE_BY_SIDE = [cw.PLANS[0], cw.PLANS[3], cw.PLANS[4], cw.PLANS[5]]     # four plans: fir, recursive, recursive_fma twice


def test_four_walks_side_by_side(hip_lib):
    """Four plans on four contexts from four threads at once (ctypes calls release the GIL; the contexts share the
    process-wide tables and the stream pool): every step of every walk has the bits of the serial fresh table."""
    for p in SIDE_BY_SIDE:
        FRESH.prefetch(cw.committed_plan(p), p[1], p[2])
    ctxs = [Ssimu2(0, blur=gpu_cases.MODES[p[1]][0]) for p in SIDE_BY_SIDE]
    barrier = threading.Barrier(len(ctxs))
    results, errors = [None] * len(ctxs), []

    def work(i):
        p = SIDE_BY_SIDE[i]
        try:
            barrier.wait(timeout=60)
            results[i] = cw.walk(ctxs[i], cw.committed_plan(p), p[1], p[2], FRESH)
        except BaseException as e:   # surfaced on the main thread
            errors.append((cw.plan_id(p), e))
    FRESH.frozen = True     # the threads only read the table
    try:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(ctxs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        FRESH.frozen = False
        for c in ctxs:
            c.close()
    assert not errors, errors
    assert all(r is not None and r["steps"] == cw.PLAN_LENGTH for r in results), results


# ---- an enqueued, unwaited score ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODE_NAMES)
def test_enqueued_score_rules(hip_lib, mode):
    """ssimu2_wait with nothing enqueued and ssimu2_ctx_set_blur while a score is enqueued are refused with
    SSIMU2_ERR_INVALID_ARG; the refused set_blur leaves the mode and the reference alone, and the wait that follows
    returns the score."""
    size = "T"
    w, h = cw.SIZES[size]
    ref, dist = cw.dev8(size, 0), cw.dev8(size, 1)
    exp = fresh_result(mode, S("enqueue_against_device", size=size, k=1), cw.Ref(size, "8d", 8, True))
    exp2 = fresh_result(mode, S("score_against", size=size, k=2), cw.Ref(size, "8d", 8, True))
    pair = fresh_result(mode, S("enqueue_device", size=size, k=1))

    def refused(call):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID_ARG

    with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as s:
        refused(s.wait)                                   # a new context
        s.set_reference_device(ref.data_ptr(), w, h)
        refused(s.wait)                                   # setting a reference enqueues no score
        s.enqueue_against_reference_device(dist.data_ptr())
        for m in cw.MODE_NAMES:                           # the current mode included
            refused(lambda: s.set_blur(gpu_cases.MODES[m][0]))
        score = s.wait()
        cw.same_result(cw.Result(score, *s.last_averages(), None, None), exp, (mode, "wait after the refused set_blur"))
        refused(s.wait)                                   # the score was waited for
        # mode and reference are as they were
        again = s.score_against_reference(cw.frame8(size, 2))
        cw.same_result(cw.Result(again, *s.last_averages(), None, None), exp2, (mode, "the reference is still live"))
        # the pair form: same rule
        s.enqueue_device(ref.data_ptr(), dist.data_ptr(), w, h)
        refused(lambda: s.set_blur(_lib.BLUR_FIR))
        cw.same_result(cw.Result(s.wait(), *s.last_averages(), None, None), pair, (mode, "pair form"))
        refused(s.wait)
        s.set_blur(gpu_cases.MODES[mode][0])              # nothing enqueued: accepted
