"""The committed plans of tests/ctx_walk.py fulfil their coverage conditions, and CtxModel says what the header says
(CPU only: plans and model need no GPU).  tests/test_gpu_ctx_walk.py executes these plans; a plan that stopped covering
an ordered pair of families, a kind of reference or a refusal would let it pass while exercising less."""
import pytest

import ctx_walk as cw
from oavif_amd import _lib

PRODUCT = [p for p in cw.PLANS if not p[2]]
INSTRUMENTED = [p for p in cw.PLANS if p[2]]


def replay(p):
    """-> (steps, the conditions the plan fulfils, refused steps) with the model run anew over the plan."""
    steps = cw.committed_plan(p)
    model, prev, met, refused = cw.CtxModel(p[1], p[2]), None, set(), 0
    for st in steps:
        assert model.predict(st) == (st.expect, st.kind), st
        met.update(cw.step_goals(model, prev, st))
        refused += st.expect is not None or st.poke is not None
        model.apply(st)
        prev = cw.FAMILY[st.op]
    return steps, met, refused


def union(plans):
    return set().union(*(replay(p)[1] for p in plans))


def test_the_committed_set():
    assert len(PRODUCT) == 6 and len(INSTRUMENTED) == 2
    assert sorted(p[1] for p in PRODUCT) == sorted(cw.MODE_NAMES * 2)
    assert len({p[:2] for p in PRODUCT}) == 6
    for p in cw.PLANS:
        assert len(cw.committed_plan(p)) == cw.PLAN_LENGTH >= 300
        assert cw.plan(*p, length=cw.PLAN_LENGTH) == cw.committed_plan(p), "a plan is a function of its arguments"


@pytest.mark.parametrize("p", cw.PLANS, ids=cw.plan_id)
def test_every_operation_occurs_in_every_plan(p):
    steps, met, _ = replay(p)
    ops = {st.op for st in steps}
    assert ops == {op for op in cw.OPS if p[2] or op != "cache_blur"}
    assert {st.arg for st in steps if st.op == "set_blur"} == set(cw.MODE_NAMES)     # the current mode included
    assert ("blur_to_current",) in met
    if p[2]:
        assert {st.arg for st in steps if st.op == "cache_blur"} == {True, False}
    # sizes, depths, layouts and batch sizes: all of them
    assert {st.size for st in steps if st.size} == set(cw.SIZES)
    assert {st.depth for st in steps if st.depth} == set(cw.DEPTHS)
    assert {st.layout for st in steps if st.op == "score_decoded"} == set(cw.LAYOUTS8)
    assert {st.layout for st in steps if st.op == "score_decoded_hbd"} == set(cw.LAYOUTS16)
    assert {st.n for st in steps if st.n} == set(cw.BATCH_N)
    assert ("mixed_depth",) in met      # a 16-bit frame at a depth other than its 16-bit reference's


def test_every_ordered_pair_of_families_is_adjacent_somewhere():
    met = union(PRODUCT)
    missing = [(a, b) for a in cw.PRODUCT_FAMILIES for b in cw.PRODUCT_FAMILIES if ("adj", a, b) not in met]
    assert len(cw.PRODUCT_FAMILIES) == 13 and not missing, missing
    met = union(INSTRUMENTED)
    missing = [(a, b) for a in cw.FAMILIES for b in cw.FAMILIES
               if "cache_blur" in (a, b) and ("adj", a, b) not in met]
    assert not missing, missing


def test_every_against_family_meets_every_kind_of_reference():
    """... in each mode where that is legal, set at a smaller and at a larger size than the reference before it."""
    met = union(PRODUCT)
    cells = [g for g in cw.all_goals(False) if g[0] == "cell"]
    assert len(cells) == 90      # 4 families x 3 kinds x 3 modes x 2, maps 2 kinds, batches FIR only
    assert not [g for g in cells if g not in met]


@pytest.mark.parametrize("p", cw.PLANS, ids=cw.plan_id)
def test_refusals_stay_below_a_quarter(p):
    steps, _, refused = replay(p)
    assert 0 < refused <= len(steps) // 4, refused


def test_every_refusal_kind_occurs():
    met = union(PRODUCT)
    assert not [g for g in cw.refusal_goals(False) if ("refusal",) + g not in met]
    met = union(INSTRUMENTED)
    assert not [g for g in cw.refusal_goals(True) if ("refusal",) + g not in met]
    codes = {st.kind: st.expect for p in cw.PLANS for st in cw.committed_plan(p) if st.kind}
    assert codes == {"no_reference": _lib.ERR_NO_REFERENCE, "batch_recursive": _lib.ERR_UNSUPPORTED,
                     "map_against_16": _lib.ERR_UNSUPPORTED, "uncached_16": _lib.ERR_OOM}


def test_every_ordered_pair_of_modes_is_switched_with_a_live_reference():
    met = union(PRODUCT)
    assert not [(a, b) for a in cw.MODE_NAMES for b in cw.MODE_NAMES if ("switch", a, b) not in met]


# ---- the model on hand-written sequences -----------------------------------------------------------------------------
S = cw.Step
REF8, REF8D, REF16 = S("set_reference", size="T"), S("set_reference_device", size="T"), S("set_reference_hbd", size="T", depth=12)
AGAINST = [S("score_against", size="T", k=1), S("enqueue_against_device", size="T", k=1),
           S("score_decoded", size="T", k=1, layout=(4, 3)), S("error_map_against", size="T", k=1),
           S("score_against_hbd", size="T", k=1, depth=10), S("score_decoded_hbd", size="T", k=1, layout=(4, 2), depth=16),
           S("score_batch_against", size="T", n=3), S("score_batch_against_device", size="T", n=3)]
PAIRS = [S("compute", size="S", k=1), S("score_device", size="S", k=1), S("enqueue_device", size="S", k=1),
         S("error_map", size="S", k=2), S("compute_hbd", size="S", k=1, depth=16)]
BATCHES = [S("score_batch", size="E", n=3), S("score_batch_device", size="E", n=17)] + AGAINST[-2:]


def test_model_every_against_call_needs_a_reference():
    m = cw.CtxModel()
    for st in AGAINST:
        assert m.apply(st) == (_lib.ERR_NO_REFERENCE, "no_reference"), st
    assert m.ref is None and m.last_single is None and m.last_batch is None


@pytest.mark.parametrize("ref", [REF8, REF8D, REF16], ids=["host", "device", "16bit"])
def test_model_keeps(ref):
    m = cw.CtxModel()
    assert m.apply(ref) == (None, None)
    live = m.ref
    assert live == cw.Ref("T", {REF8: "8h", REF8D: "8d", REF16: "16"}[ref], 12 if ref is REF16 else 8, True)
    for st in AGAINST + BATCHES[:2]:
        code = m.apply(st)
        if st.op == "error_map_against" and ref is REF16:
            assert code == (_lib.ERR_UNSUPPORTED, "map_against_16")
        else:
            assert code == (None, None), st
        assert m.ref is live, st
    assert m.last_batch == BATCHES[1] and m.last_single == AGAINST[5]


@pytest.mark.parametrize("drop", PAIRS + [S("set_blur", arg="fir"), S("set_blur", arg="recursive")], ids=lambda s: f"{s.op}-{s.arg}")
def test_model_drops(drop):
    for ref in (REF8, REF8D, REF16):
        m = cw.CtxModel()
        m.apply(ref)
        assert m.apply(drop) == (None, None)
        assert m.ref is None
        assert m.apply(AGAINST[0]) == (_lib.ERR_NO_REFERENCE, "no_reference")
        assert m.mode == (drop.arg or "fir")


def test_model_replaces_and_tells_growth_from_shrinkage():
    m = cw.CtxModel("recursive")
    m.apply(S("set_reference", size="M"))
    assert m.ref_rel is None
    m.apply(S("set_reference_hbd", size="G", depth=10))
    assert (m.ref.size, m.ref.kind, m.ref.depth, m.ref_rel) == ("G", "16", 10, "larger")
    m.apply(S("compute", size="S", k=1))          # dropped, but its buffers were sized by G
    m.apply(S("set_reference_device", size="N"))
    assert (m.ref.size, m.ref.kind, m.ref_rel) == ("N", "8d", "smaller")
    m.apply(S("set_reference", size="N"))
    assert m.ref_rel is None and m.ref.kind == "8h"


def test_model_batches_in_the_recursive_modes():
    for mode in ("recursive", "recursive_fma"):
        m = cw.CtxModel(mode)
        for st in BATCHES:      # checked before the reference: UNSUPPORTED also without one
            assert m.apply(st) == (_lib.ERR_UNSUPPORTED, "batch_recursive")
        m.apply(REF8)
        for st in BATCHES:
            assert m.apply(st) == (_lib.ERR_UNSUPPORTED, "batch_recursive")
        assert m.ref is not None and m.last_batch is None
        m.apply(S("set_blur", arg="fir"))
        assert m.apply(BATCHES[0]) == (None, None) and m.apply(BATCHES[2]) == (_lib.ERR_NO_REFERENCE, "no_reference")


def test_model_the_blur_cache_of_the_instrumented_build():
    with pytest.raises(ValueError):
        cw.CtxModel().predict(S("cache_blur", arg=False))
    m = cw.CtxModel("fir", instrumented=True)
    m.apply(REF8)
    assert m.apply(S("cache_blur", arg=False)) == (None, None) and m.ref is None     # the hook drops the reference
    assert m.apply(REF16) == (_lib.ERR_OOM, "uncached_16") and m.ref is None
    m.apply(REF8)
    assert m.ref.cached is False
    for st in AGAINST:
        exp = (_lib.ERR_OOM, "uncached_16") if "hbd" in st.op else (None, None)
        assert m.apply(st) == exp, st
        assert m.ref is not None
    m.apply(S("set_blur", arg="recursive"))       # the recursive modes have caches of their own
    assert m.apply(REF16) == (None, None) and m.apply(AGAINST[4]) == (None, None)
    m.apply(S("set_blur", arg="fir"))
    m.apply(S("cache_blur", arg=True))
    assert m.apply(REF16) == (None, None) and m.ref.cached and m.apply(AGAINST[5]) == (None, None)


def test_model_refusals_change_nothing():
    m = cw.CtxModel()
    m.apply(REF16)
    m.apply(AGAINST[0])
    before = (m.mode, m.ref, m.last_single, m.last_batch)
    assert m.apply(AGAINST[3])[0] == _lib.ERR_UNSUPPORTED
    assert (m.mode, m.ref, m.last_single, m.last_batch) == before
