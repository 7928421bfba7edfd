"""A model-based history test of one ssimu2_ctx: frames, operations, a plain model of what include/ssimu2_hip.h promises
about the blur mode and the cached reference (CtxModel), a seeded plan generator, and the executor that drives a context
through a plan and holds every step to a fresh context (walk).  Importing this module, generating plans and running the
model need no GPU; tests/test_ctx_walk_plan.py asserts the coverage of the committed plans (PLANS) on the CPU,
tests/test_gpu_ctx_walk.py executes them.

Nothing here has a tolerance: a step on the long-lived context either has the bits of the same single call on a fresh
context, or is refused with the code the model predicts."""
from __future__ import annotations

import random
import threading
from collections import namedtuple

import numpy as np

import gpu_cases
from hbd_cases import hbd_distort, lift, rows16, to_depth
from oavif_amd import _lib, synth

# ---- frames ----------------------------------------------------------------------------------------------------------
# the smallest sizes at which each buffer rule and kernel shape changes
SIZES = {"N": (7, 7),        # no scale: score 100, zero map, nothing launched but finalize
         "T": (33, 17),      # two scales, odd
         "S": (64, 64),      # one recursive tile exactly; w % 4 == 0: RGBA rows take the fast unpack
         "E": (121, 41),     # one column past a 120-column FIR strip
         "M": (333, 217),    # ragged, all six scales
         "G": (641, 359)}    # larger than every other: grows every buffer; w % 4 != 0
SIZE_ORDER = sorted(SIZES, key=lambda z: SIZES[z][0] * SIZES[z][1])
DEPTHS = (10, 12, 16)
LAYOUTS8 = ((4, 0), (4, 3), (3, 5))      # (channels, pad bytes) of gpu_cases.decoded_like
LAYOUTS16 = ((4, 0), (4, 2), (3, 3))     # (channels, pad samples) of hbd_cases.rows16: 0, 4 and 6 bytes, all even
BATCH_N = (1, 3, 17)
MODE_NAMES = ("fir", "recursive", "recursive_fma")
MIXED = (12, 10)    # the mixed pair: the reference at depth 12, the distorted frame at depth 10

_HOST = {}
_DEV = {}
_LOCK = threading.RLock()     # re-entrant: a frame is made from other frames


def _memo(store, key, make):
    with _LOCK:
        if key not in store:
            store[key] = make()
        return store[key]


def frame8(size, k):
    """Frame k of a size as (h, w, 3) uint8: 0 the reference, 1 and 2 two distortions of it."""
    def make():
        w, h = SIZES[size]
        ref = synth.make_ref(w, h, 5 * w + h)
        return ref if k == 0 else synth.distort(ref, "blockq" if k == 1 else "noise", 2, seed=k)
    return _memo(_HOST, ("u8", size, k), make)


def frame16(size, k, depth):
    """Frame k of a size as (h, w, 3) uint16 of `depth` bits: 0 the 8-bit reference scaled to the depth with low-order
    detail added, 1 hbd_distort of it, 2 the second 8-bit distortion lifted (257 u) and cut down to the depth."""
    def make():
        w, h = SIZES[size]
        if k == 2:
            return np.ascontiguousarray(lift(frame8(size, 2)) >> np.uint16(16 - depth))
        ref = to_depth(frame8(size, 0), depth, 1000 * depth + w + h)
        return ref if k == 0 else np.ascontiguousarray(hbd_distort(ref, depth, seed=depth + k))
    return _memo(_HOST, ("u16", size, k, depth), make)


def strided8(size, k, layout):
    w, h = SIZES[size]
    return _memo(_HOST, ("s8", size, k, layout), lambda: gpu_cases.decoded_like(frame8(size, k), *layout, seed=w + h))


def strided16(size, k, layout, depth):
    w, h = SIZES[size]
    return _memo(_HOST, ("s16", size, k, layout, depth),
                 lambda: rows16(frame16(size, k, depth), *layout, seed=w + h + depth))


def batch_pairs(size, n):
    """The n pairs of a pair batch, drawn from the size's frames: every third pair scores one distortion against the
    other."""
    refs, dists = [], []
    for i in range(n):
        refs.append(frame8(size, 1 if i % 3 == 2 else 0))
        dists.append(frame8(size, 2 if i % 3 == 2 else 1 + i % 2))
    return refs, dists


def batch_dists(size, n):
    """The n frames of a batch against the reference: the two distortions and the reference itself in turn."""
    return [frame8(size, (1, 2, 0)[i % 3]) for i in range(n)]


def item_stride(size):
    """Bytes between the items of the device forms: a multiple of 4 that is no multiple of 16."""
    w, h = SIZES[size]
    stride = ((w * h * 3 + 3) & ~3) + 4
    return stride + 4 if stride % 16 == 0 else stride


def dev8(size, k):
    """frame8 on the device (a torch tensor; its data_ptr() is the device address)."""
    def make():
        import torch
        t = torch.from_numpy(frame8(size, k)).cuda().contiguous()
        torch.cuda.synchronize()
        return t
    return _memo(_DEV, (size, k), make)


def dev_items(size, n, which):
    """n items `item_stride` apart on the device, noise between them: `which` = "refs" / "dists" of batch_pairs, or
    "against" (batch_dists)."""
    def make():
        import torch
        frames = batch_dists(size, n) if which == "against" else batch_pairs(size, n)[which == "dists"]
        stride = item_stride(size)
        g = torch.Generator().manual_seed(n + stride)
        buf = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, generator=g)
        for i, f in enumerate(frames):
            buf[i * stride:i * stride + f.size] = torch.from_numpy(f.reshape(-1))
        t = buf.cuda()
        torch.cuda.synchronize()
        return t
    return _memo(_DEV, (size, n, which), make)


# ---- operations --------------------------------------------------------------------------------------------------------
FAMILY = {
    "compute": "pair8", "score_device": "pair8", "enqueue_device": "pair8",
    "error_map": "map_pair",
    "set_reference": "ref8", "set_reference_device": "ref8",
    "score_against": "against8", "enqueue_against_device": "against8",
    "score_decoded": "strided8",
    "error_map_against": "map_against",
    "compute_hbd": "pair16",
    "set_reference_hbd": "ref16",
    "score_against_hbd": "against16",
    "score_decoded_hbd": "strided16",
    "score_batch": "batch_pair", "score_batch_device": "batch_pair",
    "score_batch_against": "batch_against", "score_batch_against_device": "batch_against",
    "set_blur": "blur",
    "cache_blur": "cache_blur",     # instrumented contexts only
}
OPS = list(FAMILY)
FAMILIES = list(dict.fromkeys(FAMILY.values()))
PRODUCT_FAMILIES = [f for f in FAMILIES if f != "cache_blur"]
PAIR_FAMILIES = ("pair8", "map_pair", "pair16")
AGAINST_FAMILIES = ("against8", "strided8", "map_against", "against16", "strided16", "batch_against")
BATCH_FAMILIES = ("batch_pair", "batch_against")
REF_KINDS = ("8h", "8d", "16")     # set_reference, set_reference_device, set_reference_hbd
ENQUEUE_OPS = ("enqueue_device", "enqueue_against_device")

# op: the call; size, k: the frame; layout: of the strided calls; depth: of the 16-bit calls; n: items of a batch;
# arg: the mode of set_blur, the flag of cache_blur; poke: "wait" = a wait with nothing enqueued before the call,
# a mode name = set_blur to it between an enqueue and its wait (both refused, the step itself is not);
# expect / kind: the model's prediction when the plan was made (None = succeeds)
Step = namedtuple("Step", "op size k layout depth n arg poke expect kind", defaults=(None,) * 9)
Ref = namedtuple("Ref", "size kind depth cached")
Result = namedtuple("Result", "score avg ns map items")


def legal_cell(fam, kind, mode):
    """May `fam` score against a reference of `kind` in `mode`?"""
    if fam == "map_against" and kind == "16":
        return False
    return fam != "batch_against" or mode == "fir"


class CtxModel:
    """What the header promises about the host state of one context, and nothing about its buffers: the table of
    DESIGN.md section 3 ("Which call touches which buffer") is what this model abstracts.

    State: the blur mode; the reference (none, or its size, the call that set it -- "8h" host, "8d" device, "16"
    16-bit samples -- its depth and whether the blur cache was on when it was set); the last single-score step and
    the last batch step (whose results last_averages / last_batch_averages keep); the instrumented build's cache
    flag.  predict(step) -> (error code or None, refusal kind or None) without changing the state, apply(step)
    the same and moves the state on.

    Reference life: dropped by every pair-type score (pair8, map_pair, pair16), by every set_blur and by the
    instrumented build's cache_reference_blur; replaced by ref8 / ref16; kept by every against-type call, both batch
    forms and the map pass.  A refused ssimu2_set_reference_rgb16 leaves no reference."""

    def __init__(self, mode="fir", instrumented=False):
        assert mode in MODE_NAMES
        self.mode, self.instrumented, self.cache = mode, bool(instrumented), True
        self.ref = None
        self.ref_rel = None          # the live reference against the one set before it: "larger" / "smaller" / None
        self.last_ref_size = None    # size of the last reference set, live or not
        self.last_single = self.last_batch = None

    def predict(self, st):
        fam = FAMILY[st.op]
        if fam == "cache_blur" and not self.instrumented:
            raise ValueError("cache_blur needs an instrumented context")
        if fam in BATCH_FAMILIES and self.mode != "fir":        # checked before the reference
            return _lib.ERR_UNSUPPORTED, "batch_recursive"
        if fam in AGAINST_FAMILIES:
            if self.ref is None:
                return _lib.ERR_NO_REFERENCE, "no_reference"
            if fam == "map_against" and self.ref.kind == "16":
                return _lib.ERR_UNSUPPORTED, "map_against_16"
            if fam in ("against16", "strided16") and self.mode == "fir" and not self.ref.cached:
                return _lib.ERR_OOM, "uncached_16"
        if fam == "ref16" and self.mode == "fir" and not self.cache:
            return _lib.ERR_OOM, "uncached_16"
        return None, None

    def apply(self, st):
        code, kind = self.predict(st)
        fam = FAMILY[st.op]
        if fam == "blur":
            self.mode, self.ref = st.arg, None
        elif fam == "cache_blur":
            self.cache, self.ref = bool(st.arg), None
        elif fam in ("ref8", "ref16"):
            self.ref = None
            if code is None:
                rk = {"set_reference": "8h", "set_reference_device": "8d", "set_reference_hbd": "16"}[st.op]
                self.ref = Ref(st.size, rk, st.depth if rk == "16" else 8, self.cache)
                a, b = SIZE_ORDER.index(st.size), None if self.last_ref_size is None else SIZE_ORDER.index(self.last_ref_size)
                self.ref_rel = None if b is None or a == b else "larger" if a > b else "smaller"
                self.last_ref_size = st.size
        elif code is None:
            if fam in PAIR_FAMILIES:
                self.ref = None
            if fam in BATCH_FAMILIES:
                self.last_batch = st
            else:
                self.last_single = st
        return code, kind


# ---- plans -------------------------------------------------------------------------------------------------------------
def refusal_goals(instrumented):
    """Every (refusal kind, op) the plans must provoke."""
    out = [("no_reference", op) for op in OPS if FAMILY[op] in AGAINST_FAMILIES]
    out += [("batch_recursive", op) for op in OPS if FAMILY[op] in BATCH_FAMILIES]
    out += [("map_against_16", "error_map_against"), ("wait_idle", None), ("blur_enqueued", None)]
    if instrumented:
        out += [("uncached_16", op) for op in ("set_reference_hbd", "score_against_hbd", "score_decoded_hbd")]
    return out


def step_goals(model, prev_family, st):
    """The coverage conditions of tests/test_ctx_walk_plan.py the step `st` would fulfil after `prev_family` with the
    context as `model` has it."""
    fam = FAMILY[st.op]
    code, kind = model.predict(st)
    out = [("op", st.op)]
    if prev_family is not None:
        out.append(("adj", prev_family, fam))
    if code is not None:
        out.append(("refusal", kind, st.op))
    elif fam in AGAINST_FAMILIES:
        if model.ref_rel is not None:
            out.append(("cell", fam, model.ref.kind, model.mode, model.ref_rel))
        if fam == "against16" and model.ref.kind == "16" and st.depth != model.ref.depth:
            out.append(("mixed_depth",))
    if fam == "blur":
        out.append(("blur_to", st.arg))
        if st.arg == model.mode:
            out.append(("blur_to_current",))
        if model.ref is not None:
            out.append(("switch", model.mode, st.arg))
    if fam == "cache_blur":
        out.append(("cache", bool(st.arg)))
    if st.poke == "wait":
        out.append(("refusal", "wait_idle", None))
    elif st.poke is not None:
        out.append(("refusal", "blur_enqueued", None))
    return out


def all_goals(instrumented):
    fams = FAMILIES if instrumented else PRODUCT_FAMILIES
    goals = [("op", op) for op in OPS if instrumented or op != "cache_blur"]
    goals += [("adj", a, b) for a in fams for b in fams]
    goals += [("cell", f, k, m, r) for f in AGAINST_FAMILIES for k in REF_KINDS for m in MODE_NAMES
              for r in ("smaller", "larger") if legal_cell(f, k, m)]
    goals += [("refusal",) + g for g in refusal_goals(instrumented)]
    goals += [("switch", a, b) for a in MODE_NAMES for b in MODE_NAMES]
    goals += [("blur_to", m) for m in MODE_NAMES] + [("blur_to_current",), ("mixed_depth",)]
    if instrumented:
        goals += [("cache", True), ("cache", False)]
    return goals


MAX_REFUSED = 0.2    # share of a plan's steps that may be refusals or carry a refused poke (the condition is a quarter)


def plan(seed, start_mode, instrumented, length=300):
    """A seeded plan of `length` steps for a context that starts in `start_mode`.  Greedy: of some forty drawn
    candidates the next step is the one that fulfils the most coverage conditions not yet met by this plan (weights
    drawn per plan, so that plans of different seeds go different ways), refusals only while they stay below
    MAX_REFUSED of the steps so far.  Deterministic in its arguments."""
    rng = random.Random(seed * 7919 + MODE_NAMES.index(start_mode) * 31 + int(instrumented))
    model = CtxModel(start_mode, instrumented)
    weight = {g: (6.0 if g[0] == "op" else 1.0 + 2.0 * rng.random()) for g in all_goals(instrumented)}
    open_goals = set(weight)
    steps, refused, prev = [], 0, None

    def draw(op):
        fam = FAMILY[op]
        if fam == "blur":
            return Step(op, arg=rng.choice(MODE_NAMES))
        if fam == "cache_blur":
            return Step(op, arg=rng.random() < 0.5)
        if fam in AGAINST_FAMILIES:     # the reference's size (the Python wrapper checks it), live or not
            size = model.ref.size if model.ref else model.last_ref_size or rng.choice(SIZE_ORDER)
        else:
            size = rng.choice(SIZE_ORDER)
        st = Step(op, size=size)
        if fam in PAIR_FAMILIES or (fam in AGAINST_FAMILIES and fam != "batch_against"):
            st = st._replace(k=rng.choice((1, 2)))
        if fam in ("pair16", "ref16", "against16", "strided16"):
            st = st._replace(depth=rng.choice(DEPTHS))
        if fam == "strided8":
            st = st._replace(layout=rng.choice(LAYOUTS8))
        if fam == "strided16":
            st = st._replace(layout=rng.choice(LAYOUTS16))
        if fam in BATCH_FAMILIES:
            st = st._replace(n=rng.choice(BATCH_N))
        return st

    def potential(st):
        """What a step that fulfils nothing by itself makes reachable: a reference of a kind and direction, a mode."""
        fam = FAMILY[st.op]

        def reachable(kind, mode, rel):
            return sum(1 for g in open_goals if g[0] == "cell" and g[2:] == (kind, mode, rel))
        if fam in ("ref8", "ref16") and model.predict(st)[0] is None and model.last_ref_size not in (None, st.size):
            if model.ref is not None and reachable(model.ref.kind, model.mode, model.ref_rel):
                return 0.0      # the live reference still has conditions to meet
            rk = {"set_reference": "8h", "set_reference_device": "8d", "set_reference_hbd": "16"}[st.op]
            rel = "larger" if SIZE_ORDER.index(st.size) > SIZE_ORDER.index(model.last_ref_size) else "smaller"
            return min(0.9, 0.15 * reachable(rk, model.mode, rel))
        if fam == "blur" and st.arg != model.mode:
            return min(0.4, 0.01 * sum(1 for g in open_goals if g[0] == "cell" and g[3] == st.arg))
        return 0.0

    for i in range(length):
        cands = []
        for op in OPS:
            if op == "cache_blur" and not instrumented:
                continue
            for _ in range(3 if FAMILY[op] in ("blur", "ref8", "ref16") else 2):
                st = draw(op)
                cands.append(st)
                if model.predict(st)[0] is None:
                    if ("refusal", "wait_idle", None) in open_goals or rng.random() < 0.03:
                        cands.append(st._replace(poke="wait"))
                    if op in ENQUEUE_OPS and (("refusal", "blur_enqueued", None) in open_goals or rng.random() < 0.2):
                        cands.append(st._replace(poke=rng.choice(MODE_NAMES)))
        best, best_score = None, -1.0
        for st in cands:
            is_refusal = model.predict(st)[0] is not None or st.poke is not None
            if is_refusal and refused + 1 > MAX_REFUSED * (i + 1):
                continue
            score = sum(weight[g] for g in step_goals(model, prev, st) if g in open_goals) + potential(st)
            score += 0.5 * rng.random()
            if score > best_score:
                best, best_score = st, score
        code, kind = model.predict(best)
        best = best._replace(expect=code, kind=kind)
        open_goals.difference_update(step_goals(model, prev, best))
        refused += code is not None or best.poke is not None
        model.apply(best)
        prev = FAMILY[best.op]
        steps.append(best)
    return steps


# the committed set: (seed, start mode, instrumented) -- six product plans, two seeds for each start mode, and two
# instrumented ones; seeds and length picked on the CPU so that the conditions of tests/test_ctx_walk_plan.py hold
PLAN_LENGTH = 300
PLANS = [(1, "fir", False), (2, "fir", False), (1, "recursive", False), (2, "recursive", False),
         (1, "recursive_fma", False), (3, "recursive_fma", False), (3, "fir", True), (1, "recursive", True)]
_PLANS = {}


def plan_id(p):
    return f"{'instr' if p[2] else 'product'}-{p[1]}-{p[0]}"


def committed_plan(p):
    return _memo(_PLANS, p, lambda: plan(*p, length=PLAN_LENGTH))


# ---- execution (needs the GPU) -------------------------------------------------------------------------------------------
def _refused(call, code, what):
    from oavif_amd import Ssimu2Error
    try:
        call()
    except Ssimu2Error as e:
        assert e.code == code, (what, e.code, code, str(e))
        return
    raise AssertionError((what, "was not refused", code))


def execute(s, st, pokes=True):
    """Run one step on the context `s` -> Result, or None for a step that scores nothing.  A refusal raises
    Ssimu2Error.  Device forms are given real device pointers, also where the step is to be refused."""
    op = st.op
    if st.poke == "wait" and pokes:
        before = s.last_averages()
        _refused(s.wait, _lib.ERR_INVALID_ARG, (st, "wait with nothing enqueued"))
        assert _same_avg(s.last_averages(), before), (st, "last_averages after the refused wait")
    if op == "set_blur":
        s.set_blur(gpu_cases.MODES[st.arg][0])
        return None
    if op == "cache_blur":
        s.cache_reference_blur(st.arg)
        return None
    w, h = SIZES[st.size]
    m = items = None
    if op == "set_reference":
        s.set_reference(frame8(st.size, 0))
        return None
    if op == "set_reference_device":
        s.set_reference_device(dev8(st.size, 0).data_ptr(), w, h)
        return None
    if op == "set_reference_hbd":
        s.set_reference_hbd(frame16(st.size, 0, st.depth), st.depth)
        return None
    if op == "compute":
        score = s.compute_ssimu2(frame8(st.size, 0), frame8(st.size, st.k))
    elif op == "score_device":
        score = s.score_device(dev8(st.size, 0).data_ptr(), dev8(st.size, st.k).data_ptr(), w, h)
    elif op in ENQUEUE_OPS:
        if op == "enqueue_device":
            s.enqueue_device(dev8(st.size, 0).data_ptr(), dev8(st.size, st.k).data_ptr(), w, h)
        else:
            s.enqueue_against_reference_device(dev8(st.size, st.k).data_ptr())
        if st.poke not in (None, "wait") and pokes:
            _refused(lambda: s.set_blur(gpu_cases.MODES[st.poke][0]), _lib.ERR_INVALID_ARG,
                     (st, "set_blur while a score is enqueued"))
        score = s.wait()
    elif op == "error_map":
        score, m = s.error_map(frame8(st.size, 0), frame8(st.size, st.k))
    elif op == "score_against":
        score = s.score_against_reference(frame8(st.size, st.k))
    elif op == "score_decoded":
        score = s.score_decoded_against_reference(strided8(st.size, st.k, st.layout)[1])
    elif op == "error_map_against":
        score, m = s.error_map_against_reference(frame8(st.size, st.k))
    elif op == "compute_hbd":
        score = s.compute_ssimu2_hbd(frame16(st.size, 0, st.depth), frame16(st.size, st.k, st.depth), st.depth)
    elif op == "score_against_hbd":
        score = s.score_against_reference_hbd(frame16(st.size, st.k, st.depth), st.depth)
    elif op == "score_decoded_hbd":
        score = s.score_decoded_against_reference_hbd(strided16(st.size, st.k, st.layout, st.depth)[1], bit_depth=st.depth)
    elif op == "score_batch":
        score = s.score_batch(*batch_pairs(st.size, st.n))
    elif op == "score_batch_device":
        score = s.score_batch_device(dev_items(st.size, st.n, "refs").data_ptr(), dev_items(st.size, st.n, "dists").data_ptr(),
                                     item_stride(st.size), st.n, w, h)
    elif op == "score_batch_against":
        score = s.score_batch_against_reference(batch_dists(st.size, st.n))
    elif op == "score_batch_against_device":
        score = s.score_batch_against_reference_device(dev_items(st.size, st.n, "against").data_ptr(), item_stride(st.size),
                                                       st.n)
    else:
        raise AssertionError(op)
    if FAMILY[op] in BATCH_FAMILIES:
        return Result(score, None, None, None, [s.last_batch_averages(i) for i in range(st.n)])
    avg, ns = s.last_averages()
    return Result(score, avg, ns, m, items)


def _same_avg(a, b):
    return a[1] == b[1] and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


def same_result(got, exp, what):
    """Score(s), all 108 averages and the scale count (of every item of a batch) and the map: the same bits."""
    assert np.array_equal(np.asarray(got.score, np.float64).view(np.uint64),
                          np.asarray(exp.score, np.float64).view(np.uint64)), (what, got.score, exp.score)
    if got.items is not None:
        assert len(got.items) == len(exp.items), what
        for i, (g, e) in enumerate(zip(got.items, exp.items)):
            assert _same_avg(g, e), (what, "item", i)
        return
    assert _same_avg((got.avg, got.ns), (exp.avg, exp.ns)), (what, "averages")
    assert (got.map is None) == (exp.map is None), what
    if got.map is not None:
        gpu_cases.same_bits(got.map, exp.map, what)


def set_ref(s, ref):
    """Give the context `s` the reference `ref` (a Ref), in the same form."""
    op = {"8h": "set_reference", "8d": "set_reference_device", "16": "set_reference_hbd"}[ref.kind]
    execute(s, Step(op, size=ref.size, depth=ref.depth))


class FreshTable:
    """What each single call returns on a fresh context in a mode, memoised by (instrumented, mode, operation, size,
    frame, layout, depth, items, reference: size, form, depth and cache flag)."""

    def __init__(self):
        self.table = {}
        self.created = 0
        self.frozen = False

    @staticmethod
    def key(model, st):
        ref = model.ref if FAMILY[st.op] in AGAINST_FAMILIES else None
        return (model.instrumented, model.mode, st.op, st.size, st.k, st.layout, st.depth, st.n, ref)

    def get(self, model, st):
        key = self.key(model, st)
        if key not in self.table:
            assert not self.frozen, ("not in the serial table", key)
            from oavif_amd import Ssimu2
            with Ssimu2(0, instrumented=model.instrumented, blur=gpu_cases.MODES[model.mode][0]) as s:
                self.created += 1
                if key[-1] is not None:
                    if model.instrumented:
                        s.cache_reference_blur(key[-1].cached)
                    set_ref(s, key[-1])
                self.table[key] = execute(s, st, pokes=False)
        return self.table[key]

    def prefetch(self, steps, start_mode, instrumented):
        """Fill the table with every scoring step of a plan (serially, before threads read it)."""
        model = CtxModel(start_mode, instrumented)
        for st in steps:
            if model.predict(st)[0] is None and FAMILY[st.op] not in ("blur", "cache_blur", "ref8", "ref16"):
                self.get(model, st)
            model.apply(st)


def walk(s, steps, start_mode, instrumented, fresh):
    """Drive the context `s` (fresh, in `start_mode`) through `steps`, holding every step to the model and to the
    table of fresh contexts `fresh`.  -> {"steps", "scored", "refused", "pokes"} counts."""
    from oavif_amd import Ssimu2Error
    model = CtxModel(start_mode, instrumented)
    single = s.last_averages()
    batch0 = None
    counts = {"steps": 0, "scored": 0, "refused": 0, "pokes": 0}
    for i, st in enumerate(steps):
        what = (i, model.mode, model.ref) + tuple(st)
        code, kind = model.predict(st)
        assert (code, kind) == (st.expect, st.kind), (what, "the plan was made with another model")
        fam = FAMILY[st.op]
        counts["steps"] += 1
        counts["pokes"] += st.poke is not None
        if code is not None:
            try:
                execute(s, st)
            except Ssimu2Error as e:
                assert e.code == code, (what, e.code, str(e))
            else:
                raise AssertionError((what, "was not refused"))
            assert _same_avg(s.last_averages(), single), (what, "last_averages after a refusal")
            if batch0 is not None:
                assert _same_avg(s.last_batch_averages(0), batch0), (what, "last_batch_averages after a refusal")
            counts["refused"] += 1
            model.apply(st)
            continue
        try:
            got = execute(s, st)
        except Ssimu2Error as e:
            raise AssertionError((what, "refused, predicted to succeed", e.code, str(e)))
        if got is not None:
            same_result(got, fresh.get(model, st), what)
            counts["scored"] += 1
            if fam in BATCH_FAMILIES:
                assert _same_avg(s.last_averages(), single), (what, "last_averages after a batch")
                batch0 = got.items[0]
            else:
                single = (got.avg, got.ns)
                if batch0 is not None:
                    assert _same_avg(s.last_batch_averages(0), batch0), (what, "last_batch_averages after a single score")
        model.apply(st)
    return counts
