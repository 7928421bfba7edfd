"""Batches in the recursive blur modes against the single cached pass, on the GPU box
-> profiles/rbatch_score.json.

    python scripts/gpu_rbatch_bench.py [--out profiles/rbatch_score.json] [--quick]

The protocol of scripts/gpu_batch_bench.py (whose input maker, window and summary this script takes).  Per frame size
(256x256, 512x512, 1280x720, 1920x1080) and batch size N (1, 4, 16, 64) in SSIMU2_BLUR_RECURSIVE, and at 512x512 in
SSIMU2_BLUR_RECURSIVE_FMA too, alternating in one process A B C A B C ... (ROUNDS rounds; the spread of each is
reported):
    A  single passes against the cached reference on one context: enqueued back to back, one wait per window chunk
    B  the same fanned over two contexts, each with the reference cached
    C  ssimu2_rbatch_score_against_reference_device: N frames per call, one call after the other on one context
A and B are the code paths a caller had before; C is never compared with itself.  At N = 16 the pair form runs as well:
P1 = pair scores enqueued back to back on one context, PC = ssimu2_rbatch_score_rgb8_device.  Inputs are device resident
and every mode rotates over the same set of more than 256 MiB of distinct frames (HBM-fed); every shape is warmed up; a
timed window is at least WINDOW_S of work; the clock is the host's around work that ends in a stream synchronise.  All
figures are rates over whole blocking calls, not kernel times.

Every GPU step is a child process of its own under `timeout`; the parent stops at the first child that fails.

The launches per batch call are counted in a run of its own (no counters):
    rocprofv3 --kernel-trace --stats -d OUTDIR -- python scripts/gpu_rbatch_bench.py --child trace
which makes TRACE_CALLS against-reference batch calls at N = 1 and as many at N = 64, then as many pair calls at each:
the stats show TRACE_CALLS * 4 dispatches of k_pyramid_bands_xyb_batch, k_rg_h_batch<.., false>, k_rg_v_batch and
k_finalize_batch, and TRACE_CALLS * 2 of k_rg_h_batch<.., true> and k_rg_v_emit_batch (the pair form's reference side).
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_batch_bench import ROUNDS, WINDOW_S, make_inputs, pairs_for, summarise, timed  # noqa: E402

SIZES = [(256, 256), (512, 512), (1280, 720), (1920, 1080)]
FMA_SIZES = [(512, 512)]
BATCHES = [1, 4, 16, 64]
PAIR_N = 16
TRACE_CALLS = 10
CHILD_TIMEOUT_S = 200


def child_cells(w, h, mode_name, quick):
    import oavif_amd
    from oavif_amd import _lib
    mode = {"recursive": _lib.BLUR_RECURSIVE, "recursive_fma": _lib.BLUR_RECURSIVE_FMA}[mode_name]
    P = pairs_for(w, h, quick)
    refs, dists, stride = make_inputs(w, h, P)
    pr, pd = refs.data_ptr(), dists.data_ptr()
    ctx = [oavif_amd.Ssimu2(0, blur=mode, rbatch=True), oavif_amd.Ssimu2(0, blur=mode, rbatch=True)]
    for c in ctx:
        c.set_reference_device(pr, w, h)
    chunk = 64   # frames per pass of every mode

    def run_a(base):
        s = ctx[0]
        for i in range(base, base + chunk):
            s.enqueue_against_reference_device(pd + i * stride)
        s.wait()

    def run_b(base):
        for i in range(base, base + chunk, 2):
            ctx[0].enqueue_against_reference_device(pd + i * stride)
            ctx[1].enqueue_against_reference_device(pd + (i + 1) * stride)
        ctx[0].wait()
        ctx[1].wait()

    def run_c(base, n):
        for i in range(base, base + chunk, n):
            ctx[0].score_batch_against_reference_device(pd + i * stride, stride, n)

    def run_p1(base):
        s = ctx[1]   # the pair score overwrites a context's cached reference: not on the context A and C use
        for i in range(base, base + chunk):
            s.enqueue_device(pr + i * stride, pd + i * stride, w, h)
        s.wait()

    def run_pc(base, n):
        for i in range(base, base + chunk, n):
            ctx[0].score_batch_device(pr + i * stride, pd + i * stride, stride, n, w, h)

    state = {"at": 0}

    def rotating(fn, *a):
        def call():
            fn(state["at"], *a)
            state["at"] = (state["at"] + chunk) % P
        return call

    def measure(modes):
        est = {}
        for k, fn in modes.items():   # warm-up of every shape, and the estimate that sizes the window
            fn()
            t0 = time.perf_counter()
            fn()
            fn()
            est[k] = (time.perf_counter() - t0) / 2
        runs = {k: [] for k in modes}
        for _ in range(ROUNDS):
            for k, fn in modes.items():
                runs[k].append(timed(fn, chunk, est[k]))
        return {k: summarise(v) for k, v in runs.items()}

    cells = []
    for n in BATCHES:
        res = measure({"A": rotating(run_a), "B": rotating(run_b), "C": rotating(run_c, n)})
        cell = {"w": w, "h": h, "n": n, "mode": mode_name, "distinct_frames": P,
                "A_single_one_context": res["A"], "B_single_two_contexts": res["B"], "C_batch": res["C"],
                "C_over_A": res["C"]["pairs_per_s"] / res["A"]["pairs_per_s"],
                "C_over_B": res["C"]["pairs_per_s"] / res["B"]["pairs_per_s"],
                "spread_max": max(r["spread"] for r in res.values())}
        cells.append(cell)
        print(f"# {mode_name} {w}x{h} N={n}: A {res['A']['us_per_pair']:.1f} B {res['B']['us_per_pair']:.1f} "
              f"C {res['C']['us_per_pair']:.1f} us/frame  C/A {cell['C_over_A']:.2f}  C/B {cell['C_over_B']:.2f}  "
              f"spread {cell['spread_max']:.3f}", file=sys.stderr)
    pair = None
    if mode_name == "recursive":
        res = measure({"P1": rotating(run_p1), "PC": rotating(run_pc, PAIR_N)})
        for c in ctx:
            c.set_reference_device(pr, w, h)
        pair = {"w": w, "h": h, "n": PAIR_N, "mode": mode_name, "P1_pair_single_one_context": res["P1"],
                "PC_pair_batch": res["PC"], "PC_over_P1": res["PC"]["pairs_per_s"] / res["P1"]["pairs_per_s"],
                "spread_max": max(r["spread"] for r in res.values())}
        print(f"# {mode_name} {w}x{h} pairs N={PAIR_N}: P1 {res['P1']['us_per_pair']:.1f} PC {res['PC']['us_per_pair']:.1f} "
              f"us/pair  PC/P1 {pair['PC_over_P1']:.2f}  spread {pair['spread_max']:.3f}", file=sys.stderr)
    for c in ctx:
        c.close()
    return {"cells": cells, "pair": pair}


def child_trace():
    import oavif_amd
    from oavif_amd import _lib
    w = h = 512
    refs, dists, stride = make_inputs(w, h, 64)
    s = oavif_amd.Ssimu2(0, blur=_lib.BLUR_RECURSIVE, rbatch=True)
    s.set_reference_device(refs.data_ptr(), w, h)
    for n in (1, 64):
        for _ in range(TRACE_CALLS):
            s.score_batch_against_reference_device(dists.data_ptr(), stride, n)
    for n in (1, 64):
        for _ in range(TRACE_CALLS):
            s.score_batch_device(refs.data_ptr(), dists.data_ptr(), stride, n, w, h)
    s.close()
    print(json.dumps({"calls_per_n_and_form": TRACE_CALLS, "n": [1, 64], "forms": ["against", "pair"]}))


def run_child(args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(f"child {' '.join(args)} ended with status {p.returncode}: stopping", file=sys.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(argv):
    if "--child" in argv:
        kind = argv[argv.index("--child") + 1]
        if kind == "trace":
            child_trace()
            return 0
        w, h = (int(x) for x in argv[argv.index("--size") + 1].split("x"))
        print(json.dumps(child_cells(w, h, argv[argv.index("--mode") + 1], "--quick" in argv)))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "rbatch_score.json")
    extra = ["--quick"] if "--quick" in argv else []
    import oavif_amd
    record = {"what": "ssimu2_rbatch_score_against_reference_device (C) against single cached passes on one context (A) and "
                      "fanned over two contexts (B), SSIMU2_BLUR_RECURSIVE / _FMA; at N = 16 the pair form (PC) against pair "
                      "scores on one context (P1); rates over whole blocking calls, host clock around work that ends in a "
                      "stream synchronise; inputs in HBM, rotating over distinct_frames frames; median of the rounds, "
                      "spread = (max - min) / median",
              "version": oavif_amd.version(), "rounds": ROUNDS, "window_s": WINDOW_S, "cells": [], "pair_cells": []}
    status = 0
    for mode, sizes in (("recursive", SIZES), ("recursive_fma", FMA_SIZES)):
        for w, h in sizes if status == 0 else []:
            r = run_child(["--child", "cells", "--size", f"{w}x{h}", "--mode", mode] + extra)
            if r is None:
                status = 1
                break
            record["cells"] += r["cells"]
            if r["pair"]:
                record["pair_cells"].append(r["pair"])
    record["complete"] = status == 0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {out} ({len(record['cells'])} cells, {len(record['pair_cells'])} pair cells, complete={record['complete']})")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
