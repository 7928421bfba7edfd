"""Batch scoring against the single-score paths, on the GPU box -> profiles/batch_score.json.

    python scripts/gpu_batch_bench.py [--out profiles/batch_score.json] [--quick]

Per frame size (256x256, 512x512, 1280x720, 1920x1080, 3840x2160) and batch size N (1, 4, 16, 64), alternating in one
process A B C A B C ... (ROUNDS rounds; the spread of each is reported):
    A  the single path on one context: pair scores enqueued back to back, one wait at the end of the window
    B  the single path fanned over two contexts (scorer.score_many's pattern: enqueue on both, wait for both)
    C  ssimu2_score_batch_rgb8_device: N pairs per call, one call after the other on one context
A and B are the code paths a caller had before batch scoring; C is never compared with itself.  Inputs are device
resident and every mode rotates over the same set of more than 256 MiB of distinct pairs (HBM-fed, not Infinity-Cache-
fed).  Every shape is warmed up; a timed window is at least WINDOW_S of work; the clock is the host's around work that
ends in a stream synchronise.  All figures are rates over whole calls (launches, waits and the result read included),
not kernel times.

The tiling A/B (which segment rows a batch item gets at scale 0: the single-score rule, 48, 96 or 160 rows) runs the
same way on the instrumented build at 512x512 and 1920x1080 with N = 32.

Every GPU step is a child process of its own under `timeout`; the parent stops at the first child that fails.

The three-dispatches-per-call claim is checked in a run of its own (no counters):
    rocprofv3 --kernel-trace --stats -d OUTDIR -- python scripts/gpu_batch_bench.py --child trace
which makes TRACE_CALLS batch calls at N = 1 and as many at N = 64: the stats show TRACE_CALLS * 2 dispatches of each of
k_pyramid_bands_batch, k_march_batch and k_finalize_batch.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(256, 256), (512, 512), (1280, 720), (1920, 1080), (3840, 2160)]
BATCHES = [1, 4, 16, 64]
TILING_SIZES = [(512, 512), (1920, 1080)]
TILING_ROWS = [-1, 48, 96, 160]   # -1: the single-score rule of the frame size
TILING_N = 32
ROUNDS = 3
WINDOW_S = 0.3
ROTATE_BYTES = 256 << 20
TRACE_CALLS = 10
CHILD_TIMEOUT_S = 280


def make_inputs(w, h, pairs):
    """`pairs` distinct device-resident pairs in two [pairs, stride] uint8 tensors (rolled / flipped copies of one
    synthetic pair: distinct bytes at every address)."""
    import torch
    from oavif_amd import synth
    ref = synth.make_ref(w, h, 0)
    dst = synth.distort(ref, "blockq", 2)
    tr, td = torch.from_numpy(ref).cuda(), torch.from_numpy(dst).cuda()
    stride = (w * h * 3 + 255) & ~255
    refs = torch.zeros((pairs, stride), dtype=torch.uint8, device="cuda")
    dists = torch.zeros((pairs, stride), dtype=torch.uint8, device="cuda")
    for k in range(pairs):
        a = torch.roll(tr, (k * 7 % h, k * 13 % w), (0, 1))
        b = torch.roll(td, (k * 7 % h, k * 13 % w), (0, 1))
        if k & 1:
            a, b = a.flip(0), b.flip(0)
        refs[k, :w * h * 3] = a.reshape(-1)
        dists[k, :w * h * 3] = b.reshape(-1)
    torch.cuda.synchronize()
    return refs, dists, stride


def pairs_for(w, h, quick):
    need = -(-ROTATE_BYTES // (2 * w * h * 3)) + 1
    n = max(need, 64)
    n = -(-n // 64) * 64
    return 64 if quick else n


def timed(fn, pairs_per_call, est_s):
    """Pairs per second of fn() repeated over a window of at least WINDOW_S (fn ends in a synchronise)."""
    reps = max(1, int(WINDOW_S / max(est_s, 1e-6)) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = time.perf_counter() - t0
    return pairs_per_call * reps / dt


def summarise(rates):
    med = statistics.median(rates)
    return {"pairs_per_s": med, "us_per_pair": 1e6 / med, "spread": (max(rates) - min(rates)) / med, "runs": rates}


def child_cells(w, h, quick):
    import oavif_amd
    P = pairs_for(w, h, quick)
    refs, dists, stride = make_inputs(w, h, P)
    pr, pd = refs.data_ptr(), dists.data_ptr()
    ctx = [oavif_amd.Ssimu2(0), oavif_amd.Ssimu2(0)]
    chunk = 64   # pairs per pass of A and B

    def run_a(base):
        s = ctx[0]
        for i in range(base, base + chunk):
            s.enqueue_device(pr + i * stride, pd + i * stride, w, h)
        s.wait()

    def run_b(base):
        for i in range(base, base + chunk, 2):
            ctx[0].enqueue_device(pr + i * stride, pd + i * stride, w, h)
            ctx[1].enqueue_device(pr + (i + 1) * stride, pd + (i + 1) * stride, w, h)
        ctx[0].wait()
        ctx[1].wait()

    def run_c(base, n):
        for i in range(base, base + chunk, n):
            ctx[0].score_batch_device(pr + i * stride, pd + i * stride, stride, n, w, h)

    state = {"at": 0}

    def rotating(fn, *a):
        def call():
            fn(state["at"], *a)
            state["at"] = (state["at"] + chunk) % P
        return call

    cells = []
    mp = w * h / 1e6
    for n in BATCHES:
        modes = {"A": rotating(run_a), "B": rotating(run_b), "C": rotating(run_c, n)}
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
        res = {k: summarise(v) for k, v in runs.items()}
        cell = {"w": w, "h": h, "n": n, "distinct_pairs": P,
                "A_single_one_context": res["A"], "B_single_two_contexts": res["B"], "C_batch": res["C"],
                "mp_per_s": {k: res[k]["pairs_per_s"] * mp for k in res},
                "C_over_A": res["C"]["pairs_per_s"] / res["A"]["pairs_per_s"],
                "C_over_B": res["C"]["pairs_per_s"] / res["B"]["pairs_per_s"],
                "spread_max": max(r["spread"] for r in res.values())}
        cells.append(cell)
        print(f"# {w}x{h} N={n}: A {res['A']['us_per_pair']:.1f} B {res['B']['us_per_pair']:.1f} C {res['C']['us_per_pair']:.1f} "
              f"us/pair  C/A {cell['C_over_A']:.2f}  C/B {cell['C_over_B']:.2f}  spread {cell['spread_max']:.3f}", file=sys.stderr)
    for c in ctx:
        c.close()
    return cells


def child_tiling(w, h, quick):
    import oavif_amd
    n = TILING_N
    P = pairs_for(w, h, quick)
    refs, dists, stride = make_inputs(w, h, P)
    pr, pd = refs.data_ptr(), dists.data_ptr()
    s = oavif_amd.Ssimu2(0, instrumented=True)
    chunk = 64
    state = {"at": 0}

    def call():
        for i in range(state["at"], state["at"] + chunk, n):
            s.score_batch_device(pr + i * stride, pd + i * stride, stride, n, w, h)
        state["at"] = (state["at"] + chunk) % P
    est, runs, rows_used = {}, {r: [] for r in TILING_ROWS}, {}
    for r in TILING_ROWS:
        s.set_batch_segment_rows(r)
        rows_used[r] = s.batch_segment_rows(w, h, 0)
        call()
        t0 = time.perf_counter()
        call()
        call()
        est[r] = (time.perf_counter() - t0) / 2
    for _ in range(ROUNDS + 1):   # A B C D A B C D ...
        for r in TILING_ROWS:
            s.set_batch_segment_rows(r)
            runs[r].append(timed(call, chunk, est[r]))
    s.set_batch_segment_rows(0)
    s.close()
    out = []
    for r in TILING_ROWS:
        d = summarise(runs[r])
        d.update({"w": w, "h": h, "n": n, "rule": "single-score rule" if r < 0 else f"{r} rows", "rows_scale0": rows_used[r]})
        out.append(d)
        print(f"# tiling {w}x{h} N={n} {d['rule']} ({rows_used[r]} rows): {d['us_per_pair']:.2f} us/pair spread {d['spread']:.3f}",
              file=sys.stderr)
    return out


def child_trace():
    import oavif_amd
    w = h = 512
    refs, dists, stride = make_inputs(w, h, 64)
    s = oavif_amd.Ssimu2(0)
    for n in (1, 64):
        for _ in range(TRACE_CALLS):
            s.score_batch_device(refs.data_ptr(), dists.data_ptr(), stride, n, w, h)
    s.close()
    print(json.dumps({"calls_per_n": TRACE_CALLS, "n": [1, 64]}))


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
        quick = "--quick" in argv
        if kind == "trace":
            child_trace()
            return 0
        w, h = (int(x) for x in argv[argv.index("--size") + 1].split("x"))
        print(json.dumps(child_cells(w, h, quick) if kind == "cells" else child_tiling(w, h, quick)))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "batch_score.json")
    extra = ["--quick"] if "--quick" in argv else []
    import oavif_amd
    record = {"what": "ssimu2_score_batch_rgb8_device (C) against single scores on one context (A) and fanned over two "
                      "contexts (B); rates over whole calls, host clock around work that ends in a stream synchronise; "
                      "inputs in HBM, rotating over distinct_pairs pairs; median of the rounds, spread = (max - min) / median",
              "version": oavif_amd.version(), "rounds": ROUNDS, "window_s": WINDOW_S, "cells": [], "tiling": []}
    status = 0
    for w, h in TILING_SIZES:
        r = run_child(["--child", "tiling", "--size", f"{w}x{h}"] + extra)
        if r is None:
            status = 1
            break
        record["tiling"] += r
    for w, h in SIZES if status == 0 else []:
        r = run_child(["--child", "cells", "--size", f"{w}x{h}"] + extra)
        if r is None:
            status = 1
            break
        record["cells"] += r
    record["complete"] = status == 0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {out} ({len(record['cells'])} cells, {len(record['tiling'])} tiling rows, complete={record['complete']})")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
