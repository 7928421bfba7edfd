#!/usr/bin/env python3
"""bench.py -- SSIMULACRA2 scorer throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: the command starts its own N ranks, one per GPU -- oavif_amd/launch.py -- unless a launcher has announced a
     world: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...`
     runs the same ranks)

A *step* is one pass of the hot path over one batch of synthetic input: one SSIMULACRA2
score of one (ref, dist) pair of 3840x2160 8-bit RGB frames (BASELINE.json configs[1],
"Single 3840x2160 8-bit RGB, --score-tgt 80 --max-pass 6, SSIMULACRA2 on 1 MI355X"), both
frames already resident in HBM when the timed region starts.  The steps ROTATE over
`--pairs` distinct pairs per scorer context (default 8 per context, two contexts: 16 pairs,
0.8 GB of frames), so every score reads its inputs from HBM, not from the 256 MiB Infinity
Cache -- a batch never rescans one pair.  The cache-resident figure (one pair scored over and
over, what round 1 reported) is kept as the labelled extra `cache_resident` (--full).
With N ranks every rank scores its own pairs (independent images shard with no data-path
collective: weak scaling); the only collective is the final RCCL all_gather of the per-rank
result records.  value = megapixels (scale-0 pixels of one image) scored per second, whole job.

A plain run does what the headline figure needs and nothing more: it sets up, warms up, times the steps, writes its
outputs if --dump-outputs is given and prints the line (metric, value, unit, ms_per_step, ..., `scores`: the score of
each rank's pair 0; N > 1: `collective` and per_rank_own_ms_per_step).  `--full` also measures everything else: the
extra objects below, all of them taken after the timed steps and the dump.

Extra objects on the JSON line (--full, unless said otherwise):
  roofline     -- dominant kernel (k_march: XYB + blur + maps of all six scales): algorithmic
                  bytes of SURVEY.md 8(d)'s W-model for the stages that kernel covers, divided
                  by its average launch time measured live with HIP events on the kernel's own
                  stream over launches that rotate over the same pairs (HBM-fed).  `frac` is
                  against the 8 TB/s HBM peak; north_star's own blur-pyramid figure, the measured
                  HBM traffic and the VALU-issue fractions (what actually limits the kernel) are
                  beside it.  Counter-derived fields come from profiles/counters.json, written
                  by scripts/make_counters_json.py from this round's rocprofv3 PMC run and
                  stamped with the kernel source hash; a mismatch is reported as "stale".
  cpu_baseline -- the repo's CPU oracle ("port"; the reference's Zig+fssimu2 path cannot be
                  built: no Zig, fssimu2 source absent) timed on this host, rank 0, N = 1 only.
  collective   -- what the process group really was (oavif_amd/collective.py): backend, world size, and per
                  rank the host, HIP device index, PCI bus id, NUMA node, pinned cores and the HSA_* / HIP_* / ROCR_* /
                  NCCL_* / RCCL_* variables it ran under, exchanged through the rendezvous store BEFORE any communicator
                  exists and confirmed by one all_gather over the job's process group (device tensors through RCCL when the
                  backend is nccl; at N = 1, --full only, a process group of one rank is opened for it after the timed region).  The run
                  exits non-zero (rc 4, every rank, no communicator ever created) when two RCCL ranks report one GPU or the
                  host shows fewer devices than ranks; rc 5 with RCCL's message when the process group cannot be opened.
  by_resolution -- N = 1: the named resolutions (512x512, 1920x1080, 3840x2160, 7680x4320), each HBM-fed: FIR
                  pair scoring on two contexts / one stream with the W-model fraction, the recursive cached pass, and every
                  kernel's own duration beside the stream time of a score.
  per_rank_own_ms_per_step -- N > 1 only, every run: each rank's own work per step up to its synchronize, before the closing
                  barrier; `ms_per_step` is the max over ranks of the whole block, so a slow rank shows.
  --dump-outputs DIR -- every run: after the timed steps, rank 0 writes what the last timed step computed, as its caller receives it:
                  DIR/score.npy (float64, shape (1,): the SSIMULACRA2 score ssimu2_wait returned) and
                  DIR/plane_averages.npy (float64, (6, 18): ssimu2_last_averages of that score).  The inputs are seeded, so
                  two builds run with the same arguments can be compared output for output.
  default_search_mode -- throughput of the mode the SEARCH path runs by default (the published recursion, one
                  cached-reference pass per probe), beside `value` (FIR pair scoring, two contexts); its per-kernel times
                  (recursive_blur_mode.kernels) are measured by this run: dispatch-packet timestamps of the instrumented build.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 3840, 2160
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec

# SURVEY.md 8(d) W-model: 85.97 algorithmic bytes per scale-0 pixel for one whole score
# (scale 0 reads 6 B/px of u8; every scale writes XYB_s and the blur stage reads it back,
# 48 B per pixel of that scale; scales >= 1 read linear_s, 24 B; every scale writes
# linear_{s+1}, 24 B per pixel of the next scale).  The dominant kernel -- the single fused
# marching launch over all six scales -- covers everything except the linear_{s+1} writes
# (done by the pyramid kernel): 85.97 - 24 * (1/4 + 1/16 + ...) = 85.97 - 8.00 = 77.97 B/px.
ALGO_BYTES_PER_PX_SCORE = 85.97
ALGO_BYTES_PER_PX_MARCH = 77.97
# blur-pyramid-only model of north_star's ">= 70 % HBM-read roofline" target (B-model)
ALGO_BYTES_PER_PX_BLUR = 31.99


def claim_stdout():
    """The contract is ONE JSON line on stdout, and this process is not the only writer of file descriptor 1: RCCL prints its
    banner there (the GPU box exports NCCL_DEBUG=VERSION: five lines in front of the line on every run of round 6), child
    processes inherit it.  From here on descriptor 1 IS descriptor 2 for everybody -- Python's own prints, C libraries,
    children -- and the returned `emit(obj)` writes one JSON line to what stdout was.  Called once per rank, after the
    self-launch decision (the supervisor relays its rank 0's stdout untouched)."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    def emit(obj) -> None:
        sys.stdout.flush()
        real.write(json.dumps(obj) + "\n")
        real.flush()
    return emit


def usable_cores() -> int:
    """Host threads this process may really use (cgroup quota / affinity mask, capped at 32)."""
    from oavif_amd import hostinfo
    return hostinfo.usable_cores()


def kernel_source_hash() -> str:
    """sha256 (first 16 hex digits) of the scorer's device + host sources: ties counter files to a build."""
    import hashlib
    hsh = hashlib.sha256()
    for name in ("ssimu2_kernels.h", "ssimu2_hip.hip"):
        with open(os.path.join(ROOT, "oavif_amd", "csrc", name), "rb") as f:
            hsh.update(f.read())
    return hsh.hexdigest()[:16]


def load_counters(size):
    """profiles/counters.json (scripts/make_counters_json.py from this round's rocprofv3 PMC run):
    per-launch HBM bytes and VALU instruction counts of the marching kernel at 4K.  Marked stale
    when the kernel sources have changed since the counters were taken."""
    path = os.path.join(ROOT, "profiles", "counters.json")
    if size != (W, H) or not os.path.exists(path):
        return None
    try:
        c = json.load(open(path))
    except Exception:
        return None
    c["stale"] = c.get("kernel_source_hash") != kernel_source_hash()
    return c


def rocprof_rg_csv(w: int, h: int):
    """Average kernel durations (ms) of the recursive pass in the newest committed profiles/rNN_rg_kernel_stats.csv (rocprofv3
    --kernel-trace --stats over scripts/gpu_rg_bench.py at 3840x2160): the cross-check of the live stage times, never their source."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_rg_kernel_stats.csv")))
    if not files or (w, h) != (3840, 2160):
        return None, {}
    keys = {"convert": "k_pyramid_bands_xyb", "h": "k_rg_h<false, false>", "v": "k_rg_v<false>"}
    rows = {}
    with open(files[-1]) as f:
        for r in csv.DictReader(f):
            for st, key in keys.items():
                if key in r["Name"] and (st != "v" or "emit" not in r["Name"]):
                    rows[st] = float(r["AverageNs"]) * 1e-6
    return os.path.relpath(files[-1], ROOT), rows


def recursive_pass_bytes(w: int, h: int):
    """Algorithmic bytes of the three big launches of a reference-cached recursive pass (each stage reads its inputs
    once and writes its outputs once), planes as the kernels address them: rows padded to 128 floats (ssimu2_recursive.h)."""
    n_pad = sum((((w + (1 << k) - 1) >> k) + 127) // 128 * 128 * ((h + (1 << k) - 1) >> k) for k in range(6)
                if k == 0 or (((w + (1 << (k - 1)) - 1) >> (k - 1)) >= 8 and ((h + (1 << (k - 1)) - 1) >> (k - 1)) >= 8))
    plane = n_pad * 4   # one fp32 plane over all scales
    return n_pad, {"convert": w * h * 3 + 3 * plane, "h": 6 * plane + 9 * plane, "v": 21 * plane}


def recursive_kernel_rooflines(w: int, h: int, live_pass_ms: float, stage_ms: dict, wall_timed_ms: float, wall_plain_ms: float):
    """Per-kernel achieved HBM rate of the recursive mode's cached pass: algorithmic bytes over the kernel's average duration
    MEASURED BY THIS RUN (ssimu2_time_kernels of the instrumented build: every launch of the pass made with a start / stop
    event pair, i.e. the duration its own dispatch packet recorded, passes rotating over distorted frames); the committed
    rocprofv3 averages are printed beside them as the cross-check."""
    n_pad, nbytes = recursive_pass_bytes(w, h)
    what = {"convert": ("k_pyramid_bands_xyb", "positive-XYB planes of the decoded frame at every scale, from its bytes", "mixed"),
            "h": ("k_rg_h<false, false>", "horizontal recursion of {y, yy, xy} x 3 channels: reads the XYB planes of both frames, "
                                          "writes nine planes", "mixed"),
            "v": ("k_rg_v<false>", "vertical recursion + maps: reads the nine planes, the six cached reference planes and the XYB "
                                   "planes of both frames", "read")}
    ceil = {"read": 6000.0, "write": 5600.0, "mixed": 5100.0}   # GB/s, profiles/r04_rw_mix.txt (2:3 / 1:1 read:write streams)
    csv_path, csv_ms = rocprof_rg_csv(w, h)
    ks = []
    for st, (kernel, text, which) in what.items():
        gbps = nbytes[st] / stage_ms[st] / 1e6
        k = {"kernel": kernel, "what": text, "ms": round(stage_ms[st], 4), "ms_measured_by_this_run": True,
             "algorithmic_bytes": int(nbytes[st]), "achieved_GBps": round(gbps, 1), "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBS, 3),
             "frac_of_measured_stream_ceiling": round(gbps / ceil[which], 3), "ceiling": which}
        if st in csv_ms:
            k["ms_rocprofv3_committed"] = round(csv_ms[st], 4)
        ks.append(k)
    ks.append({"kernel": "k_finalize", "what": "fixed-order fp64 sums, 108 averages, polynomial (latency, no stream)",
               "ms": round(stage_ms["finalize"], 4), "ms_measured_by_this_run": True})
    total = sum(stage_ms.values())
    moved = sum(nbytes.values())
    strict = w * h * 3 + 9 * n_pad * 4    # the distorted frame's bytes + the nine cached reference planes it is compared with
    out = {"source": "this run: ssimu2_time_kernels (instrumented build of the same sources: the library's own enqueue path, every "
                     "launch with a start / stop event pair = the duration its dispatch packet recorded), 48 passes rotating over the "
                     "distorted frames (HBM-fed)",
           "sum_of_kernels_ms": round(total, 4),
           "stream_ms_per_pass_with_timestamps": round(wall_timed_ms, 4), "stream_ms_per_pass_plain_launches": round(wall_plain_ms, 4),
           "between_launches_ms": round(wall_plain_ms - total, 4),
           "live_ms_per_pass": round(live_pass_ms, 4),
           "live_ms_per_pass_note": "the PRODUCT library's pass, host clock over a run of passes (cached_reference.ms_per_pass)",
           "live_over_sum_of_kernels": round(live_pass_ms / total, 3), "peak_GBps": HBM_PEAK_GBS,
           "measured_stream_ceilings_GBps": dict(ceil, source="profiles/r04_rw_mix.txt"),
           "kernels": ks,
           "bytes_moved_per_pass_GB": round(moved / 1e9, 3), "strict_minimum_GB": round(strict / 1e9, 3),
           "moved_over_strict_minimum": round(moved / strict, 2),
           "note": "the h -> v round trip of nine planes is the largest part of what is moved beyond the strict minimum (DESIGN.md "
                   "section 4: why it stays)"}
    if csv_path:
        out["rocprofv3_cross_check"] = {"source": csv_path + " (rocprofv3 --kernel-trace --stats of scripts/gpu_rg_bench.py, committed "
                                                             "with the round it names; another box)",
                                        "sum_of_kernels_ms": round(sum(csv_ms.values()), 4)}
    return out


def by_resolution(local_rank: int, t_ref, t_dst, fir_ctxs, budget_s: float = 1.0):
    """north_star: "throughput on synthetic RGB frames at the named resolutions"; SURVEY 8(d) names 512x512, 1920x1080,
    3840x2160 and 7680x4320.  Per size, on fresh contexts, every input resident in HBM and rotating over enough distinct pairs
    to exceed the 256 MiB Infinity Cache: FIR pair scoring on two contexts (what `value` is at 4K; `fir_ctxs` = the timed
    region's own two contexts, whose streams sit on distinct hardware queues) with its W-model fraction, the same on one
    stream, the recursive mode's reference-cached pass (the search path's default) on one stream, and every kernel's own
    duration in both modes (instrumented build, dispatch-packet timestamps) beside the stream time of a score: the difference
    is what the launches of a score wait between them.  Frames are cut from / tiled out of the 4K synthetic pair on the
    device (crops at stepped offsets; 8K = the 4K frame and its mirror images, 2 x 2)."""
    import torch
    import oavif_amd
    from oavif_amd import _lib
    W0, H0 = t_ref.shape[1], t_ref.shape[0]
    out = []

    def frames_of(w, h, k):
        if (w, h) == (W0, H0):
            a, b = torch.roll(t_ref, (k * 977) % W0, 1), torch.roll(t_dst, (k * 977) % W0, 1)
        elif w <= W0 and h <= H0:
            nx, ny = max(1, (W0 - w) // 256 + 1), max(1, (H0 - h) // 256 + 1)
            x0, y0 = min((k % nx) * 256, W0 - w), min(((k // nx) % ny) * 256, H0 - h)
            a, b = t_ref[y0:y0 + h, x0:x0 + w], t_dst[y0:y0 + h, x0:x0 + w]
            if (k // (nx * ny)) & 1:
                a, b = a.flip(1), b.flip(1)
        else:   # 2 x 2 of the frame and its mirror images (no seams: every neighbour is a reflection)
            def tile(t):
                t = torch.roll(t, (k * 977) % W0, 1)
                top = torch.cat([t, t.flip(1)], 1)
                return torch.cat([top, top.flip(0)], 0)[:h, :w]
            a, b = tile(t_ref), tile(t_dst)
        return a.contiguous(), b.contiguous()

    for (w, h) in ((512, 512), (1920, 1080), (3840, 2160), (7680, 4320)):
        mp = w * h / 1e6
        npairs = max(4, -(-272_000_000 // (2 * w * h * 3)))
        npairs += npairs & 1                      # even: the two contexts walk disjoint halves
        pairs = [frames_of(w, h, k) for k in range(npairs)]
        ptrs = [(a.data_ptr(), b.data_ptr()) for a, b in pairs]
        torch.cuda.synchronize()
        rec = {"width": w, "height": h, "megapixels": round(mp, 4), "distinct_pairs": npairs,
               "input_working_set_MB": round(npairs * 2 * w * h * 3 / 1e6, 1)}
        c0, c1 = fir_ctxs[0], fir_ctxs[1 % len(fir_ctxs)]

        def run(ctxs, n):
            for i in range(n):
                c = ctxs[i % len(ctxs)]
                pr, pd = ptrs[i % npairs]
                c.enqueue_device(pr, pd, w, h)
            sc = None
            for c in ctxs[:min(n, len(ctxs))]:
                sc = c.wait()
            return sc

        def rate(ctxs):
            run(ctxs, max(2 * npairs, 64))                       # capacity, clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(ctxs, 32)
            torch.cuda.synchronize()
            per = max((time.perf_counter() - t0) / 32, 1e-6)
            n = int(min(20000, max(32, budget_s / 4 / per)))
            t0 = time.perf_counter()
            run(ctxs, n)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        ms2 = rate([c0, c1]) if c1 is not c0 else None
        ms1 = rate([c0])
        if ms2 is not None:
            rec["fir_pair_two_contexts"] = {"ms_per_score": round(ms2, 5), "MP_per_s": round(mp / ms2 * 1e3, 1),
                                            "w_model_frac": round(ALGO_BYTES_PER_PX_SCORE * w * h / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        rec["fir_pair_one_stream"] = {"ms_per_score": round(ms1, 5), "MP_per_s": round(mp / ms1 * 1e3, 1),
                                      "w_model_frac": round(ALGO_BYTES_PER_PX_SCORE * w * h / (ms1 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        with oavif_amd.Ssimu2(local_rank, blur=_lib.BLUR_RECURSIVE) as rc_:
            rc_.set_reference_device(ptrs[0][0], w, h)
            dists = [p[1] for p in ptrs]

            def run_r(n):
                for i in range(n):
                    rc_.enqueue_against_reference_device(dists[i % npairs])
                return rc_.wait()
            run_r(max(npairs, 32))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_r(16)
            torch.cuda.synchronize()
            per = max((time.perf_counter() - t0) / 16, 1e-6)
            n = int(min(10000, max(16, budget_s / 4 / per)))
            t0 = time.perf_counter()
            run_r(n)
            torch.cuda.synchronize()
            msr = (time.perf_counter() - t0) / n * 1e3
            rec["recursive_cached_pass_one_stream"] = {"ms_per_pass": round(msr, 5), "MP_per_s": round(mp / msr * 1e3, 1)}
        # where the time goes: every kernel of a score / of a pass by its own dispatch-packet timestamps
        # (instrumented build) against the stream time per score of the same run with plain launches
        kp = min(npairs, 64)
        with oavif_amd.Ssimu2(local_rank, instrumented=True) as ic:
            st, _wt, wp = ic.time_kernels(w, h, [p[1] for p in ptrs[:kp]], 96, d_refs=[p[0] for p in ptrs[:kp]])
            rec["fir_kernels_ms"] = dict({k: round(v, 5) for k, v in st.items()}, sum=round(sum(st.values()), 5),
                                         stream_ms_per_score=round(wp, 5), between_launches_ms=round(wp - sum(st.values()), 5))
        with oavif_amd.Ssimu2(local_rank, instrumented=True, blur=_lib.BLUR_RECURSIVE) as irc:
            st, _wt, wp = irc.time_kernels(w, h, [p[1] for p in ptrs[:kp]], 96, d_ref=ptrs[0][0], recursive=True)
            rec["recursive_kernels_ms"] = dict({k: round(v, 5) for k, v in st.items()}, sum=round(sum(st.values()), 5),
                                               stream_ms_per_pass=round(wp, 5), between_launches_ms=round(wp - sum(st.values()), 5))
        out.append(rec)
        del pairs
        torch.cuda.empty_cache()
    return out


def cpu_baseline_child(argv) -> int:
    """bench.py --cpu-baseline-child CPUS THREADS W H SECONDS MAXREPS: the CPU checker (OpenMP build)
    timed on one core set in a process of its own -- the affinity is set before the first OpenMP region
    creates its threads (os.sched_setaffinity reaches only the calling thread of a process that already
    has threads), and nothing of torch / HIP runs beside it.  Prints one JSON line."""
    from oavif_amd import hostinfo, synth
    from oracle import ssimu2_oracle as orc   # checker / CPU timing only
    cpus, threads, w, h, seconds, maxreps = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), float(argv[4]), int(argv[5])
    pin_error = ""
    if cpus != "-":
        try:
            os.sched_setaffinity(0, hostinfo.parse_cpulist(cpus))
        except Exception as e:
            pin_error = f"{type(e).__name__}: {e}"
    orc.build()
    n = orc.set_num_threads(threads)
    ref = synth.make_ref(w, h, seed=0)
    dst = synth.distort(ref, "blockq", 2)
    orc.compute_ssimu2(ref[:256, :256], dst[:256, :256], orc.BLUR_FIR, omp=True)   # thread pool up
    ms, score = [], None
    t_all = time.perf_counter()
    while len(ms) < maxreps and (len(ms) < 2 or time.perf_counter() - t_all < seconds):
        t0 = time.perf_counter()
        score = orc.compute_ssimu2(ref, dst, orc.BLUR_FIR, omp=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    out = {"threads": n, "ms": [round(m, 1) for m in ms], "score": score, "pin_error": pin_error,
           "build": orc.omp_build_name()}
    if seconds > 5:   # the full run also takes the single-thread figure, on a 1/4-area crop, scaled per pixel
        crop_r, crop_d = ref[: h // 2, : w // 2], dst[: h // 2, : w // 2]
        t1 = time.perf_counter()
        orc.compute_ssimu2(crop_r, crop_d, orc.BLUR_FIR, omp=False)
        out["single_thread_MPps"] = round((w // 2) * (h // 2) / 1e6 / (time.perf_counter() - t1), 3)
    print(json.dumps(out), flush=True)
    return 0


def run_cpu_child(cpus, threads, w, h, seconds, maxreps):
    import subprocess
    from oavif_amd import hostinfo
    arg = hostinfo.format_cpus(cpus) if cpus else "-"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", arg, str(threads), str(w), str(h),
                        str(seconds), str(maxreps)], capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if not lines:
        raise RuntimeError(f"cpu_baseline child failed on cpus {arg}: {r.stderr[-400:]}")
    return json.loads(lines[-1])


def _cgroup_cpu_stat():
    try:
        return dict((k, int(v)) for k, v in (ln.split() for ln in open("/sys/fs/cgroup/cpu.stat")))
    except Exception:
        return {}


def measure_cpu_baseline(w, h, mp):
    """The CPU checker on this host's cores (rank 0, N = 1).  VERDICT r03 item 1: the figure must not depend
    on which cores a tenant-shared host happens to have free, so (i) the candidates are contiguous slices of
    whole cores near the GPU, the rank's fixed slice first (hostinfo.candidate_core_sets); (ii) each is timed
    briefly (2 repetitions) and the fastest is kept; (iii) the full sample runs there, in a process of its
    own; (iv) everything that decides the number is in the record: cgroup quota and cpuset, the per-core busy
    fractions of the chosen slice just before, the candidates' probe rates, the thread count that really ran,
    every repetition's ms, and the cgroup's throttle counters over the run."""
    from oavif_amd import hostinfo
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or usable_cores()
    quota = hostinfo.cgroup_cpu_quota()
    allowed = hostinfo.allowed_cpus()
    info = {"cgroup_cpu_quota": quota, "affinity_cpus": len(allowed)}
    try:
        info["cpuset_effective"] = open("/sys/fs/cgroup/cpuset.cpus.effective").read().strip()
    except Exception:
        info["cpuset_effective"] = None
    try:
        info["loadavg"] = open("/proc/loadavg").read().split()[0]
    except Exception:
        pass
    pin = quota is not None and quota < len(allowed)
    cands = hostinfo.candidate_core_sets(threads) if pin else [None]
    probes = []
    for cs in cands:
        try:
            r = run_cpu_child(cs, threads, w, h, 0.0, 2)
            probes.append({"cpus": hostinfo.format_cpus(cs) if cs else "unpinned",
                           "MPps_best_of_2": round(mp / min(r["ms"]) * 1e3, 1)})
        except Exception as e:
            probes.append({"cpus": hostinfo.format_cpus(cs) if cs else "unpinned", "error": str(e)[:200]})
    ok = [i for i, p_ in enumerate(probes) if "MPps_best_of_2" in p_]
    if not ok:
        raise RuntimeError(f"no candidate core set could be timed: {probes}")
    # the fixed slice unless another one is clearly (> 10 %) faster
    best = max(ok, key=lambda i: probes[i]["MPps_best_of_2"])
    pick = ok[0] if probes[best]["MPps_best_of_2"] <= 1.10 * probes[ok[0]]["MPps_best_of_2"] else best
    chosen = cands[pick]
    busy = hostinfo.busy_fractions(chosen, 1.0) if chosen else {}
    st0 = _cgroup_cpu_stat()
    full = run_cpu_child(chosen, threads, w, h, 12.0, 40)
    st1 = _cgroup_cpu_stat()
    ms = sorted(full["ms"])
    med = ms[len(ms) // 2]
    info.update({"candidates": probes, "chosen": hostinfo.format_cpus(chosen) if chosen else "unpinned",
                 "chosen_is_fixed_slice": pick == ok[0],
                 "busy_fraction_of_chosen_before": [round(busy.get(c, -1.0), 2) for c in (chosen or [])],
                 "ms_per_rep": {"min": ms[0], "median": med, "max": ms[-1], "n": len(ms)},
                 "cgroup_throttled_periods_during": (st1.get("nr_throttled", 0) - st0.get("nr_throttled", 0)) if st0 else None,
                 "pin_error": full.get("pin_error", "")})
    return {
        "value": round(mp / med * 1e3, 3), "unit": "MP/s", "cores": full["threads"],
        "pinned_to_cpus": hostinfo.format_cpus(chosen) if chosen else "unpinned", "kind": "port",
        "sample": f"{len(ms)} x the same {w}x{h} pair (median repetition), oracle/ssimu2_oracle.c (FIR, OpenMP, "
                  f"{full['threads']} threads, build {full['build']}), in a process of its own pinned to the chosen "
                  f"slice; not the reference's Zig+fssimu2 (unbuildable here)",
        "value_best_rep": round(mp / ms[0] * 1e3, 3),
        "single_thread_value": full.get("single_thread_MPps"),
        "single_thread_sample": f"1 x {w // 2}x{h // 2} crop, 1 thread",
        "placement": info, "_score": full["score"]}


def single_rank_collective(local_rank: int) -> dict:
    """N = 1: the `collective` record still travels the way an N > 1 job's does -- collective.open_group with a world of ONE
    rank on backend "nccl": the record through the rendezvous store first, then the RCCL process group opened on that store
    (device_id = this GPU, the communicator created eagerly) and the record confirmed by the all_gather of device tensors;
    then the other two collectives of an N > 1 line (all_reduce MAX, barrier).  Opened after the timed region so that RCCL's
    own streams cannot touch the measurement; bounded by a 60 s timeout; any failure is recorded, not raised (the
    throughput line does not depend on it)."""
    import torch
    import torch.distributed as dist
    from oavif_amd import collective, launch
    me = collective.rank_record(0, local_rank, local_rank, pinned=None)
    if os.environ.get("OAVIF_BENCH_COLLECTIVE", "1") == "0":
        return collective.describe("none", 1, [me], "not gathered (OAVIF_BENCH_COLLECTIVE=0)")
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(launch.free_port())
        coll, rc_ = collective.open_group(0, local_rank, local_rank, "nccl", 1, 1, pinned=None, label="bench.py", timeout_s=60.0)
        coll["gathered_through"] += "; an RCCL process group of one rank, opened after the timed region"
        if rc_ == 0:
            try:
                t_ = torch.tensor([1.0], dtype=torch.float64, device=torch.device("cuda", local_rank))
                dist.all_reduce(t_, op=dist.ReduceOp.MAX)      # the other collective of an N > 1 line (max over ranks)
                dist.barrier()
                torch.cuda.synchronize()
            finally:
                dist.destroy_process_group()
        return coll
    except Exception as e:
        c = collective.describe("nccl", 1, [me], "not gathered: the single-rank RCCL group failed")
        c["error"] = f"{type(e).__name__}: {str(e)[:300]}"
        return c


def main() -> int:
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-child":
        return cpu_baseline_child(sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks = GPUs of this node (default: 1, or the world a launcher announced)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--streams", type=int, default=2,
                    help="independent scorer contexts (HIP streams) the steps are dealt over")
    ap.add_argument("--pairs", type=int, default=8,
                    help="distinct (ref, dist) pairs per scorer context the steps rotate over")
    ap.add_argument("--no-by-resolution", action="store_true",
                    help="skip the by_resolution extra (512x512 ... 7680x4320): the rocprofv3 kernel-trace of a recorded round "
                         "uses this, so that its per-kernel averages are averages over 3840x2160 launches only")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's score and plane averages as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beside the headline figure: cache-resident rate, "
                         "rooflines, other blur modes and sizes, search passes, the CPU baseline, the N = 1 collective record")
    args = ap.parse_args()

    # One command for any N (the reference's batch entry is one command, scripts/measure.py:110-158; the driver's N = 1
    # shape is `python3 bench.py --gpus 1 ...`): asked for N > 1 ranks with no launcher's world in the environment, this
    # process starts N fresh copies of itself -- BEFORE torch is imported or a GPU touched -- relays rank 0's JSON line as
    # its own last stdout line and leaves with the first non-zero child code (oavif_amd/launch.py; a refusal stays rc 4).
    # Under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` the ranks run the same code.
    from oavif_amd import launch
    if args.gpus is None:   # not asked for: one GPU, or whatever world a launcher (torch.distributed.run) announced
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if launch.needs_self_launch(args.gpus):
        return launch.spawn_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus, label="bench.py")

    emit = claim_stdout()   # stdout carries the JSON line and nothing else (RCCL's banner, stray prints -> stderr)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    if world != args.gpus:   # a launcher announced another world than the command asks for
        print(f"bench.py: --gpus {args.gpus} but the launcher announced WORLD_SIZE={world}", file=sys.stderr)
        return 2
    # A rank of a multi-rank job pins itself to its slice of the host cores near its GPU before torch / HIP start
    # any thread (oavif_amd.hostinfo, as the batch driver does): the launch thread then sits on the GPU's NUMA node.
    pinned = None
    if world > 1 and os.environ.get("OAVIF_BENCH_NO_PIN", "") != "1":
        from oavif_amd import hostinfo as _hi
        pinned = bool(_hi.pin_rank(local_rank, local_world).pinned)

    import numpy as np
    import torch
    import torch.distributed as dist
    distributed = world > 1
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the scorer has no CPU fallback", file=sys.stderr)
        return 3
    # One process per GPU over RCCL (backend "nccl").  OAVIF_BENCH_BACKEND=gloo is a rehearsal
    # mode for boxes with fewer GPUs than ranks: ranks share devices (local_rank modulo the
    # device count) and the collectives run on CPU tensors; never used for reported numbers.
    backend = os.environ.get("OAVIF_BENCH_BACKEND", "nccl")
    from oavif_amd import collective
    if distributed:
        why = collective.preflight(backend, local_world)
        if why:   # every rank of the host sees the same count: all leave with the same code, nobody waits in a rendezvous
            print(f"bench.py: rank {rank}: refusing to run: {why}", file=sys.stderr)
            return 4
    if backend != "nccl":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    coll_dev = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")

    import oavif_amd
    from oavif_amd import synth

    # Before any communicator exists: every rank's description of itself travels through the rendezvous store and is
    # judged on every rank (collective.open_group).  A rank / device mix-up -- two ranks on one GPU is the case RCCL itself
    # answers with a hang -- ends the run here with rc 4 on every rank, no RCCL communicator ever created; only then is the
    # process group opened (eagerly, device_id = this rank's GPU) and the records are confirmed by one all_gather over it.
    # An RCCL failure at that point is printed with RCCL's own message on every rank and ends the run with rc 5.
    coll = None
    if distributed:
        coll, rc_ = collective.open_group(rank, int(os.environ.get("LOCAL_RANK", "0")), local_rank, backend, world, local_world,
                                          pinned=pinned, label="bench.py", timeout_s=300.0)
        if backend != "nccl":
            coll["note"] = "a rehearsal: ranks share devices and the collectives run on CPU tensors; never a reported number"
        if rc_:
            if rank == 0:
                emit({"metric": "ssimulacra2_megapixels_per_sec", "value": None,
                      "error": "placement refused" if rc_ == collective.RC_REFUSED else "process group failed",
                      "n_gpus": world, "collective": coll})
            return rc_

    w, h = args.width, args.height
    mp = w * h / 1e6
    # synthetic pairs of this rank (seeded): structured frame + 8x8 block quantisation, then
    # `pairs` x contexts distinct variants made on the device (the same horizontal roll / vertical
    # flip applied to both frames of a pair: distinct buffers, distinct content, same statistics)
    ref = synth.make_ref(w, h, seed=rank)
    dst = synth.distort(ref, "blockq", 2)
    t_ref = torch.from_numpy(ref).cuda().contiguous()
    t_dst = torch.from_numpy(dst).cuda().contiguous()
    nctx = max(1, args.streams)
    npairs = max(1, args.pairs)
    pairs = []   # [(ref tensor, dist tensor)] -- pairs[k] belongs to context k % nctx
    for k in range(nctx * npairs):
        if k == 0:
            pairs.append((t_ref, t_dst))
            continue
        shift = (k * w) // (nctx * npairs)
        a_, b_ = torch.roll(t_ref, shift, 1), torch.roll(t_dst, shift, 1)
        if k & 1:
            a_, b_ = a_.flip(0), b_.flip(0)
        pairs.append((a_.contiguous(), b_.contiguous()))
    assert all(a_.is_contiguous() and b_.is_contiguous() for a_, b_ in pairs)
    torch.cuda.synchronize()
    working_set_mb = len(pairs) * 2 * w * h * 3 / 1e6

    # Steps are independent scores (independent images / quantizer probes); they are dealt
    # round-robin over a few scorer contexts, each with its own HIP stream and scratch, so the
    # HBM-bound pyramid kernel and the latency-bound final reduction of one score overlap the
    # VALU-bound marching kernel of another.  Every step is still one full score.
    p_ref, p_dst = t_ref.data_ptr(), t_dst.data_ptr()
    ptrs = [(a_.data_ptr(), b_.data_ptr()) for a_, b_ in pairs]
    # Which hardware queues the contexts' streams land on is the library's business
    # (ssimu2_ctx_create places streams on distinct queues, oavif_amd/csrc/ssimu2_hip.hip "stream
    # placement"): the bench creates its contexts like any caller and keeps all of them.
    scorers = [oavif_amd.Ssimu2(local_rank) for _ in range(nctx)]
    scorer = scorers[0]

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    last = {}   # context -> the score of the last step it ran (what its wait() returned)

    def run_steps(n, rotate=True):
        """n scores dealt round-robin over the contexts; context c walks its own pairs
        (pairs[c], pairs[c + nctx], ...) when `rotate`, else every score is pair 0."""
        used = set()
        for i in range(n):
            c_ = i % nctx
            pr, pd = ptrs[c_ + nctx * ((i // nctx) % npairs)] if rotate else (p_ref, p_dst)
            scorers[c_].enqueue_device(pr, pd, w, h)
            used.add(c_)
        sc = None
        for j in sorted(used):
            sc = last[j] = scorers[j].wait()     # drains that context's stream
        return sc

    # Setup, not measurement: a fresh MI355X needs ~50 ms of work before its clocks settle (the
    # first 200 scores after idle run 7-8 % slower than every later batch,
    # scripts/gpu_streams_var.py), whatever --warmup the caller passes.
    run_steps(300)
    torch.cuda.synchronize()

    score = None
    if args.warmup:
        score = run_steps(args.warmup)

    # The timed region: EXACTLY `steps` steps, one block between barrier + synchronize on both sides,
    # max over ranks.  `--steps` is the number of steps timed, nothing more: a caller who wants a
    # steadier figure asks for more steps (ms_per_step says how many fit in a given time).
    own = []   # this rank's own work per block (up to its synchronize, before the closing barrier): shows a slow rank

    def timed_block():
        barrier()
        t_ = time.perf_counter()
        run_steps(args.steps)
        torch.cuda.synchronize()
        own.append(time.perf_counter() - t_)
        barrier()
        return time.perf_counter() - t_

    def max_over_ranks(x):
        if not distributed:
            return x
        t_ = torch.tensor([x], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t_, op=dist.ReduceOp.MAX)
        return float(t_.item())

    blocks = [max_over_ranks(timed_block())]
    elapsed = blocks[0]

    # what the last timed step computed, read back before any later work reuses its context
    if args.dump_outputs and rank == 0 and args.steps > 0:
        c_last = (args.steps - 1) % nctx
        dumped = {"score": np.array([last[c_last]], dtype=np.float64),
                  "plane_averages": np.asarray(scorers[c_last].last_averages()[0], dtype=np.float64)}
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in dumped.items():
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), arr)

    if args.full:
        # the labelled extra: the same number of steps on ONE pair (inputs and pyramid stay in the
        # Infinity Cache) -- what round 1 reported as `value`
        run_steps(min(args.steps, 200), rotate=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        score = run_steps(args.steps, rotate=False)   # = the score of pair 0
        torch.cuda.synchronize()
        elapsed_resident = time.perf_counter() - t1
    else:
        score = run_steps(1, rotate=False)            # the score of pair 0, what `scores` carries in either run

    own_median = sorted(own)[len(own) // 2]
    rec = torch.tensor([float(rank), float(score), own_median], dtype=torch.float64, device=coll_dev)
    if distributed:
        gathered = [torch.zeros_like(rec) for _ in range(world)]
        dist.all_gather(gathered, rec)   # the final RCCL gather of per-rank result records
        scores = [float(g[1]) for g in gathered]
        per_rank_ms = [round(float(g[2]) / args.steps * 1e3, 5) for g in gathered]   # each rank's OWN work per step
    else:
        scores = [float(score)]
        per_rank_ms = None
    t = elapsed
    if distributed:
        # The job's last collective is behind it: every rank leaves the process group HERE, together (barrier, then
        # destroy), before rank 0 starts its single-GPU extras (roofline, recursive mode, hand-off) -- no rank sits in an
        # RCCL kernel for the tens of seconds those take (VERDICT r05 / ADVICE r05), and ranks 1..N-1 are done.
        dist.barrier()
        if backend == "nccl":
            torch.cuda.synchronize()
        dist.destroy_process_group()

    if rank == 0:
        value = world * args.steps * mp / t
        out = {
            "metric": "ssimulacra2_megapixels_per_sec",
            "value": round(value, 2),
            "unit": "MP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t / args.steps * 1e3, 5),
            "repeats": len(blocks),
            "ms_per_step_min": round(min(blocks) / args.steps * 1e3, 5),
            "ms_per_step_max": round(max(blocks) / args.steps * 1e3, 5),
            "timed_region_s": round(sum(blocks), 4),
            "timing_note": f"the {args.steps} steps timed as one block (barrier + synchronize around it, max over "
                           "ranks); ms_per_step and value are that block",
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"ssimulacra2 score of one {w}x{h} RGB8 (ref, dist) pair per "
                                   f"step per GPU (BASELINE configs[1]); steps rotate over "
                                   f"{len(pairs)} distinct pairs per GPU = {working_set_mb:.0f} MB "
                                   f"of frames resident in HBM (> the 256 MiB Infinity Cache)",
                       "width": w, "height": h, "pairs_per_step": world,
                       "distinct_pairs_per_gpu": len(pairs), "input_working_set_MB": round(working_set_mb, 1),
                       "parallelism": f"image-per-gpu x{world}" if world > 1 else "single gpu",
                       "streams_per_gpu": nctx,
                       "kernels": oavif_amd.version()},
            "scores": [round(s, 6) for s in scores],
        }
        if coll is not None:
            out["collective"] = coll
        if per_rank_ms is not None:
            # each rank's own work per step, up to its synchronize and before the closing barrier: `ms_per_step`
            # is the max over ranks of the whole block, so a rank that is slower than the others shows here
            out["per_rank_own_ms_per_step"] = per_rank_ms
        if args.full:
            out["cache_resident"] = {
                "value": round(args.steps * mp / elapsed_resident, 2),
                "unit": "MP/s per GPU", "ms_per_step": round(elapsed_resident / args.steps * 1e3, 5),
                "note": "rank 0's GPU only: every step scores the SAME pair, so inputs and pyramid are served "
                        "by the Infinity Cache; not `value`"}

    def measure_beside(out):
        """--full, rank 0, every rank out of the process group: what the line carries beside the headline figure."""
        # ---- roofline of the dominant kernel, measured live with HIP events ----------------
        # (instrumented build of the same sources: the product library exports no timing hooks)
        from oavif_amd import _lib
        iscorer = oavif_amd.Ssimu2(local_rank, instrumented=True)
        iters = 96
        k_ms = iscorer.time_march_rotating([p[0] for p in ptrs], [p[1] for p in ptrs], w, h, iters)
        k_ms_res = iscorer.time_stage(p_ref, p_dst, w, h, _lib.STAGE_MARCH, 50)
        pyr_ms = iscorer.time_stage(p_ref, p_dst, w, h, _lib.STAGE_PYRAMID, 50)
        fin_ms = iscorer.time_stage(p_ref, p_dst, w, h, _lib.STAGE_FINALIZE, 50)
        algo_bytes = ALGO_BYTES_PER_PX_MARCH * w * h
        achieved = algo_bytes / (k_ms * 1e-3) / 1e9
        blur_frac = ALGO_BYTES_PER_PX_BLUR * w * h / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        ctr = load_counters((w, h))
        traffic = ctr.get("march_hbm_bytes_per_launch") if ctr else None
        out["roofline"] = {
            "bound": "hbm", "kernel": "k_march (fused XYB + blur + maps, all 6 scales)",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
            "kernel_ms": round(k_ms, 5),
            "kernel_ms_note": f"average of {iters} launches rotating over the {len(pairs)} pairs (HBM-fed), HIP events "
                              f"on the kernel's stream; same pair over and over: {k_ms_res:.5f} ms",
            "kernel_ms_cache_resident": round(k_ms_res, 5),
            "algorithmic_bytes": int(algo_bytes),
            "model": "SURVEY 8(d) W-model minus the pyramid writes: 77.97 B/px",
            # north_star's own figure: the blur pyramid alone (B-model, 31.99 B/px) against the
            # same kernel time, with its >= 70 % target
            "blur_pyramid_frac": round(blur_frac, 4),
            "blur_pyramid": {"model": "SURVEY 8(d) B-model: 31.99 B/px", "target": 0.70,
                             "met": bool(blur_frac >= 0.70)},
            "limiter": "valu-issue (see valu_roofline): the fused kernel moves far fewer bytes than the "
                       "model charges, HBM is idle most of the time"}
        if traffic:
            out["roofline"]["measured_traffic_GBps"] = round(traffic / (k_ms * 1e-3) / 1e9, 1)
            out["roofline"]["measured_traffic_frac_of_peak"] = round(traffic / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        if ctr:
            out["roofline"]["counters"] = {k_: ctr[k_] for k_ in ("source", "stale", "kernel_source_hash") if k_ in ctr}
        # the same figure against the read-stream bandwidth this device delivers to a plain
        # 16-byte-per-lane read kernel in the same run ("also report against a measured
        # device-copy/read-stream ceiling"); rank 0 only, 2 GiB >> the 256 MB Infinity Cache
        try:
            stream_gbs = iscorer.measure_read_stream(2 << 30, 10)
            out["roofline"]["measured_read_stream_GBps"] = round(stream_gbs, 1)
            out["roofline"]["frac_of_measured_read_stream"] = round(achieved / stream_gbs, 4)
        except Exception as e:
            out["roofline"]["measured_read_stream_GBps"] = f"error: {e}"
        # What the blur-pyramid roofline looks like when it is NOT fused away: the same marching
        # body as a plain blur stage (k_ref_blur: positive-XYB planes of one frame in, one blurred
        # plane per channel out, all six scales in one launch), rotating over 8 frames' plane sets
        # (HBM-fed), algorithmic bytes = every plane element read once and written once.
        try:
            b_ms, b_bytes = iscorer.time_blur_stage_rotating([p[0] for p in ptrs[:8]], w, h, 48)
            b_gbs = b_bytes / (b_ms * 1e-3) / 1e9
            out["roofline"]["blur_stage_unfused"] = {
                "kernel": "k_ref_blur (the marching body as a plain HBM-to-HBM blur stage, one plane per channel)",
                "ms": round(b_ms, 5), "algorithmic_bytes": int(b_bytes), "achieved": round(b_gbs, 1),
                "unit": "GB/s", "frac": round(b_gbs / HBM_PEAK_GBS, 4),
                "note": "a blur pyramid built from such HBM-to-HBM stages would show 2-3x the roofline fraction of "
                        "the fused kernel and take ~5x its time; k_march keeps the 15 blurred planes in registers"}
        except Exception as e:
            out["roofline"]["blur_stage_unfused"] = f"error: {e}"
        # what actually bounds the kernel: VALU issue.  Instruction count from this round's PMC
        # run; two peaks: the nominal one (a wave64 VALU instruction per 2 cycles at 2.4 GHz) and
        # the one a plain v_mul/v_add stream reaches on this chip at 8 waves per SIMD.
        if ctr and ctr.get("march_valu_wave_instructions_per_launch") and (w, h) == (W, H):
            n_valu = ctr["march_valu_wave_instructions_per_launch"]
            rate = n_valu / (k_ms * 1e6) / ctr.get("simds", 1024)
            nominal = 2.4 / 2.0
            measured = ctr.get("measured_peak_valu_wave_instructions_per_ns_per_simd")
            out["valu_roofline"] = {
                "kernel": "k_march", "achieved": round(rate, 4), "unit": "VALU wave-instructions/ns/SIMD",
                "peak_nominal": nominal, "frac_nominal": round(rate / nominal, 4),
                "peak_measured": measured, "frac_measured": round(rate / measured, 4) if measured else None,
                "valu_wave_instructions": n_valu, "stale": ctr.get("stale"),
                "note": "instruction count: SQ_INSTS_VALU of this round's PMC run (profiles/counters.json); "
                        "time: live.  Slow encodings (v_rcp 3.4x, SDWA / v_cndmask with an SGPR mask / "
                        "v_mul_hi / 64-bit adds 1.7x a plain op) make the true ceiling lower than either peak"}
        out["stages_ms"] = {"pyramid": round(pyr_ms, 5), "march": round(k_ms, 5),
                            "march_cache_resident": round(k_ms_res, 5), "finalize": round(fin_ms, 5)}
        # whole-score view (all kernels of one score, W-model 85.97 B/px), one stream, rotating pairs
        torch.cuda.synchronize()
        n_ws = 4 * len(ptrs)
        for i_ in range(len(ptrs)):
            scorer.enqueue_device(ptrs[i_][0], ptrs[i_][1], w, h)
        scorer.wait()
        tt = time.perf_counter()
        for i_ in range(n_ws):
            scorer.enqueue_device(ptrs[i_ % len(ptrs)][0], ptrs[i_ % len(ptrs)][1], w, h)
        scorer.wait()
        score_ms = (time.perf_counter() - tt) / n_ws * 1e3
        out["score_roofline"] = {
            "ms_per_score_one_stream": round(score_ms, 5),
            "achieved": round(ALGO_BYTES_PER_PX_SCORE * w * h / (score_ms * 1e-3) / 1e9, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(ALGO_BYTES_PER_PX_SCORE * w * h / (score_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        # what a second context buys (stream placement, DESIGN section 4 "Two scores in flight"): the timed
        # two-context step against one context scoring the same rotation.  A reported number, not a test
        # criterion (tests/test_gpu_streams.py asserts collision detection only): 0.84-0.89 across boxes;
        # 1.0 would mean the two contexts' streams share a hardware queue.
        if nctx >= 2:
            out["two_context_ratio"] = {"value": round(out["ms_per_step"] / score_ms, 3),
                                        "ms_per_score_two_contexts": out["ms_per_step"],
                                        "ms_per_score_one_context": round(score_ms, 5),
                                        "placed_streams": iscorer.placed_streams(),
                                        "placed_streams_note": "size of the placed set of the INSTRUMENTED library instance of this "
                                                               "process (same placement code as the product instance, its own probe)"}
        iscorer.close()

        # ---- the search's per-pass score: reference cached on the device (tq.zig:37 passes the
        # same e.rgb every pass), distorted frame already in HBM -------------------------------
        scorer.set_reference_device(p_ref, w, h)
        for _ in range(10):
            scorer.enqueue_against_reference_device(p_dst)
        scorer.wait()
        torch.cuda.synchronize()
        tt = time.perf_counter()
        n_c = 400
        for _ in range(n_c):
            scorer.enqueue_against_reference_device(p_dst)
        c_score = scorer.wait()
        torch.cuda.synchronize()
        c_ms = (time.perf_counter() - tt) / n_c * 1e3
        out["cached_reference"] = {"ms_per_score": round(c_ms, 5), "MP_per_s": round(mp / c_ms * 1e3, 1),
                                   "bit_identical_to_pair_score": bool(c_score == scores[0]),
                                   "note": "reference pyramid, XYB and blur(ref^2) planes cached by ssimu2_set_reference; "
                                           "one stream; separate from `value`"}

        # ---- the published-recursion blur modes (ssimu2_ctx_set_blur): what a search pays per pass
        # if fssimu2 turns out to blur recursively; reported beside, never `value` ---------------
        from oavif_amd import _lib as _abi
        with oavif_amd.Ssimu2(local_rank, blur=_abi.BLUR_RECURSIVE) as rsc:
            r_score = rsc.score_device(p_ref, p_dst, w, h)
            for i_ in range(len(ptrs)):
                rsc.enqueue_device(ptrs[i_][0], ptrs[i_][1], w, h)
            rsc.wait()
            torch.cuda.synchronize()
            tt = time.perf_counter()
            n_r = 3 * len(ptrs)
            for i_ in range(n_r):
                rsc.enqueue_device(ptrs[i_ % len(ptrs)][0], ptrs[i_ % len(ptrs)][1], w, h)
            rsc.wait()
            torch.cuda.synchronize()
            r_ms = (time.perf_counter() - tt) / n_r * 1e3
            # the search's case: reference planes (XYB, blur(x), blur(x*x) by the recursion) cached
            # once, every pass recurses the 9 planes that depend on the distorted frame
            tt = time.perf_counter()
            n_sr = 8
            for i_ in range(n_sr):
                rsc.set_reference_device(ptrs[i_ % len(ptrs)][0], w, h)
            torch.cuda.synchronize()
            sr_ms = (time.perf_counter() - tt) / n_sr * 1e3
            rsc.set_reference_device(p_ref, w, h)
            rsc.enqueue_against_reference_device(p_dst)
            rc_score = rsc.wait()
            dists = [p_dst] + [p[1] for p in ptrs[1:]]   # other frames of the same size: HBM-fed passes
            for d_ in dists:
                rsc.enqueue_against_reference_device(d_)
            rsc.wait()
            torch.cuda.synchronize()
            tt = time.perf_counter()
            n_rc = 6 * len(dists)
            for i_ in range(n_rc):
                rsc.enqueue_against_reference_device(dists[i_ % len(dists)])
            rsc.wait()
            torch.cuda.synchronize()
            rc_ms = (time.perf_counter() - tt) / n_rc * 1e3
            # the same pass as the boundary sees it (host `dist` in, score out): what the search path's
            # default mode costs per pass on the GPU side
            rsc.set_reference(ref)
            rsc.score_against_reference(dst)
            tt = time.perf_counter()
            for _ in range(5):
                rsc.score_against_reference(dst)
            r_host_ms = (time.perf_counter() - tt) / 5 * 1e3
            rsc.set_blur(_abi.BLUR_RECURSIVE_FMA)
            rf_score = rsc.score_device(p_ref, p_dst, w, h)
        # planes of the recursive modes keep their rows padded to 128 floats (ssimu2_recursive.h "Row pitch")
        n_pad = sum((((w + (1 << k) - 1) >> k) + 127) // 128 * 128 * ((h + (1 << k) - 1) >> k) for k in range(6))
        out["recursive_blur_mode"] = {
            "ms_per_score": round(r_ms, 4), "MP_per_s": round(mp / r_ms * 1e3, 1),
            "cached_reference": {"ms_per_pass": round(rc_ms, 4), "MP_per_s": round(mp / rc_ms * 1e3, 1),
                                 "ms_set_reference": round(sr_ms, 4),
                                 "bit_identical_to_pair_score": bool(rc_score == r_score),
                                 "note": f"passes rotate over {len(dists)} distorted frames (HBM-fed), one stream"},
            "ms_per_search_pass_gpu_side": round(r_host_ms, 4),
            "score_recursive": round(r_score, 6), "score_recursive_fma": round(rf_score, 6),
            "score_default_fir": round(scores[0], 6),
            "device_memory_MB": {"reference_cache": round(9 * n_pad * 4 / 1e6, 1),
                                 "per_pass_scratch": round(12 * n_pad * 4 / 1e6, 1)},
            "note": "SSIMU2_BLUR_RECURSIVE: the published recursive Gaussian operation for operation (planes "
                    "bit-identical to the oracle's OR_BLUR_IIR): one line = three lanes, all scales in one launch "
                    "per stage, reference planes cached per search, v-pass fused with the maps and persistent "
                    "(one workgroup per CU); the default of the SEARCH path (shim, CLI, batch) since round 4, "
                    "`value` stays the FIR mode"}

        # the mode the SEARCH path runs by default (shim, CLI mirror, batch driver, C host): one cached-reference
        # pass of the published recursion per probe -- beside `value`, which is FIR pair scoring on two contexts
        out["default_search_mode"] = {
            "blur": "recursive (SSIMU2_BLUR_RECURSIVE)", "what": "one cached-reference pass per probe, one stream, inputs in HBM",
            "ms_per_pass": round(rc_ms, 4), "MP_per_s": round(mp / rc_ms * 1e3, 1),
            "ms_per_pass_from_host_memory": round(r_host_ms, 4),
            "value_is": "FIR pair scoring on two contexts (SSIMU2_BLUR_FIR, a bare context's mode): "
                        f"{out['value']} MP/s; the same cached-reference pass in FIR mode: {out['cached_reference']['MP_per_s']} MP/s",
            "parity": "both modes are checked against this repository's CPU oracle only; fssimu2 parity unpinned"}

        # per-kernel rooflines of the recursive pass: its four launches timed LIVE where they run (instrumented build, HIP events
        # on the pass's own stream around each launch, passes rotating over the distorted frames) with their algorithmic bytes
        # (planes as the kernels address them: rows padded to 128 floats); the product library's whole-pass time above is the
        # cross-check (their sum), the committed rocprofv3 averages a second one
        try:
            with oavif_amd.Ssimu2(local_rank, instrumented=True, blur=_abi.BLUR_RECURSIVE) as irsc:
                st_ms, st_wt, st_wp = irsc.time_kernels(w, h, dists, 48, d_ref=p_ref, recursive=True)
            out["recursive_blur_mode"]["kernels"] = recursive_kernel_rooflines(w, h, rc_ms, st_ms, st_wt, st_wp)
        except Exception as e:  # the record is optional
            out["recursive_blur_mode"]["kernels"] = {"error": str(e)[:200]}

        # ---- the named resolutions (north_star): 512^2, 1080p, 4K, 8K -- N = 1 only ----
        if world == 1 and (w, h) == (W, H) and not args.no_by_resolution:
            try:
                t_br = time.perf_counter()
                out["by_resolution"] = {"sizes": by_resolution(local_rank, t_ref, t_dst, scorers),
                                        "seconds": None,
                                        "note": "MP = scale-0 pixels of one image; every input resident in HBM, rotating over "
                                                "`distinct_pairs` pairs (> 256 MiB of frames); w_model_frac = 85.97 B/px x pixels / "
                                                "time / 8 TB/s (SURVEY 8d W-model, a model fraction); parity of every size: this "
                                                "repository's CPU oracle only (fssimu2 parity unpinned)"}
                out["by_resolution"]["seconds"] = round(time.perf_counter() - t_br, 2)
            except Exception as e:
                out["by_resolution"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}

        # ---- one search pass as the boundary sees it: host `dist` in, score out ---------------
        scorer.set_reference(ref)
        scorer.score_against_reference(dst)
        tt = time.perf_counter()
        n_pass = 5
        for _ in range(n_pass):
            scorer.score_against_reference(dst)
        out["ms_per_search_pass_4k_gpu_side"] = round((time.perf_counter() - tt) / n_pass * 1e3, 4)
        out["search_pass_note"] = ("pageable host dist -> H2D -> score -> D2H score; excludes the "
                                   "CPU libaom encode / dav1d decode of the pass")
        # decoded-frame hand-off: libavif's RGBA rows scored as they are
        # (alpha dropped on the device) vs the reference's CPU copy loop (io.zig:654-663, timed
        # through the oracle's restatement) followed by the tight-RGB pass above
        rgba = np.concatenate([dst, np.full((h, w, 1), 255, np.uint8)], axis=2)
        s_rgba = scorer.score_decoded_against_reference(rgba)
        tt = time.perf_counter()
        for _ in range(n_pass):
            scorer.score_decoded_against_reference(rgba)
        ms_rgba = (time.perf_counter() - tt) / n_pass * 1e3
        handoff = {"ms_per_pass_rgba_strided_gpu_side": round(ms_rgba, 4),
                   "bit_identical_to_tight_rgb": bool(s_rgba == scores[0])}
        if world == 1 and not args.no_cpu_baseline:
            from oracle import ssimu2_oracle as orc_copy  # checker / CPU timing only
            orc_copy.build()
            orc_copy.copy_rgb_pixels(rgba)
            tt = time.perf_counter()
            for _ in range(3):
                orc_copy.copy_rgb_pixels(rgba)
            handoff["ms_cpu_copy_loop_io_zig_654"] = round((time.perf_counter() - tt) / 3 * 1e3, 3)
        out["decoded_frame_handoff_4k"] = handoff

        # ---- one REAL search pass end to end (tq.zig:21-38): CPU encode -> CPU decode -> upload -> GPU
        # score, through libavif's C API with the reference's own calls and defaults (oavif_amd.avif_bridge:
        # YUV444, tune=iq, speed 9, ONE encoder thread, parse_args.zig:48-63); the decoded frame goes to the
        # scorer in libavif's rows.  Pillow's plugin only if the bridge is unavailable ----
        codec4k, codec_label = None, None
        if world == 1 and synth.have_avif() and not args.no_cpu_baseline:
            try:
                from oavif_amd import avif_bridge as _ab
                from oavif_amd import cli as _cli
                if _ab.available():
                    _o = _cli.AvifEncOptions()
                    _depth, _dnote = _cli.codec_depth(_o.tenbit, False)
                    t_p = time.perf_counter()
                    _scaled = _ab.prescale_source(ref, _depth)          # once per image ...
                    _src = _ab.EncoderSource(_scaled, _depth, _o)       # ... and so is the YUV444 conversion
                    prep_ms = (time.perf_counter() - t_p) * 1e3
                    codec_label = (f"{_ab.versions()} through oavif_amd.avif_bridge: the reference's calls and defaults "
                                   f"(YUV444, tune={_o.tune}, speed {_o.speed}, {_o.max_threads} encoder thread), "
                                   f"{_depth}-bit" + (" (the reference's default is 10-bit: this image's libaom has no "
                                                      "high-bit-depth support)" if _dnote else ""))

                    def codec4k(q):
                        d_ = _src.encode(_o, q)
                        return _ab.decode_rgb8(d_), len(d_)
                    t_e = time.perf_counter()
                    data = _src.encode(_o, 65)
                    t_d = time.perf_counter()
                    frame = _ab.decode_common(data)
                    t_s = time.perf_counter()
                    real_score = scorer.score_decoded_against_reference(frame.rows.reshape(-1), frame.row_bytes,
                                                                        frame.channels)
                    t_x = time.perf_counter()
                    frame.close()
                else:
                    codec_label = f"Pillow's libavif plugin (bridge unavailable: {_ab.why_unavailable()}), 1 encoder thread"
                    codec4k = lambda q: synth.avif_roundtrip(ref, q, speed=9, max_threads=1)
                    t_e = time.perf_counter()
                    data = synth.avif_encode(ref, 65, speed=9, max_threads=1)
                    t_d = time.perf_counter()
                    dec = synth.avif_decode(data)
                    t_s = time.perf_counter()
                    real_score = scorer.score_against_reference(dec)
                    t_x = time.perf_counter()
                out["search_pass_end_to_end_4k"] = {
                    "encode_ms": round((t_d - t_e) * 1e3, 1), "decode_ms": round((t_s - t_d) * 1e3, 1),
                    "upload_plus_score_ms": round((t_x - t_s) * 1e3, 3), "q": 65,
                    "score": round(real_score, 4), "avif_bytes": len(data), "codec": codec_label,
                    "note": "the GPU share of a pass is the last term; libaom encode dominates"}
                if _ab.available():
                    out["search_pass_end_to_end_4k"]["source_to_yuv444_once_ms"] = round(prep_ms, 1)
                    out["search_pass_end_to_end_4k"]["hoist_note"] = (
                        "encode_ms is avifEncoderAddImage + Finish alone: the avifImage of the source (pre-scaling, "
                        "avifImageRGBToYUV) is made once per image (source_to_yuv444_once_ms), where "
                        "io.encodeAvifToBuffer rebuilds it on every pass (io.zig:550-623)")
            except Exception as e:  # the codec is not part of the measured path
                out["search_pass_end_to_end_4k"] = {"error": str(e)}

        # ---- one whole 4K search, sequential vs probes fanned over contexts/streams + host
        # threads: same result, waves instead of passes of encode latency.
        # Encoder threads = 1 as oavif defaults (--max-threads, parse_args.zig:51), which is
        # what leaves host cores idle for speculative probes -------------------------------------
        if world == 1 and codec4k is not None and not args.no_cpu_baseline:
            try:
                from oavif_amd import tq as _tqs
                fan = max(1, min(6, (usable_cores() or 2) - 2))
                ctxs = [oavif_amd.Ssimu2(local_rank) for _ in range(fan)]
                cases = []
                try:
                    for tgt in (80.0, 70.0, 60.0):
                        t0 = time.perf_counter()
                        seq = _tqs.search_hip(scorer, ref, codec4k, score_tgt=tgt)
                        t1 = time.perf_counter()
                        spec, st, _ = _tqs.search_speculative_hip(ctxs, ref, codec4k, score_tgt=tgt)
                        t2 = time.perf_counter()
                        cases.append({"target": tgt, "q": seq.q, "passes": seq.num_pass,
                                      "sequential_ms": round((t1 - t0) * 1e3, 1),
                                      "speculative_ms": round((t2 - t1) * 1e3, 1),
                                      "waves": st.waves, "probes_issued": st.probes_issued,
                                      "identical_result": bool((spec.q, spec.score, spec.history) ==
                                                               (seq.q, seq.score, seq.history))})
                finally:
                    for c_ in ctxs:
                        c_.close()
                out["search_end_to_end_4k"] = {
                    "fanout": fan, "encoder_threads": 1, "cases": cases, "codec": codec_label,
                    "note": "the first wave of the "
                            "speculative search is the model's guess alone (first_wave_fanout = 1), so a "
                            "search that ends on its first pass issues one probe like the sequential one; "
                            "speculation (and the reference upload to further contexts) starts with wave 2"}
            except Exception as e:
                out["search_end_to_end_4k"] = {"error": str(e)}

        # ---- quantizer match vs CPU: the same search (tq.zig:124-210) driven by the HIP scorer
        # and by the CPU oracle, same CPU codec, small frames so the oracle stays quick ---------
        if world == 1 and synth.have_avif() and not args.no_cpu_baseline:
            try:
                from oavif_amd import tq as _tq
                from oracle import ssimu2_oracle as _orc
                from oracle import tq_oracle as _tqo
                _orc.build()
                same, worst, cases = True, 0.0, []
                for seed, tgt in ((0, 80.0), (1, 65.0), (2, 90.0)):
                    r0 = synth.make_ref(384, 256, 500 + seed)
                    cache = {}

                    def codec(q, r0=r0, cache=cache):
                        if q not in cache:
                            cache[q] = synth.avif_roundtrip(r0, q, speed=9)
                        return cache[q]
                    g = _tq.search_hip(scorer, r0, codec, score_tgt=tgt)
                    cpu = _tqo.find_target_quality(
                        lambda q: _orc.compute_ssimu2(r0, codec(q)[0], _orc.BLUR_FIR), score_tgt=tgt)
                    ok = ([q for q, _ in g.history] == [q for q, _ in cpu.history]) and g.q == cpu.q
                    same = same and ok
                    worst = max([worst] + [abs(a[1] - b[1]) for a, b in zip(g.history, cpu.history)])
                    cases.append({"target": tgt, "q_hip": g.q, "q_cpu": cpu.q, "passes": g.num_pass})
                out["quantizer_match_vs_cpu"] = {"identical": bool(same), "max_abs_dscore": worst,
                                                 "cases": cases,
                                                 "cpu": "oracle/ssimu2_oracle.c (fssimu2 parity unpinned)"}
            except Exception as e:
                out["quantizer_match_vs_cpu"] = {"error": str(e)}

        # ---- external pin on the device: the calibration ladder SSIMULACRA2 was published with (libjpeg-turbo
        # quality 14 ... 95 <-> scores 10 ... 90; tests/photo_ladder.py) on the two photographs scikit-learn ships,
        # scored by the HIP path in both blur modes.  Not a timing: a sanity line beside `quantizer_match_vs_cpu` ----
        if world == 1 and not args.no_cpu_baseline:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from photo_ladder import LADDER, jpeg_round_trip, photographs
                photos = photographs()
                if photos:
                    rungs = []
                    with oavif_amd.Ssimu2(local_rank, blur=oavif_amd._lib.BLUR_RECURSIVE) as rsc2:
                        for q_, sub_, pub_ in LADDER:
                            f_, r_ = [], []
                            for _n, ph in photos:
                                dj = jpeg_round_trip(ph, q_, sub_)
                                f_.append(scorer.compute_ssimu2(ph, dj))
                                r_.append(rsc2.compute_ssimu2(ph, dj))
                            rungs.append({"libjpeg_quality": q_, "subsampling": {2: "4:2:0", 1: "4:2:2", 0: "4:4:4"}[sub_],
                                          "published_score": pub_, "hip_fir_mean": round(float(np.mean(f_)), 2),
                                          "hip_recursive_mean": round(float(np.mean(r_)), 2)})
                    out["published_quality_ladder"] = {
                        "rungs": rungs, "photographs": [n for n, _ in photos],
                        "max_abs_deviation_recursive": round(max(abs(r["hip_recursive_mean"] - r["published_score"]) for r in rungs), 2),
                        "note": "weak EXTERNAL pin: the table is the published calibration of SSIMULACRA2 (average output of "
                                "each libjpeg-turbo setting over the authors' corpus), the images are two photographs; "
                                "fssimu2 parity itself stays unpinned"}
            except Exception as e:
                out["published_quality_ladder"] = {"error": str(e)[:200]}

        # ---- N = 1: the collective record through a single-rank RCCL group (after every GPU measurement) ----
        if world == 1:
            out["collective"] = single_rank_collective(local_rank)

        # ---- CPU baseline: the oracle on this host's cores (N = 1 only) ----------------------
        if world == 1 and not args.no_cpu_baseline:
            try:
                cb = measure_cpu_baseline(w, h, mp)
                cb["score_abs_diff_vs_hip"] = abs(cb.pop("_score") - scores[0])
                out["cpu_baseline"] = cb
            except Exception as e:
                out["cpu_baseline"] = {"error": str(e)[:300], "kind": "port"}

    if rank == 0:
        if args.full:
            measure_beside(out)
        emit(out)

    for sc_ in scorers:
        sc_.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
