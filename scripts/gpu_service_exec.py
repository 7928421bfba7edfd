"""What the resident scoring service buys the one-process-per-image flow, on one MI355X.

Per-image processes: N synthetic 1920x1080 PNGs through `python -m oavif_amd.batch --exec` with the compiled C host as
the per-image program, A = as it is (every process starts HIP), B = the same with --service, run A B A B, one at a time
and four at a time; beside them the in-process one-at-a-time rate of the same images (the ceiling), and the host's own
time inside main() (OAVIF_HOST_TIMES) for a few images each way.
Per pass: host-call time of ssimu2_score_against_reference_strided (RGBA, SSIMU2_BLUR_RECURSIVE) at 1080p and 4K,
in process and through the service, from ordinary memory and from ssimu2_host_alloc memory.

Every step is a child process under a time limit, or a timed loop in this process; the first failure ends the run.

    python scripts/gpu_service_exec.py [--images 96] [--out profiles/service_exec.json]
"""
import argparse
import csv
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(cmd, env, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{cmd!r} left with {r.returncode}:\n{r.stderr[-2000:]}")
    return r, time.perf_counter() - t0


def batch_rate(imgs, work, tag, env, program, options, limit=600):
    js = os.path.join(work, f"{tag}.json")
    cmd = [sys.executable, "-m", "oavif_amd.batch", imgs, *program, os.path.join(work, f"{tag}.csv"), *options, "--out-dir",
           os.path.join(work, f"o_{tag}"), "--collective-json", js]
    run(cmd, env, limit)
    with open(js) as f:
        rec = json.load(f)
    if rec["images_ok"] != rec["images"]:
        raise SystemExit(f"{tag}: {rec['images_ok']} of {rec['images']} images")
    with open(os.path.join(work, f"{tag}.csv")) as f:
        rows = sorted((r[0], r[2], r[6]) for r in csv.reader(f))      # name, the columns the search decides
    return rec["images_per_s"], rows


def host_main_ms(host, files, work, env):
    """Milliseconds from the host's first stamp to its last (OAVIF_HOST_TIMES): the time inside main()."""
    out = []
    for i, path in enumerate(files):
        r, _ = run([host, path, os.path.join(work, f"t{i}.avif")], dict(env, OAVIF_HOST_TIMES="1"), 120)
        stamps = [float(m) for m in re.findall(r"^\s+\[\s*([0-9.]+) ms\]", r.stderr, re.M)]
        out.append(max(stamps))
    return out


def per_pass(sock, sizes, iters):
    import numpy as np
    from oavif_amd import Ssimu2, _lib, synth
    table = []
    for w, h in sizes:
        ref = synth.make_ref(w, h, 7)
        rgba = np.dstack([synth.distort(ref, "blockq", 2), np.full((h, w), 255, np.uint8)])
        for where, service in (("in process", None), ("service", sock)):
            with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, service=service) as s:
                s.set_reference(ref)
                for memory in ("ordinary", "ssimu2_host_alloc"):
                    buf = rgba
                    if memory == "ssimu2_host_alloc":
                        buf = s.host_alloc(rgba.shape)
                        buf[:] = rgba
                    flat, times = buf.reshape(-1), []
                    for i in range(iters + 5):
                        t0 = time.perf_counter()
                        score = s.score_decoded_against_reference(flat, w * 4, 4)
                        if i >= 5:
                            times.append((time.perf_counter() - t0) * 1e3)
                    table.append({"w": w, "h": h, "where": where, "memory": memory, "score": score,
                                  "ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
                                  "ms_p90": round(sorted(times)[int(0.9 * len(times))], 4), "calls": len(times)})
                    if buf is not rgba:
                        s.host_free(buf)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "service_exec.json"))
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    from PIL import Image
    from oavif_amd import avif_bridge, build, service, synth
    build.build()
    work = tempfile.mkdtemp(prefix="oavif_service_exec_")
    imgs = os.path.join(work, "imgs")
    os.makedirs(imgs)
    for i in range(a.images):
        Image.fromarray(synth.make_ref(1920, 1080, 900 + i)).save(os.path.join(imgs, "img%03d.png" % i), compress_level=1)
    env = {k: v for k, v in os.environ.items() if k != service.ENV}
    if avif_bridge._find_library():
        env.setdefault("OAVIF_LIBAVIF", avif_bridge._find_library())
    host = build.HOST_PATH
    rec = {"images": a.images, "size": "1920x1080", "target": 80, "host": "oavif_amd/lib/oavif_host", "per_image": {}}
    rows = {}
    try:
        for workers in (1, 4):
            runs = {"A": [], "B": []}
            for rep in range(a.repeats):
                for mode, extra in (("A", []), ("B", ["--service"])):
                    rate, rows[(mode, workers, rep)] = batch_rate(imgs, work, f"{mode}{workers}_{rep}", env,
                                                                  [host], ["--exec", *extra, "--workers", str(workers)])
                    runs[mode].append(rate)
                    print(f"workers {workers} {mode} run {rep}: {rate} images/s", flush=True)
            rec["per_image"][f"{workers} at a time"] = {
                "A_images_per_s": runs["A"], "B_service_images_per_s": runs["B"],
                "spread_A": round(max(runs["A"]) - min(runs["A"]), 3), "spread_B": round(max(runs["B"]) - min(runs["B"]), 3)}
        rec["same_rows_every_run"] = len({tuple(v) for v in rows.values()}) == 1     # q, score, passes, bytes per image
        rate, _ = batch_rate(imgs, work, "inproc", env, [], ["--workers", "1"])
        rec["in_process_one_at_a_time_images_per_s"] = rate
        few = sorted(os.path.join(imgs, f) for f in os.listdir(imgs))[:8]
        with service.start(max_lifetime=900) as svc:
            rec["host_main_ms"] = {"A": host_main_ms(host, few, work, env),
                                   "B_service": host_main_ms(host, few, work, dict(env, **{service.ENV: svc.socket}))}
            rec["per_pass_strided_rgba_recursive"] = per_pass(svc.socket, [(1920, 1080), (3840, 2160)], 40)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
