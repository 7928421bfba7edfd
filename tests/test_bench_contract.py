"""bench.py's one-line JSON contract, checked on the newest line recorded on the MI355X
(profiles/rNN_bench.json) and on bench.py's own constants.  CPU only."""
import glob
import ast
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line():
    return json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench.json")))[-1]))


def test_required_keys_and_types():
    d = _line()
    for k, t in [("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int),
                 ("warmup", int), ("ms_per_step", (int, float)), ("higher_is_better", bool),
                 ("scaling", str), ("dtype", str), ("data", str), ("config", dict),
                 ("roofline", dict), ("cpu_baseline", dict)]:
        assert k in d and isinstance(d[k], t), k
    assert d["vs_baseline"] is None                # BASELINE.md publishes no number for this metric
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["unit"] == "MP/s" and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]


def test_value_is_consistent_with_ms_per_step():
    d = _line()
    mp = d["config"]["width"] * d["config"]["height"] / 1e6
    assert abs(d["value"] - d["n_gpus"] * mp / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3


def test_roofline_and_cpu_baseline_objects():
    d = _line()
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["peak"] == 8000.0                      # MI355X_MICROARCH.md: HBM3E 8 TB/s
    assert abs(r["achieved"] - r["algorithmic_bytes"] / (r["kernel_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-3
    assert r["traffic"] is None or r["traffic"] < r["algorithmic_bytes"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert d["quantizer_match_vs_cpu"]["identical"] is True
    assert d["cached_reference"]["bit_identical_to_pair_score"] is True


def test_workload_is_hbm_fed_and_roofline_is_stated_honestly():
    """the timed steps rotate over distinct pairs (> the 256 MiB Infinity Cache), the
    cache-resident figure is only a labelled extra, north_star's blur-pyramid target sits beside
    the W-model fraction with its verdict, and the VALU fractions carry both peaks."""
    d = _line()
    assert d["config"]["distinct_pairs_per_gpu"] >= 8 * d["config"]["streams_per_gpu"]
    assert d["config"]["input_working_set_MB"] > 268.4
    assert "cache_resident" in d and d["cache_resident"]["value"] > 0
    r = d["roofline"]
    assert r["blur_pyramid"]["target"] == 0.70 and r["blur_pyramid"]["met"] == (r["blur_pyramid_frac"] >= 0.70)
    assert abs(r["blur_pyramid_frac"] - 31.99 * 3840 * 2160 / (r["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 2e-3
    if "valu_roofline" in d:
        v = d["valu_roofline"]
        assert v["peak_nominal"] == 1.2 and abs(v["frac_nominal"] - v["achieved"] / 1.2) < 1e-3
        assert v["frac_measured"] is None or v["frac_nominal"] < v["frac_measured"]


def test_line_describes_its_process_group_and_the_search_default_mode():
    """VERDICT r04 item 1 / ADVICE r04: the line says what the collective saw (backend, world size, per rank the
    device / PCI bus id / NUMA node / cores, RCCL version) -- at N = 1 through an RCCL group of one rank -- and
    carries the throughput of the mode the search path runs by default beside `value`."""
    d = _line()
    c = d["collective"]
    assert c["backend"] == "nccl" and c["world_size"] == d["n_gpus"] == len(c["ranks"]) and c["problems"] == []
    assert c["distinct_devices"] == d["n_gpus"] and "RCCL" in c["gathered_through"]
    for k, r in enumerate(c["ranks"]):
        assert r["rank"] == k and isinstance(r["device"], int) and r["arch"].startswith("gfx950")
        assert len(r["pci_bus_id"].split(":")) == 3 and isinstance(r["numa_node"], int) and r["n_cpus"] >= 1 and r["host"]
    assert set(c["versions"]) >= {"torch", "hip", "rccl"} and c["versions"]["rccl"][0].isdigit()
    m = d["default_search_mode"]
    mp = d["config"]["width"] * d["config"]["height"] / 1e6
    assert m["blur"].startswith("recursive") and abs(m["MP_per_s"] - mp / m["ms_per_pass"] * 1e3) / m["MP_per_s"] < 1e-3
    assert m["MP_per_s"] < d["value"] and "unpinned" in m["parity"]
    assert abs(m["ms_per_pass"] - d["recursive_blur_mode"]["cached_reference"]["ms_per_pass"]) < 1e-9
    k = d["recursive_blur_mode"]["kernels"]    # per-kernel times: test_the_default_search_modes_kernel_times_are_this_runs
    assert abs(k["moved_over_strict_minimum"] - k["bytes_moved_per_pass_GB"] / k["strict_minimum_GB"]) < 0.02


def test_counters_file_is_generated_and_stamped():
    """profiles/counters.json comes from scripts/make_counters_json.py and names the kernel
    sources it was measured on; bench.py flags it stale when they differ."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    c = json.load(open(os.path.join(ROOT, "profiles", "counters.json")))
    assert "make_counters_json.py" in c["source"] and len(c["kernel_source_hash"]) == 16
    assert c["march_hbm_bytes_per_launch"] == int(c["march_fetch_KiB_reported"] * 2048 + c["march_write_KiB_reported"] * 1024)
    loaded = bench.load_counters((3840, 2160))
    assert loaded["stale"] == (c["kernel_source_hash"] != bench.kernel_source_hash())
    assert bench.load_counters((1920, 1080)) is None


def test_bench_byte_model_matches_survey():
    """85.97 B per scale-0 pixel for the whole score; the pyramid writes are
    24 * (1/4 + 1/16 + ...) of it."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    consts = {n.targets[0].id: ast.literal_eval(n.value) for n in ast.parse(src).body
              if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
              and n.targets[0].id.startswith(("ALGO_", "HBM_"))}
    assert consts["ALGO_BYTES_PER_PX_SCORE"] == 85.97
    assert consts["HBM_PEAK_GBS"] == 8000.0
    # pyramid writes at 4K: 24 B per pixel of scales 1..5
    from ssimu2_fp64 import scale_size
    px = sum(w * h for w, h in (scale_size(3840, 2160, s) for s in range(1, 6)))
    assert abs((85.97 - consts["ALGO_BYTES_PER_PX_MARCH"]) - 24 * px / (3840 * 2160)) < 0.01


def test_round3_fields_repeated_timing_and_the_recursive_modes_pass():
    """the K-step block is timed repeatedly (>= 0.2 s of timed wall, median reported,
    spread printed); no stream calibration in the bench; the recursive blur mode reports its
    per-pass cost with a cached reference, under 0.5 ms at 4K, with the pair score's bits."""
    d = _line()
    assert d["repeats"] >= 1 and d["timed_region_s"] >= 0.2
    assert d["ms_per_step_min"] <= d["ms_per_step"] <= d["ms_per_step_max"]
    assert "stream_pair_calibration" not in d and d["config"]["streams_per_gpu"] == 2
    r = d["recursive_blur_mode"]
    assert r["cached_reference"]["bit_identical_to_pair_score"] is True
    assert r["cached_reference"]["ms_per_pass"] <= 0.5 < 2 * r["ms_per_score"]
    assert r["device_memory_MB"]["reference_cache"] + r["device_memory_MB"]["per_pass_scratch"] < 1000
    assert d["roofline"]["counters"]["stale"] is False


def test_round4_fields_cpu_baseline_placement_record_and_two_context_ratio():
    """the CPU baseline carries what decides it (quota, candidate slices with their
    probe rates, the chosen slice and its busy fractions, per-repetition min / median, throttle count) and is the
    rate of the MEDIAN repetition; the stream-overlap figure is a reported number with the placed-set size."""
    d = _line()
    c = d["cpu_baseline"]
    p = c["placement"]
    assert p["cgroup_cpu_quota"] and p["affinity_cpus"] >= c["cores"]
    assert len(p["candidates"]) >= 1 and all("cpus" in k for k in p["candidates"])
    assert p["chosen"] == c["pinned_to_cpus"] and len(p["busy_fraction_of_chosen_before"]) == c["cores"]
    reps = p["ms_per_rep"]
    assert reps["n"] >= 10 and reps["min"] <= reps["median"] <= reps["max"]
    mp = d["config"]["width"] * d["config"]["height"] / 1e6
    assert abs(c["value"] - mp / reps["median"] * 1e3) / c["value"] < 2e-3
    assert c["value"] <= c["value_best_rep"]
    # the fixed slice is kept unless another one probed > 10 % faster
    rates = [k["MPps_best_of_2"] for k in p["candidates"] if "MPps_best_of_2" in k]
    assert p["chosen_is_fixed_slice"] == (max(rates) <= 1.10 * rates[0])
    t = d["two_context_ratio"]
    assert 0.5 < t["value"] < 1.0 and t["placed_streams"] >= 2
    assert abs(t["value"] - t["ms_per_score_two_contexts"] / t["ms_per_score_one_context"]) < 2e-3


def test_cpu_baseline_keeps_the_fixed_slice_unless_another_is_clearly_faster(monkeypatch):
    """bench.measure_cpu_baseline with the child processes scripted: candidate slices are probed in order, the
    rank's fixed slice is kept unless another one is > 10 % faster, the full sample runs on the chosen slice and
    `value` is the median repetition."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from oavif_amd import hostinfo
    monkeypatch.setattr(hostinfo, "cgroup_cpu_quota", lambda: 4.0)
    monkeypatch.setattr(hostinfo, "allowed_cpus", lambda: list(range(16)))
    monkeypatch.setattr(hostinfo, "candidate_core_sets", lambda n, max_sets=3: [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]])
    monkeypatch.setattr(hostinfo, "busy_fractions", lambda cpus, s=1.0, **k: {c: 0.0 for c in cpus})
    monkeypatch.setattr(bench, "usable_cores", lambda: 4)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    calls = []

    def fake_child(rates):
        def run(cpus, threads, w, h, seconds, maxreps):
            calls.append((tuple(cpus), seconds))
            ms = 1000.0 * 8.2944 / rates[tuple(cpus)]
            reps = [ms] * 2 if seconds == 0.0 else [ms * f for f in (1.0, 1.3, 0.9, 1.1, 1.0)]
            return {"threads": threads, "ms": reps, "score": 60.0, "pin_error": "", "build": "fake", "single_thread_MPps": 3.0}
        return run
    # a second slice 8 % faster: the fixed slice stays
    monkeypatch.setattr(bench, "run_cpu_child", fake_child({(0, 1, 2, 3): 50.0, (4, 5, 6, 7): 54.0, (8, 9, 10, 11): 40.0}))
    cb = bench.measure_cpu_baseline(3840, 2160, 8.2944)
    assert cb["pinned_to_cpus"] == "0-3" and cb["placement"]["chosen_is_fixed_slice"] and calls[-1] == ((0, 1, 2, 3), 12.0)
    assert abs(cb["value"] - 50.0) < 0.01 and cb["cores"] == 4 and abs(cb["value_best_rep"] - 50.0 / 0.9) < 0.01
    # the fixed slice shared with another tenant (20 MP/s): the clearly faster slice is taken, and said so
    calls.clear()
    monkeypatch.setattr(bench, "run_cpu_child", fake_child({(0, 1, 2, 3): 20.0, (4, 5, 6, 7): 54.0, (8, 9, 10, 11): 40.0}))
    cb = bench.measure_cpu_baseline(3840, 2160, 8.2944)
    assert cb["pinned_to_cpus"] == "4-7" and not cb["placement"]["chosen_is_fixed_slice"] and calls[-1] == ((4, 5, 6, 7), 12.0)
    assert [k["cpus"] for k in cb["placement"]["candidates"]] == ["0-3", "4-7", "8-11"]


def test_recursive_pass_kernels_carry_their_rooflines():
    """`recursive_blur_mode.kernels`: the launches of the search path's default pass with algorithmic bytes, LIVE durations
    handed in by the caller (ssimu2_time_kernels), the fraction of HBM peak, the committed rocprofv3 averages beside them
    as the cross-check -- and the sum of the kernels is the pass (the live whole-pass time beside it)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    w, h = 3840, 2160
    n_pad = sum((((w + (1 << k) - 1) >> k) + 127) // 128 * 128 * ((h + (1 << k) - 1) >> k) for k in range(6))
    assert bench.recursive_pass_bytes(w, h)[0] == n_pad
    assert bench.recursive_pass_bytes(20, 12)[0] == 128 * 12 + 128 * 6      # 20x12 has two scales (the size test precedes the downsample)
    live = {"convert": 0.0351, "h": 0.1541, "v": 0.1609, "finalize": 0.0057}
    rk = bench.recursive_kernel_rooflines(w, h, 0.3598, live, 0.3775, 0.3614)
    assert "ssimu2_time_kernels" in rk["source"] and rk["peak_GBps"] == 8000.0
    ks = {k["kernel"]: k for k in rk["kernels"]}
    assert set(ks) == {"k_pyramid_bands_xyb", "k_rg_h<false, false>", "k_rg_v<false>", "k_finalize"}
    plane = n_pad * 4
    assert ks["k_rg_v<false>"]["algorithmic_bytes"] == 21 * plane and ks["k_rg_h<false, false>"]["algorithmic_bytes"] == 15 * plane
    for name, k in ks.items():
        assert k["ms_measured_by_this_run"] is True
        if name == "k_finalize":
            continue
        assert abs(k["achieved_GBps"] / (k["algorithmic_bytes"] / k["ms"] / 1e6) - 1.0) < 5e-3      # `ms` is rounded to 0.1 us
        assert 0.3 < k["frac_of_hbm_peak"] < 1.0 and abs(k["frac_of_hbm_peak"] - k["achieved_GBps"] / 8000.0) < 1e-3
        assert k["ms_rocprofv3_committed"] > 0          # the newest committed profiles/rNN_rg_kernel_stats.csv, beside the live time
    assert abs(rk["sum_of_kernels_ms"] - sum(live.values())) < 1e-3 and abs(rk["between_launches_ms"] - (0.3614 - sum(live.values()))) < 1e-3
    assert rk["rocprofv3_cross_check"]["source"].startswith("profiles/r")
    other = bench.recursive_kernel_rooflines(1920, 1080, 0.155, {"convert": 0.017, "h": 0.055, "v": 0.077, "finalize": 0.005}, 0.16, 0.155)
    assert "rocprofv3_cross_check" not in other           # the committed CSV is a 4K record
    line = _line()
    rec = line["recursive_blur_mode"]
    assert abs(rec["kernels"]["sum_of_kernels_ms"] - rec["cached_reference"]["ms_per_pass"]) < 0.012


def test_the_named_resolutions_are_on_the_driver_run_line():
    """VERDICT r05 item 2 (north_star: "throughput ... at the named resolutions"; SURVEY 8d: 512x512, 1920x1080, 3840x2160,
    7680x4320): every size with FIR pair MP/s on two contexts, its W-model fraction, the one-stream figure, the recursive
    cached pass, and each kernel's own duration beside the stream time of a score."""
    d = _line()
    br = d["by_resolution"]
    sizes = {(r["width"], r["height"]): r for r in br["sizes"]}
    assert set(sizes) == {(512, 512), (1920, 1080), (3840, 2160), (7680, 4320)}
    assert br["seconds"] < 10 and "fssimu2 parity unpinned" in br["note"]
    for (w, h), r in sizes.items():
        mp = w * h / 1e6
        assert r["input_working_set_MB"] > 268.4                      # HBM-fed at every size, not Infinity-Cache-fed
        for key in ("fir_pair_two_contexts", "fir_pair_one_stream"):
            e = r[key]
            assert abs(e["MP_per_s"] - mp / e["ms_per_score"] * 1e3) / e["MP_per_s"] < 2e-3
            assert abs(e["w_model_frac"] - 85.97 * w * h / (e["ms_per_score"] * 1e-3) / 1e9 / 8000.0) < 2e-3
        assert r["fir_pair_two_contexts"]["MP_per_s"] >= 0.95 * r["fir_pair_one_stream"]["MP_per_s"]
        p = r["recursive_cached_pass_one_stream"]
        assert abs(p["MP_per_s"] - mp / p["ms_per_pass"] * 1e3) / p["MP_per_s"] < 2e-3
        for key, names in (("fir_kernels_ms", ("pyramid", "march", "finalize")), ("recursive_kernels_ms", ("convert", "h", "v", "finalize"))):
            k = r[key]
            assert abs(k["sum"] - sum(k[n] for n in names)) < 1e-4
            wall = k.get("stream_ms_per_score", k.get("stream_ms_per_pass"))
            assert 0.85 * wall <= k["sum"] <= 1.03 * wall, (w, h, key, k)   # the kernels ARE the stream time: no gaps worth a graph
    # the 4K entry is the workload of `value`, measured a second time: same rate within box noise
    assert abs(sizes[(3840, 2160)]["fir_pair_two_contexts"]["MP_per_s"] - d["value"]) / d["value"] < 0.06
    # small frames are slower per pixel, monotonically
    rates = [sizes[k]["fir_pair_two_contexts"]["MP_per_s"] for k in ((512, 512), (1920, 1080), (3840, 2160))]
    assert rates[0] < rates[1] < rates[2]


def test_the_default_search_modes_kernel_times_are_this_runs():
    """the per-kernel times of the recursive cached pass are measured by the run that prints them
    (dispatch-packet timestamps of the instrumented build), their sum within 3 % of the live pass time of the product library,
    the committed rocprofv3 averages beside them as the cross-check."""
    k = _line()["recursive_blur_mode"]["kernels"]
    assert "ssimu2_time_kernels" in k["source"]
    names = [x["kernel"] for x in k["kernels"]]
    assert names == ["k_pyramid_bands_xyb", "k_rg_h<false, false>", "k_rg_v<false>", "k_finalize"]
    assert all(x["ms_measured_by_this_run"] is True and x["ms"] > 0 for x in k["kernels"])
    assert abs(k["sum_of_kernels_ms"] - sum(x["ms"] for x in k["kernels"])) < 1e-3
    assert abs(k["live_ms_per_pass"] / k["sum_of_kernels_ms"] - 1.0) < 0.03
    assert abs(k["live_over_sum_of_kernels"] - k["live_ms_per_pass"] / k["sum_of_kernels_ms"]) < 2e-3
    for x in k["kernels"][:3]:
        assert abs(x["achieved_GBps"] - x["algorithmic_bytes"] / x["ms"] / 1e6) / x["achieved_GBps"] < 2e-3
        if "ms_rocprofv3_committed" in x:      # another box, another day: box spread
            assert abs(x["ms_rocprofv3_committed"] / x["ms"] - 1.0) < 0.10
    assert k["rocprofv3_cross_check"]["source"].startswith("profiles/r")


def test_the_collective_record_carries_each_ranks_runtime_environment():
    """what every rank ran under is on the line; bench.py itself sets none of it."""
    c = _line()["collective"]
    for r in c["ranks"]:
        assert isinstance(r["env"], dict) and all(k.startswith(("HSA_", "HIP_", "ROCR_", "NCCL_", "RCCL_", "TORCH_NCCL_", "CUDA_VISIBLE", "GPU_DEVICE")) for k in r["env"])
    src = open(os.path.join(ROOT, "bench.py")).read() + open(os.path.join(ROOT, "oavif_amd", "batch.py")).read() + \
        open(os.path.join(ROOT, "oavif_amd", "launch.py")).read()
    assert 'environ.setdefault("HSA_' not in src and 'environ["HSA_' not in src


def test_stdout_carries_the_json_line_and_nothing_else(tmp_path):
    """The contract is ONE JSON line on stdout.  RCCL prints its banner on descriptor 1 (the GPU box exports
    NCCL_DEBUG=VERSION) and children inherit it: after bench.claim_stdout() everybody else's descriptor 1 is stderr and only
    `emit` reaches what stdout was."""
    import subprocess
    import sys
    prog = ("import os, sys, json; sys.path.insert(0, %r); import bench\n"
            "print('before the claim', flush=True)\n"
            "emit = bench.claim_stdout()\n"
            "print('python noise')\n"
            "os.write(1, b'C library noise\\n')\n"
            "os.system('echo child noise')\n"
            "emit({'metric': 'm', 'value': 1.5})\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout == 'before the claim\n{"metric": "m", "value": 1.5}\n'
    for noise in ("python noise", "C library noise", "child noise"):
        assert noise in r.stderr
    assert "torch" not in r.stderr   # importing bench.py pulls in neither torch nor a GPU
