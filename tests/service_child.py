"""A per-image client process of the scoring service, for tests/test_gpu_service.py: with OAVIF_SCORER_SOCKET in its
environment it scores one seeded pair (pair score, cached reference, averages) like any user of the library, and prints
one JSON line: the bits it got, and every file this process holds open -- a client of the service never opens the GPU.

    python tests/service_child.py W H SEED
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def frames(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = (a // 4 + np.linspace(0, 190, w, dtype=np.uint8)[None, :, None]).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    return a, b


def main():
    w, h, seed = (int(x) for x in sys.argv[1:4])
    from oavif_amd import Ssimu2
    a, b = frames(w, h, seed)
    with Ssimu2(0) as s:
        pair = s.compute_ssimu2(a, b)
        avg, ns = s.last_averages()
        s.set_reference(a)
        cached = s.score_against_reference(b)
        arch = s.device_info()["arch"]
        fds = []
        for name in os.listdir("/proc/self/fd"):
            try:
                fds.append(os.readlink(f"/proc/self/fd/{name}"))
            except OSError:
                pass
    print(json.dumps({"pair": float(pair).hex(), "cached": float(cached).hex(), "scales": int(ns),
                      "averages": np.asarray(avg, np.float64).tobytes().hex(), "arch": arch, "fds": fds}))


if __name__ == "__main__":
    main()
