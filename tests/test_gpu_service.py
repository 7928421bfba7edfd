"""The resident scoring service on the GPU: a real oavif_scored is a child of the test, and
remote contexts (OAVIF_SCORER_SOCKET set around ssimu2_ctx_create) and in-process contexts are made side by side from
this process -- the variable is read per ssimu2_ctx_create.  What a remote context returns carries the bits of the
in-process call: doubles and floats travel as their bytes.

Every server is started with --max-lifetime, every child runs under a time limit, one server runs at a time, and at
most two client children at once.  Nothing here ends a process that holds the GPU in the middle of a call."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oavif_amd import _lib, service

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 20), (121, 41), (333, 217), (1921, 1083)]
MODES = [_lib.BLUR_FIR, _lib.BLUR_RECURSIVE, _lib.BLUR_RECURSIVE_FMA]
LIFETIME = 600       # seconds: no server of this module outlives it by more


class _Servers:
    """One service at a time; a test that needs another --max-contexts gets a new one after the old one has left."""

    def __init__(self):
        self.svc, self.max_contexts = None, None

    def get(self, max_contexts=None):
        if self.svc is None or self.max_contexts != max_contexts or self.svc.proc.poll() is not None:
            self.stop()
            self.svc, self.max_contexts = service.start(max_lifetime=LIFETIME, max_contexts=max_contexts), max_contexts
        return self.svc

    def stop(self):
        if self.svc is not None:
            rc = self.svc.stop(timeout=30)
            self.svc = None
            assert rc == 0, rc


@pytest.fixture(scope="module")
def servers(hip_lib):
    s = _Servers()
    yield s
    s.stop()


def _frames(w, h, seed):
    from tests import service_child
    return service_child.frames(w, h, seed)


def _bits(x):
    return np.asarray(x).tobytes()


def _padded_rgba(rgb, pad):
    h, w, _ = rgb.shape
    row = w * 4 * rgb.dtype.itemsize + pad
    buf = np.full((h, row), 0x5A, np.uint8)
    px = np.zeros((h, w, 4), rgb.dtype)
    px[..., :3] = rgb
    px[..., 3] = 200
    buf[:, : w * 4 * rgb.dtype.itemsize] = px.reshape(h, -1).view(np.uint8)
    return buf, row


def _walk(s, a, b, mode):
    """pair, cached reference, strided RGBA with padding, a 10-bit decode against the 8-bit reference, a 16-bit pair, the
    maps; every score with its 108 averages.  Returns [(name, bytes)]."""
    out = []

    def rec(name, *vals):
        avg, ns = s.last_averages()
        out.append((name, b"".join(_bits(v) for v in vals) + _bits(avg) + bytes([ns])))

    h, w, _ = a.shape
    s.set_blur(mode)
    rec("pair", s.compute_ssimu2(a, b))
    s.set_reference(a)
    rec("cached", s.score_against_reference(b))
    buf, row = _padded_rgba(b, 12)
    rec("strided rgba", s.score_decoded_against_reference(buf.reshape(-1), row, 4))
    pinned = s.host_alloc(buf.shape)                  # the C host's path: the frame decoded into the scorer's own memory
    pinned[:] = buf
    rec("strided rgba, host_alloc", s.score_decoded_against_reference(pinned.reshape(-1), row, 4))
    s.host_free(pinned)
    b10 = ((b.astype(np.uint16) * 1023 + 127) // 255).astype(np.uint16)
    rec("10-bit decode, 8-bit reference", s.score_against_reference_hbd(b10, 10))
    buf16, row16 = _padded_rgba(b10, 10)
    rec("10-bit strided rgba", s.score_decoded_against_reference_hbd(buf16.reshape(-1).view(np.uint16), row16, 4, 10))
    score, fmap = s.error_map_against_reference(b)
    rec("map, cached", score, fmap)
    a16 = a.astype(np.uint16) * 257 + 3
    b16 = b.astype(np.uint16) * 257 + 1
    rec("16-bit pair", s.compute_ssimu2_hbd(a16, b16, 16))
    s.set_reference_hbd(a16, 16)
    rec("16-bit cached", s.score_against_reference_hbd(b16, 16))
    score, fmap = s.error_map(a, b)
    rec("map, pair", score, fmap)
    return out


@pytest.fixture(scope="module")
def local(hip_lib):
    from oavif_amd import Ssimu2
    s = Ssimu2(0)
    yield s
    s.close()


@pytest.mark.parametrize("mode", MODES, ids=["fir", "recursive", "recursive_fma"])
@pytest.mark.parametrize("w,h", SIZES)
def test_remote_results_carry_the_bits_of_the_in_process_call(servers, local, w, h, mode):
    from oavif_amd import Ssimu2
    a, b = _frames(w, h, w + h)
    with Ssimu2(0, service=servers.get().socket) as remote:
        # the server's record of the same device; the marketing name is whatever HIP runtime a process loaded makes of
        # it (this process loads torch's, the server ROCm's), everything else is the device's
        theirs, ours = remote.device_info(), local.device_info()
        assert {k: v for k, v in theirs.items() if k != "name"} == {k: v for k, v in ours.items() if k != "name"}
        got = _walk(remote, a, b, mode)
    want = _walk(local, a, b, mode)
    assert [g[0] for g in got] == [x[0] for x in want]
    for g, x in zip(got, want):
        assert g[1] == x[1], g[0]


@pytest.mark.parametrize("n", [1, 7, 33])
def test_remote_batches_carry_the_bits_of_every_item(servers, local, n):
    from oavif_amd import Ssimu2
    w, h = 121, 41
    pairs = [_frames(w, h, 900 + i) for i in range(n)]
    refs, dists = [p[0] for p in pairs], [p[1] for p in pairs]

    def walk(s):
        s.set_blur(_lib.BLUR_FIR)
        out = [_bits(s.score_batch(refs, dists))]
        out += [_bits(s.last_batch_averages(i)[0]) + bytes([s.last_batch_averages(i)[1]]) for i in range(n)]
        s.set_reference(refs[0])
        out.append(_bits(s.score_batch_against_reference(dists)))
        out += [_bits(s.last_batch_averages(i)[0]) for i in range(n)]
        out.append(_bits(s.score_against_reference(dists[0])))           # the reference stayed cached
        return out

    with Ssimu2(0, service=servers.get().socket) as remote:
        got = walk(remote)
    assert got == walk(local)


def _child(sock, w, h, seed):
    env = dict(os.environ, OAVIF_SCORER_SOCKET=sock, OAVIF_AMD_NO_TORCH="1")
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "service_child.py"), str(w), str(h), str(seed)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def _expected(local, w, h, seed):
    a, b = _frames(w, h, seed)
    local.set_blur(_lib.BLUR_FIR)
    pair = local.compute_ssimu2(a, b)
    avg, ns = local.last_averages()
    local.set_reference(a)
    return {"pair": float(pair).hex(), "cached": float(local.score_against_reference(b)).hex(), "scales": int(ns),
            "averages": np.asarray(avg, np.float64).tobytes().hex()}


def _finish(p):
    out, err = p.communicate(timeout=120)
    assert p.returncode == 0, err[-2000:]
    return json.loads(out.strip().splitlines()[-1])


def test_a_client_process_of_the_service_never_opens_the_gpu(servers, local):
    got = _finish(_child(servers.get().socket, 333, 217, 5))
    assert got["arch"].startswith("gfx950")
    gpu_files = [f for f in got["fds"] if f == "/dev/kfd" or re.match(r"/dev/dri/renderD\d+", f)]
    assert not gpu_files, got["fds"]
    assert any("oavif_scorer_frames" in f for f in got["fds"])          # the shared frame memory, and a socket
    want = _expected(local, 333, 217, 5)
    assert {k: got[k] for k in want} == want


def test_two_client_processes_at_once_each_get_their_own_bits(servers, local):
    sock = servers.get().socket
    jobs = [(333, 217, 21), (640, 360, 22)]
    procs = [_child(sock, *j) for j in jobs]
    results = [_finish(p) for p in procs]
    for j, got in zip(jobs, results):
        want = _expected(local, *j)
        assert {k: got[k] for k in want} == want, j
    assert results[0]["pair"] != results[1]["pair"]


def test_a_pooled_context_serves_the_next_connection_like_a_fresh_one(servers, hip_lib):
    """--max-contexts 1: the second connection gets the context the first one used (333x217 in RECURSIVE, a reference set)
    and serves 121x41 in FIR with the bits of a fresh in-process context."""
    import time
    from oavif_amd import Ssimu2, Ssimu2Error
    sock = servers.get(max_contexts=1).socket
    big, small = _frames(333, 217, 31), _frames(121, 41, 32)
    with Ssimu2(0, service=sock, blur=_lib.BLUR_RECURSIVE) as first:
        first.set_reference(big[0])
        first.score_against_reference(big[1])
        first.compute_ssimu2_hbd(big[0].astype(np.uint16) * 257, big[1].astype(np.uint16) * 257, 16)
        first.set_reference(big[0])
    deadline = time.monotonic() + 20
    while True:                                      # the server sees the close a moment later; until then: SSIMU2_ERR_OOM
        try:
            second = Ssimu2(0, service=sock)
            break
        except Ssimu2Error as e:
            assert e.code == _lib.ERR_OOM and "--max-contexts" in str(e) and time.monotonic() < deadline
            time.sleep(0.01)
    with second:
        with pytest.raises(Ssimu2Error) as ei:
            second.score_against_reference(small[1])
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        got = _walk(second, small[0], small[1], _lib.BLUR_FIR)
        got.append(("batch", _bits(second.score_batch([small[0]], [small[1]]))))     # FIR: batches run
    with Ssimu2(0) as fresh:
        want = _walk(fresh, small[0], small[1], _lib.BLUR_FIR)
        want.append(("batch", _bits(fresh.score_batch([small[0]], [small[1]]))))
    assert got == want


def test_the_c_host_through_the_service_equals_the_host_in_process(servers, tmp_path):
    from oavif_amd import avif_bridge as ab
    from oavif_amd import build as obuild
    from oavif_amd import synth
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    from PIL import Image
    if obuild.host_needs_build():
        obuild.build_host()
    png = tmp_path / "a.png"
    Image.fromarray(synth.make_ref(320, 240, 303)).save(png)
    args = ["--score-tgt", "75", "--tolerance", "1.5", "--tenbit", "0"]
    env = dict(os.environ, OAVIF_LIBAVIF=ab._find_library())
    env.pop("OAVIF_SCORER_SOCKET", None)
    res = {}
    for name, extra in (("in process", {}), ("service", {"OAVIF_SCORER_SOCKET": servers.get().socket})):
        out = tmp_path / "o.avif"
        r = subprocess.run([obuild.HOST_PATH, *args, str(png), str(out)], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert r.returncode == 0, (name, r.stderr[-1500:])
        found = [l for l in r.stderr.splitlines() if l.startswith("Found q")]
        assert len(found) == 1 and re.fullmatch(r"Found q(\d+) \(score (-?\d+\.\d{2}), (\d+) passes\)", found[0]), r.stderr
        res[name] = (found[0], out.read_bytes())
    assert res["service"] == res["in process"], (res["service"][0], res["in process"][0])
