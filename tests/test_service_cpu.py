"""The resident scoring service on a machine without a GPU.

Server: oavif_amd/csrc/oavif_scored.cpp built over tests/c/stub_scorer_full.c, a deterministic stand-in for the whole
of include/ssimu2_hip.h whose scores, averages and map numpy restates exactly.  Client: the real liboavif_hip.so with
OAVIF_SCORER_SOCKET set -- it loads without a GPU and, for a remote context, never starts HIP.  The same stand-in
linked directly (a shared object loaded next to the product library) is what every remote answer is held to."""
import contextlib
import ctypes
import fcntl
import os
import re
import signal
import socket
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from oavif_amd import _lib
from oavif_amd import build as obuild
from oavif_amd import service

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "oavif_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "c", "stub_scorer_full.c")
ENV = "OAVIF_SCORER_SOCKET"
SIZES = [(1, 1), (7, 9), (64, 20), (121, 41), (333, 217), (1921, 1083)]   # the last: larger than any socket buffer

# the wire structs of oavif_amd/csrc/remote_client.h
MAGIC, PROTO, NULL = 0x53324356, 1, (1 << 64) - 1
HELLO = struct.Struct("<IIIIQ512s")
HELLO_REPLY = struct.Struct("<Ii264s512s")
REQUEST = struct.Struct("<II4IIIQ6Q")

pytestmark = pytest.mark.skipif(not hasattr(os, "memfd_create"), reason="no memfd_create")


@contextlib.contextmanager
def _environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _sock(tmp_path, name):
    """A socket path under tmp_path, or -- where that is too long for sockaddr_un (108 bytes) -- in a short directory."""
    path = os.path.join(str(tmp_path), name)
    if len(path.encode()) < 100:
        return path
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="oavif_t_")
    atexit.register(shutil.rmtree, d, True)
    return os.path.join(d, name)


class Kit:
    pass


@pytest.fixture(scope="module")
def kit(hip_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("service")
    k = Kit()
    k.dir = d
    k.server = obuild.build_service(scorer=[STUB], out=str(d / "oavif_scored_stub"))
    direct = str(d / "libstub_direct.so")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", INC, STUB, "-o", direct, "-lm"], check=True)
    k.direct = _lib._load(direct)            # the stand-in, linked directly: what the service's answers are held to
    k.lib = hip_lib                          # the product library: the client
    k.version = hip_lib.ssimu2_version().decode()
    return k


def _start(kit, version=None, **kw):
    """A stub service whose ssimu2_version() is the product library's (or `version`)."""
    kw.setdefault("max_lifetime", 120)
    with _environ(STUB_SCORER_VERSION=version or kit.version):
        return service.start(program=kit.server, **kw)


@pytest.fixture(scope="module")
def svc(kit):
    s = _start(kit, socket=_sock(kit.dir, "shared.sock"))
    yield s
    assert s.stop() == 0


class Api:
    """One context of library L (remote: created with OAVIF_SCORER_SOCKET = `sock`), called through raw ctypes."""

    def __init__(self, L, sock=None, expect=0):
        self.L, self.ctx, self.keep = L, ctypes.c_void_p(), []
        with _environ(**{ENV: sock}):
            self.rc = L.ssimu2_ctx_create(0, None, ctypes.byref(self.ctx))
        assert self.rc == expect, (self.rc, L.ssimu2_last_error(None))

    def close(self):
        if self.ctx.value:
            self.L.ssimu2_ctx_destroy(self.ctx)
        self.ctx = ctypes.c_void_p()

    def err(self):
        return self.L.ssimu2_last_error(self.ctx).decode()

    def alloc(self, nbytes):
        """nbytes of ssimu2_host_alloc memory as a uint8 array."""
        p = ctypes.c_void_p()
        assert self.L.ssimu2_host_alloc(self.ctx, nbytes, ctypes.byref(p)) == 0 and p.value
        return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value)), p

    def put(self, a, pinned):
        """`a` as it is, or copied into ssimu2_host_alloc memory."""
        if not pinned:
            return a
        buf, p = self.alloc(a.nbytes)
        buf[:] = a.reshape(-1).view(np.uint8)
        self.keep.append(p)
        return buf.view(a.dtype).reshape(a.shape)

    def free_all(self):
        for p in self.keep:
            assert self.L.ssimu2_host_free(self.ctx, p) == 0
        self.keep = []


def _p8(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _p16(a):
    return None if a is None else ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_uint16))


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _padded(rgb, channels, pad):
    """(h, w, 3) -> rows of w * channels samples + `pad` bytes of padding, alpha and padding filled with noise."""
    h, w, _ = rgb.shape
    item = rgb.dtype.itemsize
    row = w * channels * item + pad
    buf = np.random.default_rng(w * 31 + h).integers(0, 256, (h, row), dtype=np.uint8)
    px = np.zeros((h, w, channels), rgb.dtype)
    px[..., :3] = rgb
    if channels == 4:
        px[..., 3] = 77
    buf[:, : w * channels * item] = px.reshape(h, -1).view(np.uint8)
    return buf, row


def _score8(a, b):
    sad = int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())
    return 100.0 - 6.0 * float(sad) / (float(a.shape[1]) * a.shape[0] * 3)


def _s16(x, depth):
    maxv = (1 << depth) - 1
    return np.minimum(x.astype(np.int64), maxv) * 65535 // maxv


def _score16(a16, b16):
    """Both already on the 16-bit scale."""
    sad = int(np.abs(a16 - b16).sum())
    return 100.0 - 6.0 * float(sad) / (float(a16.shape[1]) * a16.shape[0] * 3) / 257.0


def _map8(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32)).astype(np.float32)
    return d[..., 0] + np.float32(0.5) * d[..., 1] + np.float32(0.25) * d[..., 2]


def _walk(api, w, h, pinned):
    """Every served single-frame call on one context; returns [(name, rc, bytes of the result)]."""
    L, c, out = api.L, api.ctx, []
    a, b = _frames(w, h, w * 1000 + h)
    s, ns = ctypes.c_double(), ctypes.c_int()
    avg = np.zeros(108)
    fmap = np.zeros((h, w), np.float32)

    def rec(name, rc, *vals):
        out.append((name, rc, b"".join(np.asarray(v).tobytes() for v in vals)))

    def averages(tag):
        rc = L.ssimu2_last_averages(c, avg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(ns))
        rec("last_averages " + tag, rc, avg, ns.value)

    pa, pb = api.put(a, pinned), api.put(b, pinned)
    rec("score_rgb8", L.ssimu2_score_rgb8(c, _p8(pa), _p8(pb), w, h, 3, ctypes.byref(s)), s.value)
    averages("pair")
    rec("set_reference", L.ssimu2_set_reference(c, _p8(pa), w, h))
    rec("against", L.ssimu2_score_against_reference(c, _p8(pb), ctypes.byref(s)), s.value)
    for ch, pad in ((4, 12), (3, 5), (3, 0)):
        buf, row = _padded(b, ch, pad)
        pbuf = api.put(buf, pinned)
        rec(f"strided ch{ch} pad{pad}", L.ssimu2_score_against_reference_strided(c, _p8(pbuf), row, ch, ctypes.byref(s)), s.value)
    averages("strided")
    fp = fmap.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rec("map_against", L.ssimu2_error_map_against_reference(c, _p8(pb), fp, ctypes.byref(s)), s.value, fmap)
    rec("map_rgb8", L.ssimu2_error_map_rgb8(c, _p8(pa), _p8(pb), w, h, 3, fp, ctypes.byref(s)), s.value, fmap)
    for depth in (8, 10, 16):
        shift = 16 - depth
        a16 = ((a.astype(np.uint16) * 257) >> shift).astype(np.uint16)
        b16 = ((b.astype(np.uint16) * 257) >> shift).astype(np.uint16)
        b16[0, 0, 0] = 65535                         # above 2^d - 1 at depth < 16: clamped, not an error
        qa, qb = api.put(a16, pinned), api.put(b16, pinned)
        rec(f"score_rgb16 d{depth}", L.ssimu2_score_rgb16(c, _p16(qa), _p16(qb), w, h, 3, depth, ctypes.byref(s)), s.value)
        rec(f"set_reference_rgb16 d{depth}", L.ssimu2_set_reference_rgb16(c, _p16(qa), w, h, depth))
        rec(f"against_rgb16 d{depth}", L.ssimu2_score_against_reference_rgb16(c, _p16(qb), depth, ctypes.byref(s)), s.value)
        buf, row = _padded(b16, 4, 10)
        pbuf = api.put(buf, pinned)
        rec(f"strided16 d{depth}", L.ssimu2_score_against_reference_strided16(c, _p16(pbuf), row, 4, depth, ctypes.byref(s)), s.value)
        rec(f"against 8-bit probe of a {depth}-bit reference", L.ssimu2_score_against_reference(c, _p8(pb), ctypes.byref(s)), s.value)
    b10 = ((b.astype(np.uint16) * 257) >> 6).astype(np.uint16)
    rec("set_reference again", L.ssimu2_set_reference(c, _p8(pa), w, h))
    rec("10-bit decode against an 8-bit reference", L.ssimu2_score_against_reference_rgb16(c, _p16(api.put(b10, pinned)), 10, ctypes.byref(s)), s.value)
    averages("end")
    api.free_all()
    return out, (a, b, b10)


def _batch_walk(api, n, pinned_item):
    L, c, w, h, out = api.L, api.ctx, 64, 20, []
    pairs = [_frames(w, h, 50 + i) for i in range(n)]
    refs = [p[0] for p in pairs]
    dists = [p[1] for p in pairs]
    plain = list(dists)
    if pinned_item is not None:
        dists[pinned_item] = api.put(dists[pinned_item], True)     # one item already in the service's memory
    PA = ctypes.POINTER(ctypes.c_uint8) * n
    r_arr, d_arr = PA(*[_p8(x) for x in refs]), PA(*[_p8(x) for x in dists])
    scores, avg, ns = np.zeros(n), np.zeros(108), ctypes.c_int()
    sp = scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out.append(("batch_rgb8", L.ssimu2_score_batch_rgb8(c, r_arr, d_arr, n, w, h, sp), scores.tobytes()))
    assert L.ssimu2_set_reference(c, _p8(refs[0]), w, h) == 0
    out.append(("batch_against", L.ssimu2_score_batch_against_reference(c, d_arr, n, sp), scores.tobytes()))
    for item in (0, n - 1):
        rc = L.ssimu2_last_batch_averages(c, item, avg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(ns))
        out.append((f"last_batch_averages {item}", rc, avg.tobytes() + bytes([ns.value])))
    api.free_all()
    return out, (refs, plain)


# ---- 1. a context where there is no GPU -----------------------------------------------------------------------------
def test_a_remote_context_scores_on_a_machine_without_a_gpu(kit, svc):
    """Fails without the feature: with OAVIF_SCORER_SOCKET set, ssimu2_ctx_create of the product library succeeds here
    (unset, it returns SSIMU2_ERR_NO_DEVICE on this machine) and the score is the stand-in's formula, bit for bit."""
    api = Api(kit.lib, svc.socket)
    a, b = _frames(96, 40, 3)
    s = ctypes.c_double()
    assert kit.lib.ssimu2_score_rgb8(api.ctx, _p8(a), _p8(b), 96, 40, 3, ctypes.byref(s)) == 0, api.err()
    assert s.value == _score8(a, b) and s.value != 100.0
    info = _lib.DeviceInfo()
    assert kit.lib.ssimu2_ctx_device_info(api.ctx, ctypes.byref(info)) == 0 and info.arch == b"stub"   # the server's record
    api.close()


def test_selection_prefetch_query_and_the_local_calls(kit, svc):
    L = kit.lib
    with _environ(**{ENV: svc.socket}):
        assert L.ssimu2_prefetch(0) == 0 and L.ssimu2_prefetch_join(0) == 0       # validated, HIP not started
        assert L.ssimu2_prefetch(-1) == _lib.ERR_INVALID_ARG and L.ssimu2_prefetch_join(64) == _lib.ERR_INVALID_ARG
        info = _lib.DeviceInfo()
        assert L.ssimu2_query_device(0, ctypes.byref(info)) == 0 and info.name == b"stub scorer"
        tab = np.zeros(256, np.float32)
        assert L.ssimu2_linear_table(8, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0 and tab[255] == 1.0
        assert b"gfx950" in L.ssimu2_version()
        ctx = ctypes.c_void_p()
        assert L.ssimu2_ctx_create(0, ctypes.c_void_p(8), ctypes.byref(ctx)) == _lib.ERR_INVALID_ARG   # a hip_stream
        assert "hip_stream" in L.ssimu2_last_error(None).decode()
        assert L.ssimu2_ctx_create(0, None, None) == _lib.ERR_INVALID_ARG
    # %d in the value is the device argument
    d = os.path.dirname(svc.socket)
    link = os.path.join(d, "gpu3.sock")
    os.symlink(svc.socket, link)
    with _environ(**{ENV: os.path.join(d, "gpu%d.sock")}):
        ctx = ctypes.c_void_p()
        assert L.ssimu2_ctx_create(3, None, ctypes.byref(ctx)) == 0
        L.ssimu2_ctx_destroy(ctx)
        assert L.ssimu2_ctx_create(4, None, ctypes.byref(ctx)) == _lib.ERR_NO_DEVICE
        assert "gpu4.sock" in L.ssimu2_last_error(None).decode()
    os.unlink(link)
    with _environ(**{ENV: ""}):     # empty = unset: the local path, which finds no GPU here
        import torch
        if not torch.cuda.is_available():
            ctx = ctypes.c_void_p()
            assert L.ssimu2_ctx_create(0, None, ctypes.byref(ctx)) == _lib.ERR_NO_DEVICE


# ---- 2. every served call round-trips --------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["plain", "host_alloc"])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_single_frame_call_round_trips(kit, svc, w, h, pinned):
    remote, direct = Api(kit.lib, svc.socket), Api(kit.direct)
    got, (a, b, b10) = _walk(remote, w, h, pinned)
    want, _ = _walk(direct, w, h, pinned)
    assert [g[0] for g in got] == [x[0] for x in want]
    for g, x in zip(got, want):
        assert g[1] == x[1] == 0, (g[0], g[1], x[1], remote.err())
        assert g[2] == x[2], g[0]                    # scores, averages, maps: the bytes the server's context returned
    res = {g[0]: g[2] for g in got}
    f64 = lambda v: np.float64(v).tobytes()          # noqa: E731
    assert res["score_rgb8"] == f64(_score8(a, b)) == res["against"] == res["strided ch4 pad12"] == res["strided ch3 pad5"]
    assert res["map_rgb8"] == f64(_score8(a, b)) + _map8(a, b).tobytes() == res["map_against"]
    assert res["10-bit decode against an 8-bit reference"] == f64(_score16(a.astype(np.int64) * 257, _s16(b10, 10)))
    avg = np.frombuffer(res["last_averages pair"][:864])
    assert np.array_equal(avg, _score8(a, b) + np.arange(108)) and res["last_averages pair"][864:868] == struct.pack("<i", 1 + (w * h) % 6)
    remote.close()
    direct.close()


@pytest.mark.parametrize("n", [1, 7, 33])
def test_batches_round_trip(kit, svc, n):
    remote, direct = Api(kit.lib, svc.socket), Api(kit.direct)
    got, (refs, dists) = _batch_walk(remote, n, pinned_item=n // 2)
    want, _ = _batch_walk(direct, n, pinned_item=None)
    assert got == want and all(g[1] == 0 for g in got), remote.err()
    assert np.array_equal(np.frombuffer(got[0][2]), [_score8(r, d) for r, d in zip(refs, dists)])
    assert np.array_equal(np.frombuffer(got[1][2]), [_score8(refs[0], d) for d in dists])
    remote.close()
    direct.close()


# ---- 3. bad arguments: the answer of the same code linked directly -------------------------------------------------
def _bad_argument_cases(api):
    L, c = api.L, api.ctx
    w, h = 24, 10
    a, b = _frames(w, h, 9)
    a16, b16 = a.astype(np.uint16) * 257, b.astype(np.uint16) * 257
    odd = np.zeros(w * h * 6 + 2, np.uint8)[1:]                 # an odd address
    s = ctypes.c_double()
    S = ctypes.byref(s)
    fmap = np.zeros((h, w), np.float32)
    FP = fmap.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    avg = np.zeros(108)
    AP = avg.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    scores = np.zeros(8)
    SP = scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    PA = ctypes.POINTER(ctypes.c_uint8) * 3
    items, holed = PA(_p8(b), _p8(a), _p8(b)), PA(_p8(b), None, _p8(b))
    p = ctypes.c_void_p()
    r = []
    add = lambda name, rc: r.append((name, rc, api.err()))      # noqa: E731
    add("nothing yet", 0)
    add("score_rgb16 zero size, odd address, first call", L.ssimu2_score_rgb16(c, _p16(odd), _p16(odd), 0, 0, 3, 16, S))
    add("set_blur 7", L.ssimu2_ctx_set_blur(c, 7))
    add("score_rgb8 null ref", L.ssimu2_score_rgb8(c, None, _p8(b), w, h, 3, S))
    add("score_rgb8 null dist", L.ssimu2_score_rgb8(c, _p8(a), None, w, h, 3, S))
    add("score_rgb8 w 0", L.ssimu2_score_rgb8(c, _p8(a), _p8(b), 0, h, 3, S))
    add("score_rgb8 h 0", L.ssimu2_score_rgb8(c, _p8(a), _p8(b), w, 0, 3, S))
    add("score_rgb8 channels 4", L.ssimu2_score_rgb8(c, _p8(a), _p8(b), w, h, 4, S))
    add("score_rgb8 null out", L.ssimu2_score_rgb8(c, _p8(a), _p8(b), w, h, 3, None))
    add("score_rgb8 above 2^31/3 pixels", L.ssimu2_score_rgb8(c, _p8(a), _p8(b), 65536, 65536, 3, S))   # nothing is read
    add("set_reference null", L.ssimu2_set_reference(c, None, w, h))
    add("set_reference zero", L.ssimu2_set_reference(c, _p8(a), 0, 0))
    add("against, no reference", L.ssimu2_score_against_reference(c, _p8(b), S))
    add("strided, no reference", L.ssimu2_score_against_reference_strided(c, _p8(b), w * 3, 3, S))
    add("against_rgb16, no reference", L.ssimu2_score_against_reference_rgb16(c, _p16(b16), 16, S))
    add("strided16, no reference", L.ssimu2_score_against_reference_strided16(c, _p16(b16), w * 6, 3, 16, S))
    add("map_against, no reference", L.ssimu2_error_map_against_reference(c, _p8(b), FP, S))
    add("batch_against, no reference", L.ssimu2_score_batch_against_reference(c, items, 3, SP))
    add("set_reference", L.ssimu2_set_reference(c, _p8(a), w, h))
    add("against null dist", L.ssimu2_score_against_reference(c, None, S))
    add("against null out", L.ssimu2_score_against_reference(c, _p8(b), None))
    add("strided channels 5", L.ssimu2_score_against_reference_strided(c, _p8(b), w * 5, 5, S))
    add("strided short rows", L.ssimu2_score_against_reference_strided(c, _p8(b), w * 3 - 1, 3, S))
    add("strided null", L.ssimu2_score_against_reference_strided(c, None, w * 3, 3, S))
    add("against_rgb16 odd address", L.ssimu2_score_against_reference_rgb16(c, _p16(odd), 16, S))
    add("against_rgb16 depth 7", L.ssimu2_score_against_reference_rgb16(c, _p16(b16), 7, S))
    add("against_rgb16 depth 17", L.ssimu2_score_against_reference_rgb16(c, _p16(b16), 17, S))
    add("against_rgb16 null", L.ssimu2_score_against_reference_rgb16(c, None, 16, S))
    add("strided16 odd row_bytes", L.ssimu2_score_against_reference_strided16(c, _p16(b16), w * 6 + 1, 3, 16, S))
    add("strided16 short rows", L.ssimu2_score_against_reference_strided16(c, _p16(b16), w * 6 - 2, 3, 16, S))
    add("strided16 channels 2", L.ssimu2_score_against_reference_strided16(c, _p16(b16), w * 6, 2, 16, S))
    add("score_rgb16 odd ref", L.ssimu2_score_rgb16(c, _p16(odd), _p16(b16), w, h, 3, 16, S))
    add("score_rgb16 channels 4", L.ssimu2_score_rgb16(c, _p16(a16), _p16(b16), w, h, 4, 16, S))
    add("score_rgb16 depth 20", L.ssimu2_score_rgb16(c, _p16(a16), _p16(b16), w, h, 3, 20, S))
    add("set_reference_rgb16 depth 0", L.ssimu2_set_reference_rgb16(c, _p16(a16), w, h, 0))
    add("map_against null map", L.ssimu2_error_map_against_reference(c, _p8(b), None, S))
    add("map_rgb8 null map", L.ssimu2_error_map_rgb8(c, _p8(a), _p8(b), w, h, 3, None, S))
    add("map_rgb8 null score", L.ssimu2_error_map_rgb8(c, _p8(a), _p8(b), w, h, 3, FP, None))
    add("last_averages null", L.ssimu2_last_averages(c, None, None))
    add("last_averages, no scale count", L.ssimu2_last_averages(c, AP, None))
    add("reference survived all of that", L.ssimu2_score_against_reference(c, _p8(b), S))
    add("batch n 0", L.ssimu2_score_batch_rgb8(c, None, None, 0, 0, 0, None))
    add("batch n above SSIMU2_MAX_BATCH", L.ssimu2_score_batch_rgb8(c, items, items, 5000, w, h, SP))
    add("batch null refs", L.ssimu2_score_batch_rgb8(c, None, items, 3, w, h, SP))
    add("batch null item", L.ssimu2_score_batch_rgb8(c, items, holed, 3, w, h, SP))
    add("batch null out", L.ssimu2_score_batch_rgb8(c, items, items, 3, w, h, None))
    add("batch zero size", L.ssimu2_score_batch_rgb8(c, items, items, 3, 0, h, SP))
    add("batch_against null item", L.ssimu2_score_batch_against_reference(c, holed, 3, SP))
    add("batch_against null array", L.ssimu2_score_batch_against_reference(c, None, 3, SP))
    add("last_batch_averages before a batch", L.ssimu2_last_batch_averages(c, 0, AP, None))
    add("batch_against", L.ssimu2_score_batch_against_reference(c, items, 3, SP))
    add("last_batch_averages item 3 of 3", L.ssimu2_last_batch_averages(c, 3, AP, None))
    add("last_batch_averages null", L.ssimu2_last_batch_averages(c, 0, None, None))
    add("set_blur recursive", L.ssimu2_ctx_set_blur(c, _lib.BLUR_RECURSIVE))
    add("batch in a recursive mode", L.ssimu2_score_batch_rgb8(c, items, items, 3, w, h, SP))
    add("against after the blur switch", L.ssimu2_score_against_reference(c, _p8(b), S))
    add("set_reference_rgb16", L.ssimu2_set_reference_rgb16(c, _p16(a16), w, h, 16))
    add("map against a 16-bit reference", L.ssimu2_error_map_against_reference(c, _p8(b), FP, S))
    add("host_alloc zero bytes", L.ssimu2_host_alloc(c, 0, ctypes.byref(p)))
    add("host_alloc null out", L.ssimu2_host_alloc(c, 64, None))
    add("host_free null", L.ssimu2_host_free(c, None))
    return r


def test_bad_arguments_are_answered_as_by_the_scorer_linked_directly(kit, svc):
    remote, direct = Api(kit.lib, svc.socket), Api(kit.direct)
    got, want = _bad_argument_cases(remote), _bad_argument_cases(direct)
    for g, x in zip(got, want):
        assert g[:2] == x[:2], (g, x)                            # the code
        if not g[0].startswith("host_"):                         # and the library's own words (host memory is the client's)
            assert g[2] == x[2], (g, x)
    assert len(got) == len(want) and got[0][2] == "" and got[1][2] == "zero image dimension"
    codes = {g[0]: g[1] for g in got}
    # and the header's contract, where the stand-in follows it
    E = _lib
    for name, code in (("score_rgb8 channels 4", E.ERR_UNSUPPORTED), ("score_rgb8 above 2^31/3 pixels", E.ERR_INVALID_ARG),
                       ("against_rgb16, no reference", E.ERR_NO_REFERENCE), ("against_rgb16 odd address", E.ERR_INVALID_ARG),
                       ("against_rgb16 depth 17", E.ERR_UNSUPPORTED), ("strided16 odd row_bytes", E.ERR_INVALID_ARG),
                       ("batch n 0", 0), ("batch n above SSIMU2_MAX_BATCH", E.ERR_INVALID_ARG), ("batch null item", E.ERR_INVALID_ARG),
                       ("batch in a recursive mode", E.ERR_UNSUPPORTED), ("against after the blur switch", E.ERR_NO_REFERENCE),
                       ("map against a 16-bit reference", E.ERR_UNSUPPORTED), ("reference survived all of that", 0),
                       ("host_alloc zero bytes", E.ERR_INVALID_ARG), ("host_free null", 0), ("last_averages null", E.ERR_INVALID_ARG)):
        assert codes[name] == code, name
    # a null context never reaches the service
    assert kit.lib.ssimu2_score_rgb8(None, None, None, 1, 1, 3, None) == E.ERR_INVALID_ARG
    remote.close()
    direct.close()


def test_device_pointer_and_enqueue_forms_are_refused(kit, svc):
    L = kit.lib
    api = Api(L, svc.socket)
    c, s, vp = api.ctx, ctypes.c_double(), ctypes.c_void_p(4096)
    U = _lib.ERR_UNSUPPORTED
    assert L.ssimu2_score_rgb8_device(c, vp, vp, 8, 8, ctypes.byref(s)) == U and "scoring service" in api.err()
    assert "ssimu2_score_rgb8_device" in api.err()
    assert L.ssimu2_enqueue_rgb8_device(c, vp, vp, 8, 8) == U
    assert L.ssimu2_wait(c, ctypes.byref(s)) == U
    assert L.ssimu2_set_reference_device(c, vp, 8, 8) == U
    assert L.ssimu2_enqueue_against_reference_device(c, vp) == U
    assert L.ssimu2_score_batch_rgb8_device(c, vp, vp, 192, 1, 8, 8, ctypes.byref(s)) == U
    assert L.ssimu2_score_batch_against_reference_device(c, vp, 192, 1, ctypes.byref(s)) == U
    a, b = _frames(8, 8, 1)
    assert L.ssimu2_score_rgb8(c, _p8(a), _p8(b), 8, 8, 3, ctypes.byref(s)) == 0      # the context is still good
    api.close()
    # the instrumented library's hooks likewise
    I = _lib.instr_lib()
    api = Api(I, svc.socket)
    kind = ctypes.c_int()
    assert I.ssimu2_instr_last_march(api.ctx, ctypes.byref(kind)) == U and "scoring service" in api.err()
    assert I.ssimu2_instr_set_segment_rows(api.ctx, 0, 0) == U
    api.close()


# ---- 4. the C host through the service ---------------------------------------------------------------------------------
def test_the_c_host_through_the_service_equals_the_host_linked_against_the_scorer(kit, svc, tmp_path):
    from oavif_amd import avif_bridge as ab
    from oavif_amd import synth
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    from PIL import Image
    if obuild.host_needs_build():
        obuild.build_host()
    objs = []
    for src, cc, std in ((os.path.join(CSRC, "oavif_host.c"), "gcc", "-std=gnu11"), (os.path.join(CSRC, "tq.cpp"), "g++", "-std=c++17"),
                         (os.path.join(CSRC, "png_ingest.cpp"), "g++", "-std=c++17"), (STUB, "gcc", "-std=gnu11")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, "-O1", "-I", INC, "-c", src, "-o", obj], check=True, capture_output=True)
        objs.append(obj)
    linked = str(tmp_path / "host_stub")
    subprocess.run(["g++", *objs, "-o", linked, "-ldl", "-lm", "-lz", "-lpthread"], check=True, capture_output=True)
    png = tmp_path / "a.png"
    Image.fromarray(synth.make_ref(160, 120, 5)).save(png)
    args = ["--score-tgt", "91", "--tolerance", "1", "--max-pass", "8", "--tenbit", "0", "-s", "10"]
    env = dict(os.environ, OAVIF_LIBAVIF=ab._find_library())
    env.pop(ENV, None)
    res = {}
    for name, exe, extra in (("linked", linked, {}), ("service", obuild.HOST_PATH, {ENV: svc.socket}),
                             ("service, decode into its own memory off", obuild.HOST_PATH, {ENV: svc.socket, "OAVIF_HOST_PINNED": "0"}),
                             ("service, 4 probes at a time", obuild.HOST_PATH, {ENV: svc.socket, "OAVIF_PROBE_FANOUT": "4"})):
        out = tmp_path / "o.avif"
        r = subprocess.run([exe, *args, str(png), str(out)], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert r.returncode == 0, (name, r.stderr[-1500:])
        found = [l for l in r.stderr.splitlines() if l.startswith("Found q")]
        assert len(found) == 1, r.stderr
        res[name] = (found[0], out.read_bytes())
    assert int(re.search(r"(\d+) passes", res["linked"][0]).group(1)) >= 2          # a real multi-pass search
    assert all(v == res["linked"] for v in res.values()), {k: v[0] for k, v in res.items()}


# ---- 5. failures ----------------------------------------------------------------------------------------------------
def test_no_server_is_no_device_with_the_path_in_the_message(kit, tmp_path):
    path = _sock(tmp_path, "nobody.sock")
    api = Api(kit.lib, path, expect=_lib.ERR_NO_DEVICE)
    msg = kit.lib.ssimu2_last_error(None).decode()
    assert path in msg and "connect" in msg
    assert not api.ctx.value


def _hello(sock_path, proto=PROTO, version=b"", fds=(), flags=1, magic=MAGIC):
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(10)
    s.connect(sock_path)
    msg = HELLO.pack(magic, proto, flags, 0, 0, version)
    if fds:
        socket.send_fds(s, [msg], list(fds))
    else:
        s.sendall(msg)
    return s


def _read(s, n):
    buf = b""
    while len(buf) < n:
        chunk = s.recv(n - len(buf))
        if not chunk:
            break
        buf += chunk
    return buf


def _memfd(size):
    fd = os.memfd_create("test_frames", os.MFD_CLOEXEC | os.MFD_ALLOW_SEALING)
    os.ftruncate(fd, size)
    fcntl.fcntl(fd, fcntl.F_ADD_SEALS, fcntl.F_SEAL_SHRINK)
    return fd


def test_wrong_protocol_version_or_version_string_is_refused(kit, svc, tmp_path):
    fd = _memfd(4096)
    s = _hello(svc.socket, proto=PROTO + 1, version=kit.version.encode(), fds=[fd])
    magic, rc, _info, text = HELLO_REPLY.unpack(_read(s, HELLO_REPLY.size))
    assert magic == MAGIC and rc == _lib.ERR_NO_DEVICE and b"protocol version" in text
    assert _read(s, 1) == b""                                    # and the connection is closed
    s.close()
    s = _hello(svc.socket, version=b"some other build", fds=[fd])
    magic, rc, _info, text = HELLO_REPLY.unpack(_read(s, HELLO_REPLY.size))
    assert rc == _lib.ERR_NO_DEVICE and b"version differs" in text and _read(s, 1) == b""
    s.close()
    os.close(fd)
    # the library against a service of another build: no context, the reason in the message, no fallback
    other = _start(kit, version="oavif_amd ssimu2 gfx950 v7 (an older build)", socket=_sock(tmp_path, "old.sock"))
    try:
        Api(kit.lib, other.socket, expect=_lib.ERR_NO_DEVICE)
        msg = kit.lib.ssimu2_last_error(None).decode()
        assert other.socket in msg and "version differs" in msg and "v7" in msg
    finally:
        assert other.stop() == 0


def test_a_killed_server_is_a_hip_error_within_the_timeout_and_stays_one(kit, tmp_path):
    s = _start(kit, socket=_sock(tmp_path, "k.sock"))
    with _environ(OAVIF_SCORER_TIMEOUT_S="2"):
        api = Api(kit.lib, s.socket)
    a, b = _frames(40, 30, 2)
    out = ctypes.c_double()
    assert kit.lib.ssimu2_set_reference(api.ctx, _p8(a), 40, 30) == 0
    assert kit.lib.ssimu2_score_against_reference(api.ctx, _p8(b), ctypes.byref(out)) == 0
    s.proc.kill()                                                # SIGKILL between two calls (the stand-in: no GPU here)
    s.proc.wait()
    t0 = time.monotonic()
    for _ in range(3):
        assert kit.lib.ssimu2_score_against_reference(api.ctx, _p8(b), ctypes.byref(out)) == _lib.ERR_HIP
        assert api.err() == "scoring service: connection lost"
    assert kit.lib.ssimu2_set_reference(api.ctx, _p8(a), 40, 30) == _lib.ERR_HIP
    p = ctypes.c_void_p()
    assert kit.lib.ssimu2_host_alloc(api.ctx, 64, ctypes.byref(p)) == _lib.ERR_HIP
    assert time.monotonic() - t0 < 2.0
    api.close()
    s.stop()
    os.unlink(s.socket)                                          # SIGKILL leaves the file; the next service replaces it


def test_a_silent_server_times_out(kit, tmp_path):
    """Something that accepts and never answers: the handshake gives up after OAVIF_SCORER_TIMEOUT_S."""
    path = _sock(tmp_path, "mute.sock")
    srv = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    srv.bind(path)
    srv.listen(1)
    t0 = time.monotonic()
    with _environ(OAVIF_SCORER_TIMEOUT_S="0.3"):
        Api(kit.lib, path, expect=_lib.ERR_NO_DEVICE)
    assert 0.25 < time.monotonic() - t0 < 5.0 and path in kit.lib.ssimu2_last_error(None).decode()
    srv.close()


def test_after_a_hip_error_the_server_answers_refuses_and_exits_nonzero(kit, tmp_path):
    s = _start(kit, socket=_sock(tmp_path, "f.sock"))
    one, two = Api(kit.lib, s.socket), Api(kit.lib, s.socket)
    a, b = _frames(13, 13, 2)                                    # the stand-in's injected SSIMU2_ERR_HIP
    c, d = _frames(20, 10, 2)
    out = ctypes.c_double()
    assert kit.lib.ssimu2_score_rgb8(two.ctx, _p8(c), _p8(d), 20, 10, 3, ctypes.byref(out)) == 0
    assert kit.lib.ssimu2_score_rgb8(one.ctx, _p8(a), _p8(b), 13, 13, 3, ctypes.byref(out)) == _lib.ERR_HIP
    text = one.err()
    assert "injected HIP error" in text and "scoring service" in text
    # every later request, on every connection: the same code and text, nothing reaches the scorer
    assert kit.lib.ssimu2_score_rgb8(two.ctx, _p8(c), _p8(d), 20, 10, 3, ctypes.byref(out)) == _lib.ERR_HIP and two.err() == text
    assert kit.lib.ssimu2_ctx_set_blur(one.ctx, 0) == _lib.ERR_HIP and one.err() == text
    Api(kit.lib, s.socket, expect=_lib.ERR_HIP)
    assert "injected HIP error" in kit.lib.ssimu2_last_error(None).decode()
    one.close()
    two.close()
    assert s.proc.wait(timeout=10) == 3 and not os.path.exists(s.socket)
    s.stop()


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------
def test_idle_exit_max_lifetime_and_sigterm_end_the_server_and_remove_the_socket(kit, tmp_path):
    idle = _start(kit, socket=_sock(tmp_path, "i.sock"), idle_exit=0.3)
    api = Api(kit.lib, idle.socket)
    assert os.stat(idle.socket).st_mode & 0o7777 == 0o600
    time.sleep(0.5)                                              # connected: not idle
    assert idle.proc.poll() is None
    api.close()
    assert idle.proc.wait(timeout=10) == 0 and not os.path.exists(idle.socket)
    idle.stop()
    life = _start(kit, socket=_sock(tmp_path, "l.sock"), max_lifetime=0.5)
    api = Api(kit.lib, life.socket)                              # whatever is connected
    assert life.proc.wait(timeout=10) == 0 and not os.path.exists(life.socket)
    a, b = _frames(8, 8, 1)
    assert kit.lib.ssimu2_score_rgb8(api.ctx, _p8(a), _p8(b), 8, 8, 3, ctypes.byref(ctypes.c_double())) == _lib.ERR_HIP
    api.close()
    life.stop()
    term = _start(kit, socket=_sock(tmp_path, "t.sock"))
    term.proc.send_signal(signal.SIGTERM)
    assert term.proc.wait(timeout=10) == 0 and not os.path.exists(term.socket)
    term.stop()
    with _start(kit) as private:                                 # the default socket: in a directory of its own, 0700
        assert os.stat(os.path.dirname(private.socket)).st_mode & 0o7777 == 0o700
        d = os.path.dirname(private.socket)
    assert not os.path.exists(d)


def test_the_server_leaves_when_its_parent_is_gone(kit, tmp_path):
    """A launcher starts the service and dies without stopping it: --parent-pid ends the service."""
    sock = _sock(tmp_path, "p.sock")
    code = ("import os, sys\nsys.path.insert(0, %r)\nfrom oavif_amd import service\n"
            "s = service.start(socket=%r, program=%r, max_lifetime=60)\nprint(s.proc.pid, flush=True)\nsys.stdin.read()\n") % (ROOT, sock, kit.server)
    launcher = subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                env=dict(os.environ, STUB_SCORER_VERSION=kit.version))
    pid = int(launcher.stdout.readline())
    assert os.path.exists(sock)
    launcher.kill()
    launcher.wait()
    deadline = time.monotonic() + 10
    while os.path.exists(sock) and time.monotonic() < deadline:
        time.sleep(0.02)
    assert not os.path.exists(sock)
    while time.monotonic() < deadline:
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        time.sleep(0.02)
    else:
        pytest.fail("the service outlived its launcher")


def test_a_live_socket_is_not_stolen_and_a_stale_one_is_replaced(kit, svc, tmp_path):
    with _environ(STUB_SCORER_VERSION=kit.version):
        r = subprocess.run(service.command(svc.socket, max_lifetime=5, program=kit.server), capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and "running service" in r.stderr and "ready" not in r.stdout
    api = Api(kit.lib, svc.socket)                               # the first one still serves
    api.close()
    stale = _sock(tmp_path, "stale.sock")
    old = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    old.bind(stale)
    old.close()                                                  # the file stays, nobody listens
    assert os.path.exists(stale)
    with _start(kit, socket=stale) as s:
        Api(kit.lib, s.socket).close()
    plain = tmp_path / "file.sock"
    plain.write_text("not a socket")
    with _environ(STUB_SCORER_VERSION=kit.version):
        r = subprocess.run(service.command(str(plain), max_lifetime=5, program=kit.server), capture_output=True, text=True, timeout=30)
    assert r.returncode == 2 and plain.read_text() == "not a socket"


def test_max_contexts_gives_the_next_client_oom_and_a_freed_slot_is_reusable(kit, tmp_path):
    with _start(kit, socket=_sock(tmp_path, "m.sock"), max_contexts=2) as s:
        one, two = Api(kit.lib, s.socket), Api(kit.lib, s.socket)
        t0 = time.monotonic()
        Api(kit.lib, s.socket, expect=_lib.ERR_OOM)              # answered at once, never left waiting
        assert time.monotonic() - t0 < 2.0
        msg = kit.lib.ssimu2_last_error(None).decode()
        assert "--max-contexts" in msg and "2 contexts" in msg
        with _environ(**{ENV: s.socket}):                        # a device query takes no slot
            assert kit.lib.ssimu2_query_device(0, ctypes.byref(_lib.DeviceInfo())) == 0
        one.close()
        deadline = time.monotonic() + 5
        while True:                                              # the server sees the close a moment later
            three = Api.__new__(Api)
            three.L, three.ctx, three.keep = kit.lib, ctypes.c_void_p(), []
            with _environ(**{ENV: s.socket}):
                rc = kit.lib.ssimu2_ctx_create(0, None, ctypes.byref(three.ctx))
            if rc == 0 or time.monotonic() > deadline:
                break
            time.sleep(0.01)
        assert rc == 0
        a, b = _frames(8, 8, 1)
        out = ctypes.c_double()
        assert kit.lib.ssimu2_score_rgb8(three.ctx, _p8(a), _p8(b), 8, 8, 3, ctypes.byref(out)) == 0
        assert kit.lib.ssimu2_score_rgb8(two.ctx, _p8(a), _p8(b), 8, 8, 3, ctypes.byref(out)) == 0
        two.close()
        three.close()


# ---- 7. the pool ------------------------------------------------------------------------------------------------------
def test_a_pooled_context_comes_back_fresh(kit, tmp_path):
    """One slot, so connection B gets the context connection A used: default blur, no reference, no error text."""
    with _start(kit, socket=_sock(tmp_path, "pool.sock"), max_contexts=1) as s:
        L = kit.lib
        a, b = _frames(30, 20, 4)
        out = ctypes.c_double()
        A = Api(L, s.socket)
        assert L.ssimu2_ctx_set_blur(A.ctx, _lib.BLUR_RECURSIVE) == 0
        assert L.ssimu2_set_reference(A.ctx, _p8(a), 30, 20) == 0
        assert L.ssimu2_score_against_reference(A.ctx, _p8(b), ctypes.byref(out)) == 0
        assert L.ssimu2_ctx_set_blur(A.ctx, 9) == _lib.ERR_INVALID_ARG and A.err()
        A.close()
        deadline = time.monotonic() + 5
        while True:
            B = Api.__new__(Api)
            B.L, B.ctx, B.keep = L, ctypes.c_void_p(), []
            with _environ(**{ENV: s.socket}):
                rc = L.ssimu2_ctx_create(0, None, ctypes.byref(B.ctx))
            if rc == 0 or time.monotonic() > deadline:
                break
            time.sleep(0.01)
        assert rc == 0
        assert B.err() == ""
        assert L.ssimu2_score_against_reference(B.ctx, _p8(b), ctypes.byref(out)) == _lib.ERR_NO_REFERENCE
        PA = ctypes.POINTER(ctypes.c_uint8) * 1
        scores = np.zeros(1)
        assert L.ssimu2_score_batch_rgb8(B.ctx, PA(_p8(a)), PA(_p8(b)), 1, 30, 20,
                                         scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0      # FIR: batches run
        assert scores[0] == _score8(a, b)
        B.close()


# ---- 8. sanitizers: stand-alone programs only -------------------------------------------------------------------------
def _san_server(kit, tmp_path, san):
    return obuild.build_service(scorer=[STUB], out=str(tmp_path / f"scored_{san.split(',')[0]}"),
                                flags=["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"])


def _request(op, a=(0, 0, 0, 0), flags=0, shm=4096, in0=(NULL, 0), in1=(NULL, 0), out=(NULL, 0), magic=MAGIC):
    return REQUEST.pack(magic, op, *a, flags, 0, shm, *in0, *in1, *out)


def test_the_server_survives_malformed_messages_under_asan_and_ubsan(kit, tmp_path):
    """The server (a stand-alone program) under ASan + UBSan + LSan, fed truncated, oversized, inconsistent and random
    messages over a raw socket: no report, only that connection is closed, the next client is served."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    exe = _san_server(kit, tmp_path, "address,undefined")
    sock = _sock(tmp_path, "a.sock")
    with _environ(STUB_SCORER_VERSION=kit.version, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"):
        proc = subprocess.Popen(service.command(sock, max_lifetime=120, program=exe), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        assert proc.stdout.readline().startswith(b"ready ")
        ver = kit.version.encode()
        rng = np.random.default_rng(11)

        def session():
            fd = _memfd(8192)
            s = _hello(sock, version=ver, fds=[fd])
            rep = HELLO_REPLY.unpack(_read(s, HELLO_REPLY.size))
            assert rep[1] == 0
            return s, fd

        def closed(s):
            try:
                return _read(s, 1) == b""
            except ConnectionResetError:
                return True

        def served():
            api = Api(kit.lib, sock)
            a, b = _frames(33, 9, 1)
            out = ctypes.c_double()
            assert kit.lib.ssimu2_score_rgb8(api.ctx, _p8(a), _p8(b), 33, 9, 3, ctypes.byref(out)) == 0 and out.value == _score8(a, b)
            api.close()

        frame = 16 * 16 * 3
        bad = [
            _request(2, (16, 16, 3, 0), shm=8192, in0=(0, frame), in1=(8192 - 10, frame)),      # past the end of the file
            _request(2, (16, 16, 3, 0), shm=8192, in0=(0, frame - 1), in1=(1024, frame)),       # length not what w, h imply
            _request(2, (16, 16, 3, 0), shm=8192, in0=(NULL - 5, frame), in1=(0, frame)),       # offset + length wraps
            _request(2, (16, 16, 3, 0), shm=1 << 30, in0=(0, frame), in1=(1024, frame)),        # a file size it does not have
            _request(2, (16, 16, 3, 0), shm=1 << 62, in0=(0, frame), in1=(1024, frame)),
            _request(10, (16, 16, 3, 0), shm=8192, in0=(0, frame), in1=(1024, frame), out=(8000, 16 * 16 * 4)),   # map past the end
            _request(10, (16, 16, 3, 0), shm=8192, in0=(0, frame), in1=(1024, frame), out=(4097, 16 * 16 * 4)),   # misaligned output
            _request(13, (3, 16, 16, 0), shm=8192, in0=(0, 24), in1=(64, 24), out=(4096, 16)),  # batch: 3 items, 2 scores
            _request(0), _request(16), _request(0xFFFFFFFF), _request(2, magic=7),
            _request(12, shm=8192, out=(8192 - 8, 864)),
            _request(2, (16, 16, 3, 0))[:40],                                                    # truncated, then closed
        ]
        for i, msg in enumerate(bad):
            s, fd = session()
            s.sendall(msg)
            if len(msg) < REQUEST.size:
                s.shutdown(socket.SHUT_WR)
            assert closed(s), i
            s.close()
            os.close(fd)
            served()
        # a batch whose offset array points outside the file
        s, fd = session()
        with open(fd, "r+b", closefd=False) as f:
            f.write(struct.pack("<3Q", 0, 1 << 40, 64))
        s.sendall(_request(13, (3, 16, 16, 0), shm=8192, in0=(0, 24), in1=(0, 24), out=(4096, 24)))
        assert closed(s)
        s.close()
        os.close(fd)
        served()
        # handshakes: no descriptor, a descriptor that is no sealed memfd, an unterminated version, noise
        for kw in (dict(fds=()), dict(fds=[os.open(os.devnull, os.O_RDONLY)]), dict(version=b"x" * 512, fds=[_memfd(4096)]), dict(magic=1)):
            s = _hello(sock, **{"version": ver, **kw})
            data = _read(s, HELLO_REPLY.size)
            assert data == b"" or HELLO_REPLY.unpack(data)[1] == _lib.ERR_NO_DEVICE
            assert closed(s)
            s.close()
            for f in kw.get("fds", ()):
                os.close(f)
        for _ in range(40):
            s, fd = session()
            blob = rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
            if rng.integers(0, 2):
                blob = struct.pack("<II", MAGIC, int(rng.integers(0, 18))) + blob       # past the first check
            s.sendall(blob)
            s.shutdown(socket.SHUT_WR)
            while True:                                         # whatever it answers, it ends the connection
                try:
                    if not s.recv(4096):
                        break
                except ConnectionResetError:
                    break
            s.close()
            os.close(fd)
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)   # connects and says nothing, then leaves
        s.connect(sock)
        s.close()
        served()
        proc.send_signal(signal.SIGTERM)
        _out, err = proc.communicate(timeout=30)
        assert proc.returncode == 0, err.decode()[-3000:]
        assert b"Sanitizer" not in err and b"runtime error" not in err, err.decode()[-3000:]
        assert not os.path.exists(sock)
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.wait()


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_server_and_client_under_sanitizers_with_eight_concurrent_clients(kit, tmp_path, san):
    """oavif_scored and a stand-alone driver of remote_client.cpp (tests/c/service_client_driver.cpp), both built with
    the sanitizer: 8 clients at once, every answer the stand-in's formula, no report from either program."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    flags = ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    exe = _san_server(kit, tmp_path, san)
    driver = str(tmp_path / "client_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, "-I", CSRC, os.path.join(CSRC, "remote_client.cpp"),
                    os.path.join(ROOT, "tests", "c", "service_client_driver.cpp"), "-o", driver, "-lpthread"], check=True)
    sock = _sock(tmp_path, "s.sock")
    env = dict(os.environ, STUB_SCORER_VERSION=kit.version, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1", **{ENV: sock})
    proc = subprocess.Popen(service.command(sock, max_lifetime=120, program=exe), stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, env={k: v for k, v in env.items() if k != ENV})
    try:
        assert proc.stdout.readline().startswith(b"ready ")
        for _ in range(2):
            r = subprocess.run([driver, kit.version, "8", "3"], capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        proc.send_signal(signal.SIGTERM)
        _out, err = proc.communicate(timeout=30)
        assert proc.returncode == 0 and b"Sanitizer" not in err and b"runtime error" not in err, err.decode()[-3000:]
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.wait()
