"""Host-side mirror of the scorer interface the reference binds at tq.zig:37.

    fssimu2.computeSsimu2(allocator, ref, dist, w, h, 3, null) -> f64      (tq.zig:37)

`Ssimu2.compute_ssimu2(ref, dist)` is that call on the MI355X; errors surface as
`Ssimu2Error` carrying the C ABI's negative code (the Zig error-union counterpart).
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref

import numpy as np

from . import _lib


class Ssimu2Error(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ssimu2 error {code}: {msg}")
        self.code = code


_F64P = ctypes.POINTER(ctypes.c_double)

# OAVIF_SCORER_SOCKET is read by ssimu2_ctx_create at every call: Ssimu2(..., service=...) sets it around that one call
SERVICE_ENV = "OAVIF_SCORER_SOCKET"
_service_lock = threading.Lock()


def _u8p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _check_rgb8(a, name: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{name} must be (h, w, 3) uint8, got {a.shape}")
    return a


def _u16p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def _check_rgb16(a, name: str) -> np.ndarray:
    """An (h, w, 3) uint16 array as the 16-bit calls take it (no silent conversion from another dtype)."""
    a = np.asarray(a)
    if a.dtype != np.uint16:
        raise TypeError(f"{name} must be uint16 (16-bit samples), got {a.dtype}")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{name} must be (h, w, 3) uint16, got {a.shape}")
    return np.ascontiguousarray(a)


def _check_pair(ref, dist, check):
    """Two frames of one shape, each through `check` (_check_rgb8 / _check_rgb16)."""
    ref, dist = check(ref, "ref"), check(dist, "dist")
    if ref.shape != dist.shape:
        raise ValueError("ref and dist must have the same shape")
    return ref, dist


def linear_table(bit_depth: int) -> np.ndarray:
    """ssimu2_linear_table: the 2^bit_depth-entry sRGB -> linear table the 16-bit calls read (host only, no device)."""
    L = _lib.lib()
    out = np.empty(1 << max(0, min(int(bit_depth), 16)), np.float32)
    rc = L.ssimu2_linear_table(int(bit_depth), _f32p(out))
    if rc != 0:
        raise Ssimu2Error(rc, f"bit_depth {bit_depth} outside 8..16" if rc == _lib.ERR_UNSUPPORTED else "ssimu2_linear_table failed")
    return out


def alpha_table() -> np.ndarray:
    """ssimu2_alpha_table: the 65,026-entry table T the RGBA calls read composite codes n = a*c + (255 - a)*b through
    (include/ssimu2_hip_ext.h; host only, no device).  Needs the extension library."""
    out = np.empty(_lib.ALPHA_CODES, np.float32)
    rc = _lib.ext_lib().ssimu2_alpha_table(_f32p(out))
    if rc != 0:
        raise Ssimu2Error(rc, "ssimu2_alpha_table failed")
    return out


def background_rgb(background) -> int:
    """An (r, g, b) tuple of 8-bit values or an 0xRRGGBB int -> 0xRRGGBB."""
    if isinstance(background, (int, np.integer)):
        v = int(background)
        if not 0 <= v <= 0xFFFFFF:
            raise ValueError(f"background must be 0xRRGGBB, got {v:#x}")
        return v
    r, g, b = (int(x) for x in background)
    if not all(0 <= x <= 255 for x in (r, g, b)):
        raise ValueError(f"background components must be 0..255, got {(r, g, b)}")
    return r << 16 | g << 8 | b


def _check_rgba8(a, name: str) -> np.ndarray:
    """An (h, w, 4) uint8 frame whose pixels are tightly packed within a row; rows any distance >= 4 w apart (a view
    into libavif's padded rows goes through as it is, anything else is copied)."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{name} must be uint8 RGBA, got {a.dtype}")
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"{name} must be (h, w, 4) uint8, got {a.shape}")
    if a.strides[2] != 1 or a.strides[1] != 4 or (a.shape[0] > 1 and a.strides[0] < 4 * a.shape[1]):
        a = np.ascontiguousarray(a)
    return a


MATRIX_COEFFICIENTS = (1, 2, 5, 6, 9)   # the CICP codes include/ssimu2_hip_yuv.h converts


class YuvFrame:
    """A decoder's planes as the YUV calls take them (ssimu2_yuv_frame, include/ssimu2_hip_yuv.h): `planes` is (Y, U, V)
    for format _lib.YUV_444 or (Y,) for _lib.YUV_400, each an (h, w) array -- uint8 at depth 8, uint16 at depth 10 and
    12 -- whose rows may be any distance apart (a strided view of libavif's yuvPlanes goes through as it is; a view
    whose samples are not adjacent within a row is copied).  For the subsampled formats _lib.YUV_422 and _lib.YUV_420
    (include/ssimu2_hip_chroma.h, a chroma=True context) U and V are (ch, cw) with cw = (w + 1) // 2 and ch = h (4:2:2)
    or (h + 1) // 2 (4:2:0); `width` and `height` are plane 0's.  `full_range` and `matrix_coefficients` are the image's
    yuvRange and CICP matrix code.  `alpha` (include/ssimu2_hip_yuva.h, a yuva=True context): the image's alpha plane, an
    array of plane 0's shape and dtype whose rows may be any distance apart, straight and full range; None = opaque.
    `alpha_premultiplied` is the image's flag, which the library refuses when it is set."""

    def __init__(self, planes, depth: int = 8, format: int = _lib.YUV_444, full_range: bool = True,
                 matrix_coefficients: int = 6, alpha=None, alpha_premultiplied: bool = False):
        self.depth, self.format = int(depth), int(format)
        self.full_range, self.matrix_coefficients = int(full_range), int(matrix_coefficients)
        self.subsampled = self.format in (_lib.YUV_422, _lib.YUV_420)
        dtype = np.uint8 if self.depth == 8 else np.uint16
        need = 1 if self.format == _lib.YUV_400 else 3
        planes = list(planes)[:need]
        if len(planes) < need:
            raise ValueError(f"format {self.format} needs {need} plane(s), got {len(planes)}")
        self.planes = []
        for k, a in enumerate(planes):
            a = np.asarray(a)
            if a.dtype != dtype:
                raise TypeError(f"plane {k} of a {self.depth}-bit frame must be {np.dtype(dtype).name}, got {a.dtype}")
            if k and self.subsampled:   # plane 0 has passed: (ch, cw) of its (h, w)
                h0, w0 = self.planes[0].shape
                want = ((h0 + 1) // 2 if self.format == _lib.YUV_420 else h0, (w0 + 1) // 2)
                if a.shape != want:
                    raise ValueError(f"plane {k} of a subsampled frame (format {self.format}) must be (ch, cw) = {want} "
                                     f"for a {w0} x {h0} plane 0, got {a.shape}")
            elif a.ndim != 2 or a.shape != np.asarray(planes[0]).shape:
                raise ValueError(f"plane {k} must be (h, w) like plane 0, got {a.shape}")
            if a.strides[1] != a.itemsize or (a.shape[0] > 1 and a.strides[0] < a.shape[1] * a.itemsize):
                a = np.ascontiguousarray(a)
            self.planes.append(a)
        self.height, self.width = self.planes[0].shape
        self.alpha, self.alpha_premultiplied = None, int(bool(alpha_premultiplied))
        if alpha is not None:
            a = np.asarray(alpha)
            if a.dtype != dtype:
                raise TypeError(f"the alpha plane of a {self.depth}-bit frame must be {np.dtype(dtype).name}, got {a.dtype}")
            if a.ndim != 2 or a.shape != self.planes[0].shape:
                raise ValueError(f"the alpha plane must be (h, w) like plane 0, got {a.shape}")
            if a.strides[1] != a.itemsize or (a.shape[0] > 1 and a.strides[0] < a.shape[1] * a.itemsize):
                a = np.ascontiguousarray(a)
            self.alpha = a

    def as_c(self) -> "_lib.YuvFrameC":
        """The C struct; it points into self.planes, which must stay alive for the call."""
        c = _lib.YuvFrameC()
        for k, a in enumerate(self.planes):
            c.planes[k] = a.ctypes.data
            c.row_bytes[k] = a.strides[0] if a.shape[0] > 1 else a.shape[1] * a.itemsize
        c.depth, c.format, c.full_range, c.matrix_coefficients = self.depth, self.format, self.full_range, self.matrix_coefficients
        return c

    def as_yuva_c(self) -> "_lib.YuvaFrameC":
        """ssimu2_yuva_frame; it points into self.planes and self.alpha, which must stay alive for the call."""
        c = _lib.YuvaFrameC()
        c.yuv = self.as_c()
        if self.alpha is not None:
            a = self.alpha
            c.alpha = a.ctypes.data
            c.alpha_row_bytes = a.strides[0] if a.shape[0] > 1 else a.shape[1] * a.itemsize
        c.alpha_premultiplied = self.alpha_premultiplied
        return c


def query_device(device: int = 0, instrumented: bool = False) -> dict:
    """ssimu2_query_device: what the library reads off HIP device `device` without creating a context
    (`usable` False = ssimu2_ctx_create would refuse it: not gfx950, or less than 160 KB of LDS per CU)."""
    L = _lib.instr_lib() if instrumented else _lib.lib()
    d = _lib.DeviceInfo()
    rc = L.ssimu2_query_device(int(device), ctypes.byref(d))
    if rc != 0:
        raise Ssimu2Error(rc, L.ssimu2_last_error(None).decode() or "ssimu2_query_device failed")
    return d.as_dict()


class _CtxHolder:
    """The native context and who still needs it: the Ssimu2 object that created it (`owner`) and every page-locked buffer
    handed out by host_alloc whose numpy array is still referenced.  ssimu2_ctx_destroy runs when the owner has closed AND
    the last such array is gone -- closing a scorer never unmaps memory a live array points into."""

    def __init__(self, L, ctx):
        self.L, self.ctx, self.owner, self.buffers = L, ctx, True, 0

    def release_owner(self):
        self.owner = False
        self._maybe_destroy()

    def buffer_gone(self):
        self.buffers -= 1
        self._maybe_destroy()

    def _maybe_destroy(self):
        if not self.owner and self.buffers <= 0 and self.ctx is not None and self.ctx.value:
            self.L.ssimu2_ctx_destroy(self.ctx)
            self.ctx = None


class _PinnedBuffer:
    """One allocation of ssimu2_host_alloc as the base object of the numpy array handed to the caller: every view of that
    array keeps this object alive, and the memory is returned (ssimu2_host_free) when the last of them is gone or when the
    caller says host_free.  Freed exactly once."""

    def __init__(self, holder: _CtxHolder, ptr: int, nbytes: int):
        self.holder, self.ptr, self.nbytes, self.freed = holder, ptr, nbytes, False
        holder.buffers += 1
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def free(self) -> int:
        if self.freed:
            return 0
        self.freed = True
        rc = 0
        if self.holder.ctx is not None and self.holder.ctx.value:
            rc = self.holder.L.ssimu2_host_free(self.holder.ctx, ctypes.c_void_p(self.ptr))
        self.holder.buffer_gone()
        return rc

    def __del__(self):
        try:
            self.free()
        except Exception:   # interpreter shutdown
            pass


# the batch calls of include/ssimu2_hip.h -> their counterparts of include/ssimu2_hip_rbatch.h (Ssimu2._batch_fn)
_RBATCH_CALLS = {"ssimu2_score_batch_rgb8": "ssimu2_rbatch_score_rgb8",
                 "ssimu2_score_batch_against_reference": "ssimu2_rbatch_score_against_reference",
                 "ssimu2_score_batch_rgb8_device": "ssimu2_rbatch_score_rgb8_device",
                 "ssimu2_score_batch_against_reference_device": "ssimu2_rbatch_score_against_reference_device"}


class Ssimu2:
    """One scorer context = one HIP stream + device scratch (not re-entrant)."""

    # (h, w, 3) of the cached reference, recorded by the calls that set one; None = none recorded, the library decides
    _ref_shape = None

    extended = False   # bound to liboavif_hip_ext.so (the RGBA calls of include/ssimu2_hip_ext.h)
    yuv = False        # bound to liboavif_hip_yuv.so (the YUV calls of include/ssimu2_hip_yuv.h, and the RGBA calls)
    maps = False       # bound to liboavif_hip_map.so (the error maps of include/ssimu2_hip_map.h, and the RGBA and YUV calls)
    chroma = False     # bound to liboavif_hip_chroma.so (4:2:2 / 4:2:0 frames, include/ssimu2_hip_chroma.h, and all of the above)
    yuva = False       # bound to liboavif_hip_yuva.so (YUV frames with an alpha plane, include/ssimu2_hip_yuva.h, and all of the above)
    rbatch = False     # bound to liboavif_hip_rbatch.so (batches in every blur mode, include/ssimu2_hip_rbatch.h, and all of the above)
    hbatch = False     # bound to liboavif_hip_hbatch.so (16-bit and YUV batches, include/ssimu2_hip_hbatch.h, and all of the above)
    abatch = False     # bound to liboavif_hip_abatch.so (RGBA and YUV-with-alpha batches, include/ssimu2_hip_abatch.h, and all of the above)

    def __init__(self, device: int = 0, stream: int | None = None, instrumented: bool = False,
                 blur: int | None = None, service: str | None = None, extended: bool = False, yuv: bool = False,
                 maps: bool = False, chroma: bool = False, yuva: bool = False, rbatch: bool = False,
                 hbatch: bool = False, abatch: bool = False):
        """`service`: socket path of a running scoring service (oavif_amd.service): the context lives there, and this
        process makes no HIP call for it (OAVIF_SCORER_SOCKET set around ssimu2_ctx_create, then restored; None = the
        environment as it is).  `instrumented=True` binds liboavif_hip_instr.so (the hooks of
        include/ssimu2_hip_internal.h: stage timing, plane download, experiment knobs); the
        default is the product library, which has none of them.  `blur`: _lib.BLUR_FIR /
        _lib.BLUR_RECURSIVE (ssimu2_ctx_set_blur); None = FIR.  `extended=True` binds liboavif_hip_ext.so instead: the
        product library plus the RGBA calls of include/ssimu2_hip_ext.h (composite_rgba, compute_ssimu2_rgba,
        set_reference_rgba, score_against_reference_rgba); not together with `instrumented`.  `yuv=True` binds
        liboavif_hip_yuv.so: the YUV calls of include/ssimu2_hip_yuv.h (convert_yuv, compute_ssimu2_yuv,
        set_reference_yuv, score_against_reference_yuv); that library has the RGBA calls too, so `extended=True` may be
        given as well; not together with `instrumented`.  `maps=True` binds liboavif_hip_map.so: the error maps of
        16-bit, RGBA and YUV frames of include/ssimu2_hip_map.h (error_map_hbd, error_map_rgba, error_map_yuv and their
        against-reference forms); that library has the RGBA and YUV calls too, so `extended=True` / `yuv=True` may be
        given with it; not together with `instrumented`.  `chroma=True` binds liboavif_hip_chroma.so: everything
        `maps=True` has, the YUV calls included, and YuvFrames of the subsampled formats 4:2:2 and 4:2:0 in every YUV
        method (include/ssimu2_hip_chroma.h); not together with `instrumented`.  `yuva=True` binds liboavif_hip_yuva.so:
        everything `chroma=True` has, and the calls of include/ssimu2_hip_yuva.h that composite a YuvFrame with an alpha
        plane over a background (composite_yuva, compute_ssimu2_yuva, set_reference_yuva, score_against_reference_yuva,
        error_map_yuva_alpha, error_map_against_reference_yuva_alpha); not together with `instrumented`.  `rbatch=True`
        binds liboavif_hip_rbatch.so: everything `yuva=True` has, and score_batch, score_batch_against_reference and
        their _device forms go through the calls of include/ssimu2_hip_rbatch.h, which batch in the context's blur
        mode, the recursive ones included (without it they are SSIMU2_ERR_UNSUPPORTED there); not together with
        `instrumented`.  `hbatch=True` binds liboavif_hip_hbatch.so: everything `rbatch=True` has, and the batches of
        16-bit and YUV frames of include/ssimu2_hip_hbatch.h, which run in the recursive blur modes (score_batch_hbd,
        score_batch_against_reference_hbd, their _device forms, score_batch_against_reference_yuv, convert_yuv_batch);
        not together with `instrumented`.  `abatch=True` binds liboavif_hip_abatch.so: everything `hbatch=True` has, and
        the batches of frames with transparency of include/ssimu2_hip_abatch.h, which run in the recursive blur modes
        (score_batch_against_reference_yuva, composite_yuva_batch, score_batch_against_reference_rgba, score_batch_rgba,
        composite_rgba_batch); not together with `instrumented`."""
        if instrumented and abatch:
            raise ValueError("instrumented=True and abatch=True are different libraries: choose one")
        self.abatch = bool(abatch)
        hbatch = bool(hbatch or abatch)
        if instrumented and hbatch:
            raise ValueError("instrumented=True and hbatch=True are different libraries: choose one")
        self.hbatch = bool(hbatch)
        rbatch = bool(rbatch or hbatch)
        if instrumented and rbatch:
            raise ValueError("instrumented=True and rbatch=True are different libraries: choose one")
        self.rbatch = bool(rbatch)
        yuva = bool(yuva or rbatch)
        if instrumented and yuva:
            raise ValueError("instrumented=True and yuva=True are different libraries: choose one")
        chroma = bool(chroma or yuva)
        self.yuva = bool(yuva)
        if instrumented and chroma:
            raise ValueError("instrumented=True and chroma=True are different libraries: choose one")
        if instrumented and maps:
            raise ValueError("instrumented=True and maps=True are different libraries: choose one")
        if instrumented and extended:
            raise ValueError("instrumented=True and extended=True are different libraries: choose one")
        if instrumented and yuv:
            raise ValueError("instrumented=True and yuv=True are different libraries: choose one")
        self.chroma = bool(chroma)
        # a yuva context scores against RGBA references and beside RGBA frames: the RGBA methods come with it
        self.instrumented, self.extended = bool(instrumented), bool(extended or yuva)
        self.yuv, self.maps = bool(yuv or chroma), bool(maps or chroma)
        self._L = (_lib.instr_lib() if instrumented else _lib.abatch_lib() if abatch else _lib.hbatch_lib() if hbatch else _lib.rbatch_lib() if rbatch else _lib.yuva_lib() if yuva else _lib.chroma_lib() if chroma else _lib.map_lib() if maps
                   else _lib.yuv_lib() if yuv else _lib.ext_lib() if extended else _lib.lib())
        self._ctx = ctypes.c_void_p()
        self._holder = None
        if service is None:
            rc = self._L.ssimu2_ctx_create(int(device), ctypes.c_void_p(stream or 0), ctypes.byref(self._ctx))
        else:
            with _service_lock:
                before = os.environ.get(SERVICE_ENV)
                os.environ[SERVICE_ENV] = os.fspath(service)
                try:
                    rc = self._L.ssimu2_ctx_create(int(device), ctypes.c_void_p(stream or 0), ctypes.byref(self._ctx))
                finally:
                    if before is None:
                        del os.environ[SERVICE_ENV]
                    else:
                        os.environ[SERVICE_ENV] = before
        if rc != 0:
            msg = self._L.ssimu2_last_error(None).decode()
            self._ctx = ctypes.c_void_p()
            raise Ssimu2Error(rc, msg or "ssimu2_ctx_create failed")
        self._holder = _CtxHolder(self._L, ctypes.c_void_p(self._ctx.value))
        self._pinned = {}   # data address -> weak reference to the _PinnedBuffer behind a host_alloc array
        self.device = device
        if blur is not None and int(blur) != _lib.BLUR_FIR:
            self.set_blur(blur)

    def close(self) -> None:
        """The context is unusable from here on.  Page-locked buffers of host_alloc whose arrays are still referenced stay
        mapped -- and the native context alive underneath them -- until the last such array is dropped."""
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._ctx = ctypes.c_void_p()
            self._pinned = {}
            self._holder.release_owner()

    # -- the one call path: every C function of a context goes through here ---------------------
    def _raise(self, rc: int):
        raise Ssimu2Error(rc, self._L.ssimu2_last_error(self._ctx).decode())

    def _call(self, fn, *args) -> None:
        """fn(ctx, *args); a non-zero code raises Ssimu2Error with the library's text.  `fn` is the bound function
        object (self._L.ssimu2_...): no name lookup per call."""
        rc = fn(self._ctx, *args)
        if rc != 0:
            self._raise(rc)

    def _need_instr(self):
        if not self.instrumented:
            raise RuntimeError("this hook needs Ssimu2(..., instrumented=True) (liboavif_hip_instr.so)")

    def _icall(self, hook: str, *args) -> None:
        """A hook of include/ssimu2_hip_internal.h whose arguments are passed as they are, by name: the product library
        has no such attribute to pass, and the refusal comes first.  A hook that converts, sizes or allocates
        anything for its call does _need_instr() itself, before that, and then _call."""
        self._need_instr()
        self._call(getattr(self._L, hook), *args)

    # The three shapes of result.  The two scoring ones make the C call themselves, not through _call: one Python frame
    # per score, not two.
    def _score(self, fn, *args) -> float:
        """A call whose last parameter is `double* out_score`."""
        out = ctypes.c_double()
        rc = fn(self._ctx, *args, ctypes.byref(out))
        if rc != 0:
            self._raise(rc)
        return out.value

    def _scores(self, fn, n: int, *args) -> np.ndarray:
        """A batch call whose last parameter is `double* out_scores` (n of them)."""
        out = np.zeros(int(n), np.float64)
        rc = fn(self._ctx, *args, out.ctypes.data_as(_F64P))
        if rc != 0:
            self._raise(rc)
        return out

    def _averages(self, fn, *args):
        """-> ((6, 18) float64 plane averages, number of scales) of ssimu2_last_averages / ssimu2_last_batch_averages."""
        avg = np.zeros(_lib.NUM_SCALES * _lib.STATS_PER_SCALE, np.float64)
        ns = ctypes.c_int()
        self._call(fn, *args, avg.ctypes.data_as(_F64P), ctypes.byref(ns))
        return avg.reshape(_lib.NUM_SCALES, _lib.STATS_PER_SCALE), ns.value

    def _check_ref_shape(self, shape, what: str = "dist shape") -> None:
        """`shape`, (h, w, 3) or (h, w), against the recorded shape of the cached reference."""
        if self._ref_shape is not None and shape != self._ref_shape[:len(shape)]:
            raise ValueError(f"{what} differs from the reference's")

    def device_info(self) -> dict:
        """ssimu2_ctx_device_info: the record the context was created with (arch, LDS per CU, PCI bus id, ...)."""
        d = _lib.DeviceInfo()
        self._call(self._L.ssimu2_ctx_device_info, ctypes.byref(d))
        return d.as_dict()

    def host_alloc(self, shape) -> np.ndarray:
        """ssimu2_host_alloc: a uint8 array of `shape` in page-locked host memory (uploads from it skip the HIP runtime's
        staging copy).  The memory belongs to the array: it is returned when the array and all its views are gone, or at
        host_free(array) -- after which the caller must not touch the array again.  Closing the scorer first is safe (the
        memory stays mapped while an array points into it).  ssimu2_host_free synchronises the whole device: allocate
        once per context and reuse, never per score."""
        shape = tuple(int(x) for x in (shape if hasattr(shape, "__len__") else (shape,)))
        n = int(np.prod(shape))
        ptr = ctypes.c_void_p()
        self._call(self._L.ssimu2_host_alloc, n, ctypes.byref(ptr))
        buf = _PinnedBuffer(self._holder, ptr.value, n)
        a = np.asarray(buf).reshape(shape)      # a.base chain ends at `buf`
        self._pinned[a.ctypes.data] = weakref.ref(buf)
        return a

    def host_free(self, a: np.ndarray) -> None:
        """Return a host_alloc buffer now (a device-wide synchronisation, see host_alloc).  `a` and its views must not be
        used afterwards."""
        ref = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        buf = ref() if ref is not None else None
        if buf is None or buf.freed:
            raise ValueError("not a (live) buffer of this context's host_alloc")
        rc = buf.free()
        if rc != 0:
            self._raise(rc)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host-buffer entry points ---------------------------------------------------------
    def compute_ssimu2(self, ref, dist, channels: int = 3) -> float:
        ref, dist = _check_pair(ref, dist, _check_rgb8)
        h, w, _ = ref.shape
        return self._score(self._L.ssimu2_score_rgb8, _u8p(ref), _u8p(dist), w, h, channels)

    def error_map(self, ref, dist, channels: int = 3):
        """ssimu2_error_map_rgb8 -> (score, (h, w) float32 map): the score bit for bit as compute_ssimu2, and
        where the frame is damaged (the map's definition: include/ssimu2_hip.h)."""
        ref, dist = _check_pair(ref, dist, _check_rgb8)
        h, w, _ = ref.shape
        out = np.empty((h, w), np.float32)
        return self._score(self._L.ssimu2_error_map_rgb8, _u8p(ref), _u8p(dist), w, h, channels, _f32p(out)), out

    def error_map_against_reference(self, dist):
        """ssimu2_error_map_against_reference -> (score, (h, w) float32 map) against the cached reference."""
        dist = _check_rgb8(dist, "dist")
        self._check_ref_shape(dist.shape)
        h, w, _ = dist.shape
        out = np.empty((h, w), np.float32)
        return self._score(self._L.ssimu2_error_map_against_reference, _u8p(dist), _f32p(out)), out

    def set_reference(self, ref) -> None:
        ref = _check_rgb8(ref, "ref")
        h, w, _ = ref.shape
        self._call(self._L.ssimu2_set_reference, _u8p(ref), w, h)
        self._ref_shape = ref.shape

    def score_against_reference(self, dist) -> float:
        dist = _check_rgb8(dist, "dist")
        self._check_ref_shape(dist.shape)
        return self._score(self._L.ssimu2_score_against_reference, _u8p(dist))

    def _score_decoded(self, fn, a: np.ndarray, sample, row_bytes, channels, *bit_depth) -> float:
        """The body of score_decoded_against_reference[_hbd]: `a` holds samples of ctypes type `sample`."""
        size = ctypes.sizeof(sample)
        if a.ndim == 3:
            if a.strides[2] != size or a.strides[1] != size * a.shape[2]:
                raise ValueError("pixels of a row must be tightly packed")
            self._check_ref_shape(a.shape[:2], "frame size")
            row_bytes = a.strides[0] if row_bytes is None else row_bytes
            channels = a.shape[2] if channels is None else channels
        elif row_bytes is None or channels is None:
            raise ValueError("flat buffers need row_bytes and channels")
        ptr = ctypes.cast(ctypes.c_void_p(a.ctypes.data), ctypes.POINTER(sample))
        return self._score(fn, ptr, int(row_bytes), int(channels), *bit_depth)

    def score_decoded_against_reference(self, pixels, row_bytes: int | None = None,
                                        channels: int | None = None) -> float:
        """Score a decoded frame in libavif's avifRGBImage layout without the CPU copy loop of
        io.decodeAvifToRgb (io.zig:654-663): `pixels` is an (h, w, 3|4) uint8 array whose rows
        may be padded (strides[0] >= w * channels, pixels tightly packed within a row), or a flat
        uint8 buffer with explicit `row_bytes` / `channels`.  Alpha and padding are dropped on
        the device."""
        a = np.asarray(pixels)
        if a.dtype != np.uint8:
            raise TypeError("pixels must be uint8")
        return self._score_decoded(self._L.ssimu2_score_against_reference_strided, a, ctypes.c_uint8, row_bytes, channels)

    # -- 16-bit input (include/ssimu2_hip.h) --------------------------------
    def compute_ssimu2_hbd(self, ref, dist, bit_depth: int) -> float:
        """ssimu2_score_rgb16: (h, w, 3) uint16 frames of `bit_depth` (8..16) bits; samples above 2^d - 1 are clamped."""
        ref, dist = _check_pair(ref, dist, _check_rgb16)
        h, w, _ = ref.shape
        return self._score(self._L.ssimu2_score_rgb16, _u16p(ref), _u16p(dist), w, h, 3, int(bit_depth))

    def set_reference_hbd(self, ref, bit_depth: int) -> None:
        """ssimu2_set_reference_rgb16; later 8-bit and 16-bit frames can both be scored against it."""
        ref = _check_rgb16(ref, "ref")
        h, w, _ = ref.shape
        self._call(self._L.ssimu2_set_reference_rgb16, _u16p(ref), w, h, int(bit_depth))
        self._ref_shape = ref.shape

    def score_against_reference_hbd(self, dist, bit_depth: int) -> float:
        """ssimu2_score_against_reference_rgb16 against the reference of set_reference or set_reference_hbd."""
        dist = _check_rgb16(dist, "dist")
        self._check_ref_shape(dist.shape)
        return self._score(self._L.ssimu2_score_against_reference_rgb16, _u16p(dist), int(bit_depth))

    def score_decoded_against_reference_hbd(self, rows, row_bytes: int | None = None, channels: int | None = None,
                                            bit_depth: int = 16) -> float:
        """ssimu2_score_against_reference_strided16: libavif's avifRGBImage at depth > 8 as it is -- an (h, w, 3|4)
        uint16 array whose rows may be padded (pixels tightly packed within a row), or a flat uint16 buffer with
        explicit `row_bytes` / `channels`.  Alpha and padding are skipped on the device."""
        a = np.asarray(rows)
        if a.dtype != np.uint16:
            raise TypeError(f"rows must be uint16, got {a.dtype}")
        return self._score_decoded(self._L.ssimu2_score_against_reference_strided16, a, ctypes.c_uint16, row_bytes,
                                   channels, int(bit_depth))

    # -- RGBA input (include/ssimu2_hip_ext.h): the extension library only --------
    def _need_ext(self):
        if not self.extended:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "RGBA input needs Ssimu2(..., extended=True) (liboavif_hip_ext.so)")

    def composite_rgba(self, pixels, background) -> np.ndarray:
        """ssimu2_composite_rgba8: the (h, w, 3) uint16 codes n = a*c + (255 - a)*b of an (h, w, 4) uint8 frame with
        straight alpha over `background` ((r, g, b) or 0xRRGGBB): the frame as the scorer sees it."""
        self._need_ext()
        a, bg = _check_rgba8(pixels, "pixels"), background_rgb(background)
        h, w, _ = a.shape
        out = np.empty((h, w, 3), np.uint16)
        self._call(self._L.ssimu2_composite_rgba8, _u8p(a), a.strides[0] if h > 1 else 4 * w, w, h, bg, _u16p(out))
        return out

    def compute_ssimu2_rgba(self, ref, dist, background) -> float:
        """ssimu2_score_rgba8: two (h, w, 4) uint8 frames (rows may be padded), each composited over `background`."""
        self._need_ext()
        ref, dist = _check_pair(ref, dist, _check_rgba8)
        h, w, _ = ref.shape
        tight = 4 * w
        return self._score(self._L.ssimu2_score_rgba8, _u8p(ref), ref.strides[0] if h > 1 else tight, _u8p(dist),
                           dist.strides[0] if h > 1 else tight, w, h, background_rgb(background))

    def set_reference_rgba(self, ref, background) -> None:
        """ssimu2_set_reference_rgba8; later RGBA frames are composited over the same background, and 8-bit and 16-bit
        frames can be scored against it too."""
        self._need_ext()
        ref, bg = _check_rgba8(ref, "ref"), background_rgb(background)
        h, w, _ = ref.shape
        self._call(self._L.ssimu2_set_reference_rgba8, _u8p(ref), ref.strides[0] if h > 1 else 4 * w, w, h, bg)
        self._ref_shape = (h, w, 3)

    def score_against_reference_rgba(self, pixels, row_bytes: int | None = None) -> float:
        """ssimu2_score_against_reference_rgba8: an (h, w, 4) uint8 array or view (an avif_bridge.DecodedFrame's
        pixels()), or libavif's rows as they are -- its (h, rowBytes) `rows`, or a flat buffer with `row_bytes`."""
        self._need_ext()
        a = np.asarray(pixels)
        if a.dtype != np.uint8:
            raise TypeError(f"pixels must be uint8 RGBA, got {a.dtype}")
        if a.ndim == 3:
            a = _check_rgba8(a, "pixels")
            self._check_ref_shape(a.shape[:2], "frame size")
            row_bytes = (a.strides[0] if a.shape[0] > 1 else 4 * a.shape[1]) if row_bytes is None else row_bytes
        elif a.ndim == 2 and a.strides[1] == 1 and row_bytes is None:
            self._check_ref_shape(a.shape[:1], "frame height")
            row_bytes = a.strides[0]
        elif a.ndim != 1 or row_bytes is None or not a.flags.c_contiguous:
            raise ValueError("pixels must be (h, w, 4), libavif's (h, rowBytes) rows, or a flat buffer with row_bytes")
        return self._score(self._L.ssimu2_score_against_reference_rgba8, _u8p(a), int(row_bytes))

    # -- YUV input (include/ssimu2_hip_yuv.h): the YUV library only ---------------
    def _need_yuv(self):
        if not self.yuv:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "YUV input needs Ssimu2(..., yuv=True) (liboavif_hip_yuv.so)")

    @staticmethod
    def _yuv_frame(frame, name: str) -> YuvFrame:
        if not isinstance(frame, YuvFrame):
            raise TypeError(f"{name} must be a YuvFrame, got {type(frame).__name__}")
        return frame

    _CHROMA_UPSAMPLING = {"bilinear": _lib.CHROMA_BILINEAR, "nearest": _lib.CHROMA_NEAREST}

    def _chroma_args(self, chroma_upsampling, *frames) -> tuple:
        """What follows `rgb_depth` in a YUV call: nothing on a context of another library (which refuses a subsampled
        frame here, before any C call), the upsampling code on a chroma=True context, whose calls take it."""
        try:
            up = self._CHROMA_UPSAMPLING[chroma_upsampling]
        except (KeyError, TypeError):
            raise ValueError(f"chroma_upsampling must be 'bilinear' or 'nearest', got {chroma_upsampling!r}") from None
        if not self.chroma and any(f.subsampled for f in frames):
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "subsampled chroma (4:2:2 / 4:2:0) needs Ssimu2(..., chroma=True) "
                                                    "(liboavif_hip_chroma.so)")
        return (up,) if self.chroma else ()

    def _yuv_fn(self, name: str):
        """The C function of a YUV method: ssimu2_<name>, or on a chroma=True context ssimu2_<name>_chroma."""
        return getattr(self._L, f"ssimu2_{name}_chroma" if self.chroma else f"ssimu2_{name}")

    def convert_yuv(self, frame: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_convert_yuv: the (h, w, 3) uint16 RGB codes of depth `rgb_depth` the scorer makes of `frame`.
        `chroma_upsampling` ("bilinear" or "nearest", here and in the other YUV methods) is how a 4:2:2 or 4:2:0
        frame's chroma is upsampled (include/ssimu2_hip_chroma.h); a 4:4:4 or 4:0:0 frame does not depend on it."""
        f = self._yuv_frame(frame, "frame")
        up = self._chroma_args(chroma_upsampling, f)
        self._need_yuv()
        out = np.empty((f.height, f.width, 3), np.uint16)
        c = f.as_c()
        self._call(self._yuv_fn("convert_yuv"), ctypes.byref(c), f.width, f.height, int(rgb_depth), *up, _u16p(out))
        return out

    def compute_ssimu2_yuv(self, ref: YuvFrame, dist: YuvFrame, rgb_depth: int = 16,
                           chroma_upsampling: str = "bilinear") -> float:
        """ssimu2_score_yuv: two YUV frames of one size, each converted with its own format, depth, range and matrix."""
        r, d = self._yuv_frame(ref, "ref"), self._yuv_frame(dist, "dist")
        up = self._chroma_args(chroma_upsampling, r, d)
        self._need_yuv()
        if (r.height, r.width) != (d.height, d.width):
            raise ValueError("ref and dist must have the same shape")
        cr, cd = r.as_c(), d.as_c()
        return self._score(self._yuv_fn("score_yuv"), ctypes.byref(cr), ctypes.byref(cd), r.width, r.height, int(rgb_depth), *up)

    def set_reference_yuv(self, ref: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> None:
        """ssimu2_set_reference_yuv; later 8-bit, 16-bit and YUV frames can all be scored against it."""
        r = self._yuv_frame(ref, "ref")
        up = self._chroma_args(chroma_upsampling, r)
        self._need_yuv()
        c = r.as_c()
        self._call(self._yuv_fn("set_reference_yuv"), ctypes.byref(c), r.width, r.height, int(rgb_depth), *up)
        self._ref_shape = (r.height, r.width, 3)

    def score_against_reference_yuv(self, frame: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> float:
        """ssimu2_score_against_reference_yuv against the reference of any set_reference* call."""
        f = self._yuv_frame(frame, "frame")
        up = self._chroma_args(chroma_upsampling, f)
        self._need_yuv()
        self._check_ref_shape((f.height, f.width), "frame size")
        c = f.as_c()
        return self._score(self._yuv_fn("score_against_reference_yuv"), ctypes.byref(c), int(rgb_depth), *up)

    # -- error maps of 16-bit, RGBA and YUV frames (include/ssimu2_hip_map.h): the map library only
    def _need_maps(self):
        if not self.maps:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "error maps of 16-bit, RGBA and YUV frames need Ssimu2(..., maps=True) "
                                                    "(liboavif_hip_map.so)")

    def _map(self, fn, h: int, w: int, *args):
        """A call whose last two parameters are `float* out_map, double* out_score` -> (score, (h, w) float32 map)."""
        out = np.empty((h, w), np.float32)
        return self._score(fn, *args, _f32p(out)), out

    def error_map_hbd(self, ref, dist, bit_depth: int):
        """ssimu2_error_map_rgb16 -> (score, (h, w) float32 map) of two (h, w, 3) uint16 frames of `bit_depth` bits: the
        score bit for bit as compute_ssimu2_hbd, the map of DESIGN.md section 9 from the 16-bit pipeline's terms."""
        self._need_maps()
        ref, dist = _check_pair(ref, dist, _check_rgb16)
        h, w, _ = ref.shape
        return self._map(self._L.ssimu2_error_map_rgb16, h, w, _u16p(ref), _u16p(dist), w, h, int(bit_depth))

    def error_map_against_reference_hbd(self, dist, bit_depth: int):
        """ssimu2_error_map_against_reference_rgb16 -> (score, map) against the reference of any set_reference* call."""
        self._need_maps()
        dist = _check_rgb16(dist, "dist")
        self._check_ref_shape(dist.shape)
        h, w, _ = dist.shape
        return self._map(self._L.ssimu2_error_map_against_reference_rgb16, h, w, _u16p(dist), int(bit_depth))

    def error_map_rgba(self, ref, dist, background):
        """ssimu2_error_map_rgba8 -> (score, map) of two (h, w, 4) uint8 frames (rows may be padded), each composited
        over `background`."""
        self._need_maps()
        ref, dist = _check_pair(ref, dist, _check_rgba8)
        h, w, _ = ref.shape
        tight = 4 * w
        return self._map(self._L.ssimu2_error_map_rgba8, h, w, _u8p(ref), ref.strides[0] if h > 1 else tight, _u8p(dist),
                         dist.strides[0] if h > 1 else tight, w, h, background_rgb(background))

    def error_map_against_reference_rgba(self, pixels, row_bytes: int | None = None):
        """ssimu2_error_map_against_reference_rgba8 -> (score, map): an (h, w, 4) uint8 array or view whose rows are
        `row_bytes` apart (None: its own stride) against the reference of set_reference_rgba, over its background."""
        self._need_maps()
        a = np.asarray(pixels)
        if a.dtype != np.uint8:
            raise TypeError(f"pixels must be uint8 RGBA, got {a.dtype}")
        a = _check_rgba8(a, "pixels")
        self._check_ref_shape(a.shape[:2], "frame size")
        h, w, _ = a.shape
        row_bytes = (a.strides[0] if h > 1 else 4 * w) if row_bytes is None else row_bytes
        return self._map(self._L.ssimu2_error_map_against_reference_rgba8, h, w, _u8p(a), int(row_bytes))

    def error_map_yuv(self, ref: YuvFrame, dist: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear"):
        """ssimu2_error_map_yuv -> (score, map) of two YUV frames of one size, converted to codes of `rgb_depth` bits."""
        r, d = self._yuv_frame(ref, "ref"), self._yuv_frame(dist, "dist")
        up = self._chroma_args(chroma_upsampling, r, d)
        self._need_maps()
        if (r.height, r.width) != (d.height, d.width):
            raise ValueError("ref and dist must have the same shape")
        cr, cd = r.as_c(), d.as_c()
        return self._map(self._yuv_fn("error_map_yuv"), r.height, r.width, ctypes.byref(cr), ctypes.byref(cd), r.width,
                         r.height, int(rgb_depth), *up)

    def error_map_against_reference_yuv(self, frame: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear"):
        """ssimu2_error_map_against_reference_yuv -> (score, map) against the reference of any set_reference* call."""
        f = self._yuv_frame(frame, "frame")
        up = self._chroma_args(chroma_upsampling, f)
        self._need_maps()
        self._check_ref_shape((f.height, f.width), "frame size")
        c = f.as_c()
        return self._map(self._yuv_fn("error_map_against_reference_yuv"), f.height, f.width, ctypes.byref(c), int(rgb_depth), *up)

    # -- YUV frames with an alpha plane (include/ssimu2_hip_yuva.h): the yuva library only --------
    def _yuva_args(self, chroma_upsampling, *frames) -> int:
        """The refusal of a context of another library, then the upsampling code."""
        if not self.yuva:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "YUV frames with an alpha plane need Ssimu2(..., yuva=True) "
                                                    "(liboavif_hip_yuva.so)")
        for k, f in enumerate(frames):
            self._yuv_frame(f, "frame" if len(frames) == 1 else ("ref", "dist")[k])
        try:
            return self._CHROMA_UPSAMPLING[chroma_upsampling]
        except (KeyError, TypeError):
            raise ValueError(f"chroma_upsampling must be 'bilinear' or 'nearest', got {chroma_upsampling!r}") from None

    def composite_yuva(self, frame: YuvFrame, background, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_composite_yuva: the (h, w, 3) uint16 composite codes n (0..65025) of `frame` -- its colour codes of
        depth `rgb_depth` under its alpha plane over `background` ((r, g, b) or 0xRRGGBB): the frame as the scorer sees it."""
        up = self._yuva_args(chroma_upsampling, frame)
        bg = background_rgb(background)
        out = np.empty((frame.height, frame.width, 3), np.uint16)
        c = frame.as_yuva_c()
        self._call(self._L.ssimu2_composite_yuva, ctypes.byref(c), frame.width, frame.height, int(rgb_depth), up, bg, _u16p(out))
        return out

    def compute_ssimu2_yuva(self, ref: YuvFrame, dist: YuvFrame, background, rgb_depth: int = 16,
                            chroma_upsampling: str = "bilinear") -> float:
        """ssimu2_score_yuva: two frames of one size, each with its own format, depth and alpha plane, both composited
        over `background`."""
        up = self._yuva_args(chroma_upsampling, ref, dist)
        if (ref.height, ref.width) != (dist.height, dist.width):
            raise ValueError("ref and dist must have the same shape")
        cr, cd = ref.as_yuva_c(), dist.as_yuva_c()
        return self._score(self._L.ssimu2_score_yuva, ctypes.byref(cr), ctypes.byref(cd), ref.width, ref.height,
                           int(rgb_depth), up, background_rgb(background))

    def set_reference_yuva(self, ref: YuvFrame, background, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> None:
        """ssimu2_set_reference_yuva; later frames with an alpha plane (and RGBA frames) are composited over the same
        background."""
        up = self._yuva_args(chroma_upsampling, ref)
        c = ref.as_yuva_c()
        self._call(self._L.ssimu2_set_reference_yuva, ctypes.byref(c), ref.width, ref.height, int(rgb_depth), up,
                   background_rgb(background))
        self._ref_shape = (ref.height, ref.width, 3)

    def score_against_reference_yuva(self, frame: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> float:
        """ssimu2_score_against_reference_yuva against the reference of set_reference_yuva or set_reference_rgba, over
        its background."""
        up = self._yuva_args(chroma_upsampling, frame)
        self._check_ref_shape((frame.height, frame.width), "frame size")
        c = frame.as_yuva_c()
        return self._score(self._L.ssimu2_score_against_reference_yuva, ctypes.byref(c), int(rgb_depth), up)

    def error_map_yuva_alpha(self, ref: YuvFrame, dist: YuvFrame, background, rgb_depth: int = 16,
                             chroma_upsampling: str = "bilinear"):
        """ssimu2_error_map_yuva -> (score, map) of two frames with alpha planes, both composited over `background`."""
        up = self._yuva_args(chroma_upsampling, ref, dist)
        if (ref.height, ref.width) != (dist.height, dist.width):
            raise ValueError("ref and dist must have the same shape")
        cr, cd = ref.as_yuva_c(), dist.as_yuva_c()
        return self._map(self._L.ssimu2_error_map_yuva, ref.height, ref.width, ctypes.byref(cr), ctypes.byref(cd), ref.width,
                         ref.height, int(rgb_depth), up, background_rgb(background))

    def error_map_against_reference_yuva_alpha(self, frame: YuvFrame, rgb_depth: int = 16, chroma_upsampling: str = "bilinear"):
        """ssimu2_error_map_against_reference_yuva -> (score, map) against the reference, over its background."""
        up = self._yuva_args(chroma_upsampling, frame)
        self._check_ref_shape((frame.height, frame.width), "frame size")
        c = frame.as_yuva_c()
        return self._map(self._L.ssimu2_error_map_against_reference_yuva, frame.height, frame.width, ctypes.byref(c),
                         int(rgb_depth), up)

    # -- device-resident entry points (pointers are raw device addresses) -------------------
    # The per-frame ones make their C call in their own body, not through _call / _score / _scores: a 512x512 score is
    # bound by its 29 us of host time, and the helper's extra Python frame is 0.15 to 0.3 % of its rate, measured.
    def score_device(self, d_ref: int, d_dist: int, w: int, h: int) -> float:
        out = ctypes.c_double()
        rc = self._L.ssimu2_score_rgb8_device(self._ctx, ctypes.c_void_p(d_ref), ctypes.c_void_p(d_dist), w, h,
                                              ctypes.byref(out))
        if rc != 0:
            self._raise(rc)
        return out.value

    def enqueue_device(self, d_ref: int, d_dist: int, w: int, h: int) -> None:
        rc = self._L.ssimu2_enqueue_rgb8_device(self._ctx, ctypes.c_void_p(d_ref), ctypes.c_void_p(d_dist), w, h)
        if rc != 0:
            self._raise(rc)

    def set_reference_device(self, d_ref: int, w: int, h: int) -> None:
        self._call(self._L.ssimu2_set_reference_device, ctypes.c_void_p(d_ref), w, h)
        self._ref_shape = (h, w, 3)

    def enqueue_against_reference_device(self, d_dist: int) -> None:
        rc = self._L.ssimu2_enqueue_against_reference_device(self._ctx, ctypes.c_void_p(d_dist))
        if rc != 0:
            self._raise(rc)

    def wait(self) -> float:
        out = ctypes.c_double()
        rc = self._L.ssimu2_wait(self._ctx, ctypes.byref(out))
        if rc != 0:
            self._raise(rc)
        return out.value

    # -- batch scoring (include/ssimu2_hip.h "Batch scoring") -----------------
    @staticmethod
    def _check_batch(frames, name: str):
        """[N, h, w, 3] uint8 or a sequence of (h, w, 3) uint8 -> list of contiguous frames of one size."""
        out = [_check_rgb8(f, f"{name}[{i}]") for i, f in enumerate(frames)]
        if any(f.shape != out[0].shape for f in out):
            raise ValueError(f"{name}: the frames of a batch must have one size")
        return out

    @staticmethod
    def _ptr_array(frames):
        return (ctypes.POINTER(ctypes.c_uint8) * len(frames))(*[_u8p(f) for f in frames])

    def _batch_fn(self, name: str):
        """The batch call `name` of include/ssimu2_hip.h, or on an rbatch=True context its counterpart of
        include/ssimu2_hip_rbatch.h (the same parameters; every blur mode)."""
        return getattr(self._L, _RBATCH_CALLS[name] if self.rbatch else name)

    def score_batch(self, refs, dists) -> np.ndarray:
        """ssimu2_score_batch_rgb8: N pairs of one size in one launch set -> float64 scores in input order.
        A cached reference is kept.  FIR only, unless the context was made with rbatch=True (_batch_fn); so are the
        three methods below."""
        refs, dists = self._check_batch(refs, "refs"), self._check_batch(dists, "dists")
        if len(refs) != len(dists):
            raise ValueError("refs and dists must hold the same number of frames")
        if not refs:
            return np.zeros(0, np.float64)
        if refs[0].shape != dists[0].shape:
            raise ValueError("refs and dists must have the same shape")
        h, w, _ = refs[0].shape
        return self._scores(self._batch_fn("ssimu2_score_batch_rgb8"), len(refs), self._ptr_array(refs), self._ptr_array(dists),
                            len(refs), w, h)

    def score_batch_against_reference(self, dists) -> np.ndarray:
        """ssimu2_score_batch_against_reference: N distorted frames against the cached reference (kept)."""
        dists = self._check_batch(dists, "dists")
        if not dists:
            return np.zeros(0, np.float64)
        self._check_ref_shape(dists[0].shape)
        return self._scores(self._batch_fn("ssimu2_score_batch_against_reference"), len(dists), self._ptr_array(dists), len(dists))

    def score_batch_device(self, d_refs: int, d_dists: int, item_stride_bytes: int, n: int, w: int, h: int) -> np.ndarray:
        """ssimu2_score_batch_rgb8_device: item i at d_refs + i * item_stride_bytes / d_dists + i * item_stride_bytes."""
        out = np.zeros(int(n), np.float64)   # in its own body: see "device-resident entry points"
        rc = self._batch_fn("ssimu2_score_batch_rgb8_device")(self._ctx, ctypes.c_void_p(d_refs), ctypes.c_void_p(d_dists),
                                                              int(item_stride_bytes), int(n), w, h, out.ctypes.data_as(_F64P))
        if rc != 0:
            self._raise(rc)
        return out

    def score_batch_against_reference_device(self, d_dists: int, item_stride_bytes: int, n: int) -> np.ndarray:
        """ssimu2_score_batch_against_reference_device against the reference of set_reference / set_reference_device."""
        out = np.zeros(int(n), np.float64)
        rc = self._batch_fn("ssimu2_score_batch_against_reference_device")(self._ctx, ctypes.c_void_p(d_dists), int(item_stride_bytes),
                                                                           int(n), out.ctypes.data_as(_F64P))
        if rc != 0:
            self._raise(rc)
        return out

    # -- batches of 16-bit and YUV frames (include/ssimu2_hip_hbatch.h): the hbatch library only --
    def _need_hbatch(self):
        if not self.hbatch:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "batches of 16-bit and YUV frames need Ssimu2(..., hbatch=True) "
                                                    "(liboavif_hip_hbatch.so)")

    @staticmethod
    def _check_batch16(frames, name: str):
        """[N, h, w, 3] uint16 or a sequence of (h, w, 3) uint16 -> list of contiguous frames of one size."""
        out = [_check_rgb16(f, f"{name}[{i}]") for i, f in enumerate(frames)]
        if any(f.shape != out[0].shape for f in out):
            raise ValueError(f"{name}: the frames of a batch must have one size")
        return out

    @staticmethod
    def _ptr_array16(frames):
        return (ctypes.POINTER(ctypes.c_uint16) * len(frames))(*[_u16p(f) for f in frames])

    def score_batch_hbd(self, refs, dists, bit_depth: int) -> np.ndarray:
        """ssimu2_hbatch_score_rgb16: N pairs of (h, w, 3) uint16 frames of `bit_depth` bits and one size in one launch
        set -> float64 scores in input order, each with the bits of compute_ssimu2_hbd.  Recursive blur modes only.
        A cached reference is kept."""
        self._need_hbatch()
        refs, dists = self._check_batch16(refs, "refs"), self._check_batch16(dists, "dists")
        if len(refs) != len(dists):
            raise ValueError("refs and dists must hold the same number of frames")
        if not refs:
            return np.zeros(0, np.float64)
        if refs[0].shape != dists[0].shape:
            raise ValueError("refs and dists must have the same shape")
        h, w, _ = refs[0].shape
        return self._scores(self._L.ssimu2_hbatch_score_rgb16, len(refs), self._ptr_array16(refs), self._ptr_array16(dists),
                            len(refs), w, h, int(bit_depth))

    def score_batch_against_reference_hbd(self, dists, bit_depth: int) -> np.ndarray:
        """ssimu2_hbatch_score_against_reference_rgb16: N uint16 frames against the cached reference (kept), each with
        the bits of score_against_reference_hbd."""
        self._need_hbatch()
        dists = self._check_batch16(dists, "dists")
        if not dists:
            return np.zeros(0, np.float64)
        self._check_ref_shape(dists[0].shape)
        return self._scores(self._L.ssimu2_hbatch_score_against_reference_rgb16, len(dists), self._ptr_array16(dists),
                            len(dists), int(bit_depth))

    def score_batch_hbd_device(self, d_refs: int, d_dists: int, item_stride_bytes: int, n: int, w: int, h: int,
                               bit_depth: int) -> np.ndarray:
        """ssimu2_hbatch_score_rgb16_device: item i at d_refs + i * item_stride_bytes / d_dists + i * item_stride_bytes
        (tight uint16 frames; the stride even, any multiple of 2)."""
        self._need_hbatch()
        return self._scores(self._L.ssimu2_hbatch_score_rgb16_device, n, ctypes.c_void_p(d_refs), ctypes.c_void_p(d_dists),
                            int(item_stride_bytes), int(n), int(w), int(h), int(bit_depth))

    def score_batch_against_reference_hbd_device(self, d_dists: int, item_stride_bytes: int, n: int, bit_depth: int) -> np.ndarray:
        """ssimu2_hbatch_score_against_reference_rgb16_device against the cached reference."""
        self._need_hbatch()
        return self._scores(self._L.ssimu2_hbatch_score_against_reference_rgb16_device, n, ctypes.c_void_p(d_dists),
                            int(item_stride_bytes), int(n), int(bit_depth))

    def _yuv_batch(self, frames, chroma_upsampling):
        """-> (the frames, their C array, the upsampling code) of a YUV batch: YuvFrames of one size, none with an alpha
        plane (refused: the C struct of a batch has no room for one, and dropping it would score another image)."""
        self._need_hbatch()
        frames = [self._yuv_frame(f, f"frames[{i}]") for i, f in enumerate(frames)]
        for i, f in enumerate(frames):
            if f.alpha is not None:
                raise ValueError(f"frames[{i}] carries an alpha plane, which a YUV batch does not composite: score it "
                                 "with score_against_reference_yuva")
        up, = self._chroma_args(chroma_upsampling, *frames)
        if any((f.height, f.width) != (frames[0].height, frames[0].width) for f in frames):
            raise ValueError("frames: the frames of a batch must have one size")
        arr = (_lib.YuvFrameC * max(len(frames), 1))(*[f.as_c() for f in frames])
        return frames, arr, up

    def score_batch_against_reference_yuv(self, frames, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_hbatch_score_against_reference_yuv: N YuvFrames of one size, depth, format, range and matrix (no alpha
        plane) against the cached reference (kept), each with the bits of score_against_reference_yuv."""
        frames, arr, up = self._yuv_batch(frames, chroma_upsampling)
        if not frames:
            return np.zeros(0, np.float64)
        self._check_ref_shape((frames[0].height, frames[0].width), "frame size")
        return self._scores(self._L.ssimu2_hbatch_score_against_reference_yuv, len(frames), arr, len(frames), int(rgb_depth), up)

    def convert_yuv_batch(self, frames, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_hbatch_convert_yuv: the (n, h, w, 3) uint16 codes the scorer makes of the N frames of a YUV batch, item
        i with the bits of convert_yuv(frames[i])."""
        frames, arr, up = self._yuv_batch(frames, chroma_upsampling)
        if not frames:
            return np.zeros((0, 0, 0, 3), np.uint16)
        h, w = frames[0].height, frames[0].width
        out = np.empty((len(frames), h, w, 3), np.uint16)
        self._call(self._L.ssimu2_hbatch_convert_yuv, arr, len(frames), w, h, int(rgb_depth), up, _u16p(out))
        return out

    # -- batches of RGBA and YUV-with-alpha frames (include/ssimu2_hip_abatch.h): the abatch library only --
    def _need_abatch(self):
        if not self.abatch:
            raise Ssimu2Error(_lib.ERR_UNSUPPORTED, "batches of RGBA and YUV-with-alpha frames need Ssimu2(..., abatch=True) "
                                                    "(liboavif_hip_abatch.so)")

    def _yuva_batch(self, frames, chroma_upsampling):
        """-> (the frames, their C array, the upsampling code) of a YUVA batch: YuvFrames of one size, with or without
        an alpha plane (the library refuses a batch that mixes the two)."""
        self._need_abatch()
        frames = [self._yuv_frame(f, f"frames[{i}]") for i, f in enumerate(frames)]
        up = self._yuva_args(chroma_upsampling)
        if any((f.height, f.width) != (frames[0].height, frames[0].width) for f in frames):
            raise ValueError("frames: the frames of a batch must have one size")
        arr = (_lib.YuvaFrameC * max(len(frames), 1))(*[f.as_yuva_c() for f in frames])
        return frames, arr, up

    def score_batch_against_reference_yuva(self, frames, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_abatch_score_against_reference_yuva: N YuvFrames of one size, depth, format, range and matrix, all with
        or all without an alpha plane, each composited over the reference's background and scored against the cached
        reference (kept), each with the bits of score_against_reference_yuva.  Recursive blur modes only."""
        frames, arr, up = self._yuva_batch(frames, chroma_upsampling)
        if not frames:
            return np.zeros(0, np.float64)
        self._check_ref_shape((frames[0].height, frames[0].width), "frame size")
        return self._scores(self._L.ssimu2_abatch_score_against_reference_yuva, len(frames), arr, len(frames), int(rgb_depth), up)

    def composite_yuva_batch(self, frames, background, rgb_depth: int = 16, chroma_upsampling: str = "bilinear") -> np.ndarray:
        """ssimu2_abatch_composite_yuva: the (n, h, w, 3) uint16 composite codes of the N frames of a YUVA batch over
        `background`, item i with the bits of composite_yuva(frames[i], background)."""
        frames, arr, up = self._yuva_batch(frames, chroma_upsampling)
        bg = background_rgb(background)
        if not frames:
            return np.zeros((0, 0, 0, 3), np.uint16)
        h, w = frames[0].height, frames[0].width
        out = np.empty((len(frames), h, w, 3), np.uint16)
        self._call(self._L.ssimu2_abatch_composite_yuva, arr, len(frames), w, h, int(rgb_depth), up, bg, _u16p(out))
        return out

    @staticmethod
    def _rgba_batch(frames, name: str):
        """[N, h, w, 4] uint8 or a sequence of (h, w, 4) uint8 frames or views of one size -> (the frames, their pointer
        array, the one row_bytes of all).  Views whose rows lie one distance apart go through as they are; if the
        distances differ every frame is made tight."""
        out = [_check_rgba8(f, f"{name}[{i}]") for i, f in enumerate(frames)]
        if any(f.shape != out[0].shape for f in out):
            raise ValueError(f"{name}: the frames of a batch must have one size")
        if not out:
            return out, None, 0
        h, w, _ = out[0].shape
        pitches = {f.strides[0] if h > 1 else 4 * w for f in out}
        if len(pitches) > 1:
            out = [np.ascontiguousarray(f) for f in out]
            pitches = {4 * w}
        return out, (ctypes.POINTER(ctypes.c_uint8) * len(out))(*[_u8p(f) for f in out]), pitches.pop()

    def score_batch_against_reference_rgba(self, frames) -> np.ndarray:
        """ssimu2_abatch_score_against_reference_rgba8: N (h, w, 4) uint8 frames (rows may be padded), each composited
        over the reference's background and scored against the cached reference (kept), each with the bits of
        score_against_reference_rgba.  Recursive blur modes only."""
        self._need_abatch()
        frames, arr, row_bytes = self._rgba_batch(frames, "frames")
        if not frames:
            return np.zeros(0, np.float64)
        self._check_ref_shape(frames[0].shape[:2], "frame size")
        return self._scores(self._L.ssimu2_abatch_score_against_reference_rgba8, len(frames), arr, row_bytes, len(frames))

    def score_batch_rgba(self, refs, dists, background) -> np.ndarray:
        """ssimu2_abatch_score_rgba8: N pairs of (h, w, 4) uint8 frames of one size, both sides composited over
        `background`, each with the bits of compute_ssimu2_rgba.  Recursive blur modes only."""
        self._need_abatch()
        refs, rarr, rrow = self._rgba_batch(refs, "refs")
        dists, darr, drow = self._rgba_batch(dists, "dists")
        bg = background_rgb(background)
        if len(refs) != len(dists):
            raise ValueError("refs and dists must hold the same number of frames")
        if not refs:
            return np.zeros(0, np.float64)
        if refs[0].shape != dists[0].shape:
            raise ValueError("refs and dists must have the same shape")
        h, w, _ = refs[0].shape
        return self._scores(self._L.ssimu2_abatch_score_rgba8, len(refs), rarr, rrow, darr, drow, len(refs), w, h, bg)

    def composite_rgba_batch(self, frames, background) -> np.ndarray:
        """ssimu2_abatch_composite_rgba8: the (n, h, w, 3) uint16 composite codes of N RGBA frames over `background`, item
        i with the bits of composite_rgba(frames[i], background)."""
        self._need_abatch()
        frames, arr, row_bytes = self._rgba_batch(frames, "frames")
        bg = background_rgb(background)
        if not frames:
            return np.zeros((0, 0, 0, 3), np.uint16)
        h, w, _ = frames[0].shape
        out = np.empty((len(frames), h, w, 3), np.uint16)
        self._call(self._L.ssimu2_abatch_composite_rgba8, arr, row_bytes, len(frames), w, h, bg, _u16p(out))
        return out

    def last_batch_averages(self, item: int):
        """-> ((6, 18) float64 plane averages of `item` of the last batch, number of scales)."""
        return self._averages(self._L.ssimu2_last_batch_averages, int(item))

    def last_averages(self):
        """-> ((6, 18) float64 plane averages of the last score, number of scales)."""
        return self._averages(self._L.ssimu2_last_averages)

    def set_blur(self, mode: int) -> None:
        """ssimu2_ctx_set_blur: _lib.BLUR_FIR (default, the fused 9-tap kernels) or
        _lib.BLUR_RECURSIVE (the published recursion, operation for operation: 0.4 ms per 4K pass
        against a cached reference where the default takes 0.16)."""
        self._call(self._L.ssimu2_ctx_set_blur, int(mode))

    # -- measurement / parity hooks: instrumented build only ------------------------------------
    def set_batch_segment_rows(self, rows_scale0: int) -> None:
        """Instrumented build: scale-0 rows of a batch item (0 = the rule, -1 = the single-score rule, 8..160)."""
        self._need_instr()
        self._call(self._L.ssimu2_instr_set_batch_segment_rows, int(rows_scale0))

    def batch_segment_rows(self, w: int, h: int, scale: int) -> int:
        """Instrumented build: rows per workgroup a batch item of w x h gets at `scale` (ssimu2_instr_batch_segment_rows)."""
        self._need_instr()
        rows = ctypes.c_int()
        self._call(self._L.ssimu2_instr_batch_segment_rows, int(w), int(h), int(scale), ctypes.byref(rows))
        return int(rows.value)

    def time_device(self, d_ref: int, d_dist: int, w: int, h: int, iters: int):
        """-> (total device ms for `iters` back-to-back scores, score)."""
        self._need_instr()
        ms, out = ctypes.c_float(), ctypes.c_double()
        self._call(self._L.ssimu2_time_device, ctypes.c_void_p(d_ref), ctypes.c_void_p(d_dist), w, h, iters,
                    ctypes.byref(ms), ctypes.byref(out))
        return ms.value, out.value

    def time_stage(self, d_ref: int, d_dist: int, w: int, h: int, stage: int, iters: int) -> float:
        """-> average device ms of one execution of `stage` (_lib.STAGE_*) of the score."""
        self._need_instr()
        ms = ctypes.c_float()
        self._call(self._L.ssimu2_time_stage, ctypes.c_void_p(d_ref), ctypes.c_void_p(d_dist), w, h, stage, iters,
                    ctypes.byref(ms))
        return ms.value

    def measure_read_stream(self, nbytes: int = 2 << 30, iters: int = 10) -> float:
        """-> measured HBM read-stream bandwidth of the device in GB/s (ssimu2_measure_read_stream)."""
        self._need_instr()
        out = ctypes.c_double()
        self._call(self._L.ssimu2_measure_read_stream, ctypes.c_size_t(nbytes), iters, ctypes.byref(out))
        return out.value

    def placed_streams(self) -> int:
        """Instrumented build: streams on distinct hardware queues its library instance holds for this
        context's device (ssimu2_instr_placed_streams)."""
        n = ctypes.c_int(0)
        self._icall("ssimu2_instr_placed_streams", ctypes.byref(n))
        return int(n.value)

    def rg_stop_after_scale(self, scale: int) -> None:
        """Instrumented build: the recursive mode keeps the 15 raw planes of `scale` (after the
        horizontal pass and after both passes) downloadable (debug_download what = 4 / 5);
        negative = keep nothing.  (The name is round 2's, when the run stopped after that scale.)"""
        self._need_instr()
        self._call(self._L.ssimu2_instr_rg_stop_after_scale, int(scale))

    def debug_download(self, what: int, scale: int, w: int, h: int) -> np.ndarray:
        """-> (3, h_s, w_s) float32 planes; (15, h_s, w_s) for what = 4 / 5 (see ssimu2_debug_download)."""
        self._need_instr()
        sw, sh = w, h
        for _ in range(scale):
            sw, sh = (sw + 1) // 2, (sh + 1) // 2
        out = np.empty((15 if what in (4, 5) else 3, sh, sw), np.float32)
        ow, oh = ctypes.c_uint32(), ctypes.c_uint32()
        self._call(self._L.ssimu2_debug_download, what, scale, w, h, _f32p(out), ctypes.byref(ow), ctypes.byref(oh))
        assert (ow.value, oh.value) == (sw, sh)
        return out

    def time_march_rotating(self, d_refs, d_dists, w: int, h: int, iters: int) -> float:
        """-> average device ms of the marching kernel over `iters` launches that rotate over the
        device-resident pairs (d_refs[i], d_dists[i]) -- inputs from HBM, not from the Infinity Cache."""
        self._need_instr()
        n = len(d_refs)
        assert n == len(d_dists) and n > 0
        arr = ctypes.c_void_p * n
        ms = ctypes.c_float()
        self._call(self._L.ssimu2_time_march_rotating, arr(*d_refs), arr(*d_dists), n, w, h, iters, ctypes.byref(ms))
        return ms.value

    def time_blur_stage_rotating(self, d_frames, w: int, h: int, iters: int):
        """-> (average device ms, algorithmic bytes per launch) of k_ref_blur -- the marching body as a
        plain blur stage: XYB planes of one frame in, one blurred plane per channel out -- over
        `iters` launches rotating over the plane sets of the device-resident frames (HBM-fed)."""
        self._need_instr()
        n = len(d_frames)
        ms, nbytes = ctypes.c_float(), ctypes.c_double()
        self._call(self._L.ssimu2_time_blur_stage_rotating, (ctypes.c_void_p * n)(*d_frames), n, w, h, iters,
                    ctypes.byref(ms), ctypes.byref(nbytes))
        return ms.value, nbytes.value

    KERNEL_NAMES = {(False, True): ("pyramid", "march_refblur", "finalize"), (False, False): ("pyramid", "march", "finalize"),
                    (True, True): ("convert", "h", "v", "finalize"),
                    (True, False): ("ref_convert", "ref_h", "ref_v_emit", "convert", "h", "v", "finalize")}

    def time_kernels(self, w: int, h: int, d_dists, iters: int, d_ref: int | None = None, d_refs=None, recursive: bool = False):
        """ssimu2_time_kernels (instrumented build): every kernel of a score timed where it runs, from its own dispatch packet.
        `d_ref` = reference-cached passes over the distorted frames `d_dists`; `d_refs` = pair scores of (d_refs[i], d_dists[i]).
        -> ({launch name: average device ms}, stream ms per score with the timestamps, stream ms per score without).
        `recursive` names the launches only (the context's blur mode decides what runs)."""
        self._need_instr()
        n = len(d_dists)
        arr = ctypes.c_void_p * n
        ms = (ctypes.c_float * 8)()
        nl = ctypes.c_int()
        wt, wp = ctypes.c_float(), ctypes.c_float()
        self._call(self._L.ssimu2_time_kernels, ctypes.c_void_p(d_ref or 0), arr(*d_refs) if d_refs is not None else None,
                    arr(*d_dists), n, w, h, iters, ms, ctypes.byref(nl), ctypes.byref(wt), ctypes.byref(wp))
        if d_refs is None:
            self._ref_shape = (h, w, 3)
        names = self.KERNEL_NAMES[(bool(recursive), d_refs is None)]
        if nl.value != len(names):   # e.g. a frame with one scale has no pyramid launch
            names = tuple(f"launch{k}" for k in range(nl.value))
        return dict(zip(names, (float(ms[k]) for k in range(nl.value)))), float(wt.value), float(wp.value)

    def set_segment_rows(self, rows_scale0: int, rows_other_scales: int) -> None:
        self._icall("ssimu2_instr_set_segment_rows", rows_scale0, rows_other_scales)

    def cache_reference_blur(self, enabled: bool) -> None:
        self._icall("ssimu2_instr_cache_reference_blur", 1 if enabled else 0)

    MARCH_KERNELS = (None, "k_march", "k_march_refblur", "k_march_lin", "k_march_refblur_lin", "k_march_batch",
                     "k_march_refblur_batch")

    def last_march(self):
        """Instrumented build: the marching kernel the last score or batch launched (ssimu2_instr_last_march), by name;
        None when it launched none (a frame below 8 x 8)."""
        kind = ctypes.c_int()
        self._icall("ssimu2_instr_last_march", ctypes.byref(kind))
        return self.MARCH_KERNELS[kind.value]


def score_many(scorers, d_ref: int, d_dists, w: int, h: int):
    """Score several distorted frames against one reference, fanned over `scorers`
    (independent contexts = independent HIP streams on one or more GPUs).  All pointers are
    device addresses valid on each scorer's device.  Returns the scores in input order; each is
    bit-identical to scoring that frame alone (a context never shares state with another).

    This is the mechanism for speculative quantizer probes: the decoded frames
    of several candidate quantizers are scored concurrently, then tq replays its sequential
    decision logic over the cached scores.
    """
    out = [None] * len(d_dists)
    n = len(scorers)
    for base in range(0, len(d_dists), n):
        batch = list(range(base, min(base + n, len(d_dists))))
        for j, i in enumerate(batch):
            scorers[j].enqueue_device(d_ref, d_dists[i], w, h)
        for j, i in enumerate(batch):
            out[i] = scorers[j].wait()
    return out


def version() -> str:
    return _lib.lib().ssimu2_version().decode()
