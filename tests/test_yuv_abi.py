"""The YUV library without a GPU (include/ssimu2_hip_yuv.h): the header against the binding table
and the struct's layout, the library's exports (the public ABI, the five RGBA entry points, the four YUV ones and nothing
else), what every new call answers to a null context, no CPU fallback, the refusals the Python side makes before any C
call, and the command lines of oavif_amd.yuvscore and --score-yuv."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import _declared_functions, _exported
from test_binding_signatures import ROOT, check, prototypes

YUV_HEADER = "ssimu2_hip_yuv.h"
YUV_NAMES = ["ssimu2_convert_yuv", "ssimu2_score_yuv", "ssimu2_set_reference_yuv", "ssimu2_score_against_reference_yuv"]


@pytest.fixture(scope="module")
def yuv_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.yuv_lib()


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.YUV_FUNCTIONS) == YUV_NAMES                         # header order
    assert _lib.YUV_SYMBOLS == tuple(_lib.YUV_FUNCTIONS)
    assert set(_declared_functions(YUV_HEADER)) == set(_lib.YUV_FUNCTIONS)
    assert list(prototypes(YUV_HEADER)) == YUV_NAMES
    assert not set(_lib.YUV_FUNCTIONS) & (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS))


@pytest.mark.parametrize("name", YUV_NAMES)
def test_signature_matches_the_header(name):
    """test_binding_signatures.check holds the count and the class of every argument; it knows no ssimu2_yuv_frame, so
    the struct pointers are held here: every `const ssimu2_yuv_frame*` parameter is a POINTER(YuvFrameC), nothing else is."""
    from oavif_amd import _lib
    restype, argtypes = _lib.YUV_FUNCTIONS[name]
    ret, params = prototypes(YUV_HEADER)[name]
    check(name, (ret, params), restype, argtypes)
    for decl, ctype in zip(params, argtypes):
        is_frame = re.match(r"const\s+ssimu2_yuv_frame\s*\*", decl) is not None
        assert (ctype is ctypes.POINTER(_lib.YuvFrameC)) == is_frame, (name, decl, ctype)
    assert sum("ssimu2_yuv_frame" in d for d in params) == (2 if name == "ssimu2_score_yuv" else 1)


def test_struct_layout_is_the_headers(tmp_path):
    """sizeof and every offsetof of ssimu2_yuv_frame, as a C compiler sees the header, against the ctypes structure."""
    from oavif_amd import _lib
    fields = [name for name, _t in _lib.YuvFrameC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ssimu2_hip_yuv.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ssimu2_yuv_frame));\n'
                   + "".join(f'    printf(" %zu", offsetof(ssimu2_yuv_frame, {f}));\n' for f in fields)
                   + '    printf(" %d %d\\n", SSIMU2_YUV_444, SSIMU2_YUV_400);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.YuvFrameC)] + [getattr(_lib.YuvFrameC, f).offset for f in fields] + [_lib.YUV_444, _lib.YUV_400]
    assert got == want == [56, 0, 24, 36, 40, 44, 48, 1, 4]


def test_yuv_library_exports_the_public_abi_the_rgba_calls_and_the_yuv_calls(yuv_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS)
    got = {s for s in _exported(_lib.YUV_LIB_PATH) if s.startswith(("ssimu2_", "oavif_"))}
    assert got == want, got ^ want
    plain = {s for s in _exported(_lib.YUV_LIB_PATH) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}
    assert plain == want, plain ^ want
    for name in want:
        assert hasattr(yuv_lib, name), name


def test_the_other_libraries_have_none_of_it(hip_lib):
    from oavif_amd import _lib
    for path in (_lib.LIB_PATH, _lib.INSTR_LIB_PATH, _lib.EXT_LIB_PATH):
        assert not set(_exported(path)) & set(_lib.YUV_SYMBOLS), path


def test_build_knows_the_fourth_library(hip_lib):
    from oavif_amd import _lib, build
    assert os.path.samefile(os.path.dirname(build.YUV_LIB_PATH), os.path.dirname(_lib.YUV_LIB_PATH))
    assert os.path.basename(build.YUV_LIB_PATH) == "liboavif_hip_yuv.so" and build.YUV_SOURCES[-1] == "ssimu2_yuv.hip"
    assert build.LIBRARIES[build.YUV_LIB_PATH] is build.YUV_SOURCES  # the table is what build() links
    assert build.LIBRARIES[build.EXT_LIB_PATH] is build.EXT_SOURCES and build.LIBRARIES[build.LIB_PATH] is build.SOURCES
    # its other inputs are exactly the extension library's, and that library's other inputs exactly the product's
    assert build.YUV_SOURCES[:-1] == build.EXT_SOURCES and "ssimu2_yuv.hip" not in build.EXT_SOURCES
    assert build.EXT_SOURCES[:-1] == build.SOURCES and build.EXT_SOURCES[-1] == "ssimu2_ext.hip"
    assert "ssimu2_ext.hip" not in build.SOURCES
    assert os.path.exists(build.YUV_LIB_PATH)


def test_same_version_as_the_product_library(hip_lib, yuv_lib):
    assert yuv_lib.ssimu2_version() == hip_lib.ssimu2_version()


def _frame():
    from oavif_amd.scorer import YuvFrame
    planes = [np.full((4, 4), v, np.uint8) for v in (100, 128, 128)]
    f = YuvFrame(planes)
    return f, f.as_c()


def test_null_context_is_an_invalid_argument(yuv_lib):
    from oavif_amd import _lib
    _f, c = _frame()
    codes = (ctypes.c_uint16 * 48)()
    out = ctypes.c_double()
    assert yuv_lib.ssimu2_convert_yuv(None, ctypes.byref(c), 4, 4, 16, codes) == _lib.ERR_INVALID_ARG
    assert yuv_lib.ssimu2_score_yuv(None, ctypes.byref(c), ctypes.byref(c), 4, 4, 16, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert yuv_lib.ssimu2_set_reference_yuv(None, ctypes.byref(c), 4, 4, 16) == _lib.ERR_INVALID_ARG
    assert yuv_lib.ssimu2_score_against_reference_yuv(None, ctypes.byref(c), 16, ctypes.byref(out)) == _lib.ERR_INVALID_ARG


def test_no_cpu_fallback_without_device(yuv_lib):
    """Without a GPU the YUV library refuses as the product library does; with one it creates a context."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    ctx = ctypes.c_void_p()
    rc = yuv_lib.ssimu2_ctx_create(0, None, ctypes.byref(ctx))
    if torch.cuda.is_available():
        assert rc == _lib.OK and ctx.value
        yuv_lib.ssimu2_ctx_destroy(ctx)
        return
    assert rc == _lib.ERR_NO_DEVICE and not ctx.value
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, yuv=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


def test_yuv_and_instrumented_exclude_each_other():
    from oavif_amd import Ssimu2
    with pytest.raises(ValueError):
        Ssimu2(0, instrumented=True, yuv=True)


def test_yuv_methods_need_the_yuv_library():
    """A context of another library refuses before any C call, naming yuv=True; extended=True alone is not enough, and
    the RGBA refusal keeps its own words."""
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    f, _c = _frame()
    for extended in (False, True):
        s = Ssimu2.__new__(Ssimu2)        # no library, no device: the refusal comes first
        s._L, s._ctx, s.extended = None, ctypes.c_void_p(1), extended
        for call in (lambda: s.convert_yuv(f), lambda: s.compute_ssimu2_yuv(f, f), lambda: s.set_reference_yuv(f),
                     lambda: s.score_against_reference_yuv(f)):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "yuv=True" in str(ei.value)
        s._ctx = ctypes.c_void_p()
    s = Ssimu2.__new__(Ssimu2)
    s._L, s._ctx = None, ctypes.c_void_p(1)
    with pytest.raises(Ssimu2Error) as ei:
        s.composite_rgba(np.zeros((4, 4, 4), np.uint8), 0)
    assert "extended=True" in str(ei.value) and "yuv" not in str(ei.value)
    s._ctx = ctypes.c_void_p()


def test_yuv_frame_values():
    """What YuvFrame takes, copies and refuses, and the struct it makes: no device."""
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    buf = np.arange(3 * 5 * 16, dtype=np.uint8).reshape(3, 5, 16)
    views = [buf[k, :, 1:8] for k in range(3)]                       # rows 16 apart, 7 samples, starts off alignment
    f = YuvFrame(views, 8, _lib.YUV_444, False, 9)
    c = f.as_c()
    assert [c.planes[k] for k in range(3)] == [v.ctypes.data for v in views] and list(c.row_bytes) == [16] * 3
    assert (c.depth, c.format, c.full_range, c.matrix_coefficients, f.width, f.height) == (8, 1, 0, 9, 7, 5)
    g = YuvFrame([buf[0, :, ::2]] * 3)                                # samples not adjacent: copied
    assert g.planes[0].flags.c_contiguous and np.array_equal(g.planes[0], buf[0, :, ::2])
    m = YuvFrame([views[0]], 8, _lib.YUV_400)
    cm = m.as_c()
    assert len(m.planes) == 1 and cm.planes[1] is None and cm.row_bytes[1] == 0
    one = YuvFrame([np.zeros((1, 6), np.uint16)] * 3, 10)             # one row: row_bytes is the row's own length
    assert list(one.as_c().row_bytes) == [12] * 3
    with pytest.raises(TypeError):
        YuvFrame(views, 10)                                           # 10-bit samples are uint16
    with pytest.raises(TypeError):
        YuvFrame([v.astype(np.uint16) for v in views], 8)
    with pytest.raises(ValueError):
        YuvFrame(views[:2])                                           # 4:4:4 needs three planes
    with pytest.raises(ValueError):
        YuvFrame([views[0], views[1], views[2][:, :3]])               # of one shape
    with pytest.raises(ValueError):
        YuvFrame([buf] * 3)


# ---- command lines -------------------------------------------------------------------------------------------------
def test_yuvscore_command_line():
    from oavif_amd import yuvscore
    a = yuvscore.parse_args(["r.png", "d.avif"])
    assert (a.ref, a.dist, a.rgb_depth, a.blur, a.compare, a.device) == ("r.png", "d.avif", 16, "fir", False, 0)
    a = yuvscore.parse_args(["R.AVIF", "d.avif", "--rgb-depth", "8", "--blur", "recursive_fma", "--compare"])
    assert (a.ref, a.rgb_depth, a.blur, a.compare) == ("R.AVIF", 8, "recursive_fma", True)
    for bad in (["r.png"], ["r.png", "d.png"], ["r.jpg", "d.avif"], ["r.png", "d.avif", "--rgb-depth", "7"],
                ["r.png", "d.avif", "--rgb-depth", "17"], ["r.png", "d.avif", "--rgb-depth", "x"],
                ["r.png", "d.avif", "--blur", "gauss"], ["r.png", "d.avif", "extra"]):
        with pytest.raises(SystemExit) as ei:
            yuvscore.parse_args(bad)
        assert ei.value.code == 2, bad
    with pytest.raises(SystemExit) as ei:
        yuvscore.parse_args(["--help"])
    assert ei.value.code == 0


def test_yuvscore_help_names_its_options(capsys):
    from oavif_amd import yuvscore
    with pytest.raises(SystemExit):
        yuvscore.parse_args(["-h"])
    out = capsys.readouterr().out
    assert "--rgb-depth" in out and "--compare" in out and "--blur" in out


def test_score_yuv_option():
    from oavif_amd import cli
    o, inp, out = cli.parse_args(["a.png", "b.avif"])
    assert o.score_yuv is False
    o, inp, out = cli.parse_args(["--score-yuv", "1", "a.png", "--tenbit", "0", "b.avif"])
    assert o.score_yuv is True and o.tenbit is False and (inp, out) == ("a.png", "b.avif")
    assert cli.parse_args(["--score-yuv", "0", "a.png", "b.avif"])[0].score_yuv is False
    for argv, name in ((["--score-yuv"], "MissingOptionValue"), (["--score-yuv", "2"], "InvalidOptionValue"),
                       (["--score-yuv", "x"], "InvalidCharacter")):
        with pytest.raises(cli.CliError) as ei:
            cli.parse_args(argv)
        assert ei.value.name == name


def test_score_yuv_probes_hand_over_planes_or_fall_back_with_a_note(monkeypatch):
    """search_image under --score-yuv 1, the search itself replaced by one probe (no device): a yuv context gets the
    decoder's planes; a context without the YUV calls, and an image with an alpha plane, get libavif's RGB rows and
    one note."""
    from oavif_amd import avif_bridge as ab, cli, search, synth, tq
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    handed = []

    def one_probe(scorer, ref, codec_frame, **how):
        for q in (60, 70):
            frame, size = codec_frame(q)
            handed.append((type(frame).__name__, getattr(frame, "matrix_coefficients", None), size > 0))
            frame.close()
        return tq.TQResult(q=70, score=80.0, num_pass=2, buf_q=70, history=[(60, 75.0), (70, 80.0)])

    monkeypatch.setattr(tq, "search_hip_frames", one_probe)

    class Ctx:
        def __init__(self, yuv):
            self.yuv = yuv

    rgb = synth.make_ref(48, 32, seed=1)
    rgba = np.concatenate([rgb, np.full((32, 48, 1), 200, np.uint8)], -1)
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.quality_alpha, o.score_yuv = False, 10, 90, True
    for pixels, yuv, want, noted in ((rgb, True, "DecodedYuv", None), (rgb, False, "DecodedFrame", "yuv=True"),
                                     (rgba, True, "DecodedFrame", "alpha plane")):
        del handed[:]
        notes = []
        src = cli.Source(rgb, pixels, pixels.shape[2], False, None)
        with cli.encoder_input(pixels, o) as prepared:
            r, data = search.search_image(src, o, [Ctx(yuv)], prepared, note=notes.append)
        assert r.q == 70 and len(data) > 0
        assert [h[0] for h in handed] == [want] * 2 and all(h[2] for h in handed), handed
        if want == "DecodedYuv":
            assert handed[0][1] == o.matrix_coefficients and notes == []
        else:
            assert len(notes) == 1 and "--score-yuv" in notes[0] and noted in notes[0], notes
    o.score_yuv = False                      # the default: the RGB path, and not a word
    del handed[:]
    notes = []
    with cli.encoder_input(rgb, o) as prepared:
        search.search_image(cli.Source(rgb, rgb, 3, False, None), o, [Ctx(True)], prepared, note=notes.append)
    assert [h[0] for h in handed] == ["DecodedFrame"] * 2 and notes == []
