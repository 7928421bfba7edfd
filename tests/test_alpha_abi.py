"""The extension library without a GPU (include/ssimu2_hip_ext.h): the header against the binding
table, the library's exports (the public ABI plus the five RGBA entry points and nothing else), what every new call
answers to a null context, no CPU fallback, and the command line of oavif_amd.alpha."""
import ctypes

import pytest

from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes

EXT_HEADER = "ssimu2_hip_ext.h"
EXT_NAMES = ["ssimu2_alpha_table", "ssimu2_composite_rgba8", "ssimu2_score_rgba8", "ssimu2_set_reference_rgba8",
             "ssimu2_score_against_reference_rgba8"]


@pytest.fixture(scope="module")
def ext_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.ext_lib()


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.EXT_FUNCTIONS) == EXT_NAMES                         # header order
    assert _lib.EXT_SYMBOLS == tuple(_lib.EXT_FUNCTIONS)
    assert set(_declared_functions(EXT_HEADER)) == set(_lib.EXT_FUNCTIONS)
    protos = prototypes(EXT_HEADER)
    assert list(protos) == EXT_NAMES
    assert not set(_lib.EXT_FUNCTIONS) & (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS))


@pytest.mark.parametrize("name", EXT_NAMES)
def test_signature_matches_the_header(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.EXT_FUNCTIONS[name]
    check(name, prototypes(EXT_HEADER)[name], restype, argtypes)


def test_the_code_count_is_the_headers():
    import os
    import re
    from oavif_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", EXT_HEADER)).read()
    assert int(re.search(r"#define\s+SSIMU2_ALPHA_CODES\s+(\d+)", text).group(1)) == _lib.ALPHA_CODES == 255 * 255 + 1


def test_extension_library_exports_the_public_abi_plus_the_rgba_calls(ext_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = public | set(_lib.EXT_SYMBOLS)
    got = {s for s in _exported(_lib.EXT_LIB_PATH) if s.startswith(("ssimu2_", "oavif_"))}
    assert got == want, got ^ want
    plain = {s for s in _exported(_lib.EXT_LIB_PATH) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}
    assert plain == want, plain ^ want
    for name in want:
        assert hasattr(ext_lib, name), name


def test_the_other_libraries_have_none_of_it(hip_lib):
    from oavif_amd import _lib
    for path in (_lib.LIB_PATH, _lib.INSTR_LIB_PATH):
        assert not set(_exported(path)) & set(_lib.EXT_SYMBOLS), path


def test_same_version_as_the_product_library(hip_lib, ext_lib):
    """The scoring service compares ssimu2_version(): a context of the extension library must still be served."""
    assert ext_lib.ssimu2_version() == hip_lib.ssimu2_version()


def test_null_context_is_an_invalid_argument(ext_lib):
    from oavif_amd import _lib
    px = (ctypes.c_uint8 * 64)()
    codes = (ctypes.c_uint16 * 48)()
    out = ctypes.c_double()
    assert ext_lib.ssimu2_composite_rgba8(None, px, 16, 4, 4, 0, codes) == _lib.ERR_INVALID_ARG
    assert ext_lib.ssimu2_score_rgba8(None, px, 16, px, 16, 4, 4, 0, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert ext_lib.ssimu2_set_reference_rgba8(None, px, 16, 4, 4, 0) == _lib.ERR_INVALID_ARG
    assert ext_lib.ssimu2_score_against_reference_rgba8(None, px, 16, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert ext_lib.ssimu2_alpha_table(None) == _lib.ERR_INVALID_ARG


def test_no_cpu_fallback_without_device(ext_lib):
    """Without a GPU the extension library refuses as the product library does; with one it creates a context."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    ctx = ctypes.c_void_p()
    rc = ext_lib.ssimu2_ctx_create(0, None, ctypes.byref(ctx))
    if torch.cuda.is_available():
        assert rc == _lib.OK and ctx.value
        ext_lib.ssimu2_ctx_destroy(ctx)
        return
    assert rc == _lib.ERR_NO_DEVICE and not ctx.value
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, extended=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


def test_extended_and_instrumented_exclude_each_other():
    from oavif_amd import Ssimu2
    with pytest.raises(ValueError):
        Ssimu2(0, instrumented=True, extended=True)


def test_rgba_methods_need_the_extension_library():
    """A context of the product library refuses before any C call, naming extended=True."""
    import numpy as np
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    s = Ssimu2.__new__(Ssimu2)        # no library, no device: the refusal comes first
    s._L, s._ctx = None, ctypes.c_void_p(1)
    a = np.zeros((4, 4, 4), np.uint8)
    for call in (lambda: s.composite_rgba(a, 0), lambda: s.compute_ssimu2_rgba(a, a, (1, 2, 3)),
                 lambda: s.set_reference_rgba(a, 0), lambda: s.score_against_reference_rgba(a)):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "extended=True" in str(ei.value)
    s._ctx = ctypes.c_void_p()


def test_backgrounds_as_tuples_and_ints():
    from oavif_amd.scorer import background_rgb
    assert background_rgb((0x1A, 0x80, 0xE6)) == 0x1A80E6 == background_rgb(0x1A80E6)
    assert background_rgb((0, 0, 0)) == 0 and background_rgb((255, 255, 255)) == 0xFFFFFF
    for bad in (-1, 0x1000000, (256, 0, 0), (0, -1, 0)):
        with pytest.raises(ValueError):
            background_rgb(bad)
    with pytest.raises(ValueError):
        background_rgb((1, 2))


def test_command_line_backgrounds():
    from oavif_amd import alpha
    a = alpha.parse_args(["r.png", "d.png"])
    assert a.background == [0x1A1A1A, 0xE6E6E6] == list(alpha.DEFAULT_BACKGROUNDS) and a.blur == "fir"
    a = alpha.parse_args(["r.png", "d.png", "--background", "ffFFff", "--background", "000000", "--blur", "recursive_fma"])
    assert a.background == [0xFFFFFF, 0] and a.blur == "recursive_fma" and (a.ref, a.dist) == ("r.png", "d.png")
    assert alpha.parse_background("1A80E6") == 0x1A80E6
    for bad in ("FFF", "1234567", "GGGGGG", "0x1A1A", "", "+1A1A1", "1A 1A1"):
        with pytest.raises(SystemExit):
            alpha.parse_args(["r.png", "d.png", "--background", bad])
    with pytest.raises(SystemExit):
        alpha.parse_args(["r.png", "d.png", "--blur", "gauss"])


def test_rgb_sources_count_as_opaque():
    import numpy as np
    from oavif_amd import alpha
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    out = alpha.as_rgba(rgb)
    assert out.shape == (2, 3, 4) and np.array_equal(out[..., :3], rgb) and (out[..., 3] == 255).all()
    rgba = np.zeros((2, 3, 4), np.uint8)
    assert np.array_equal(alpha.as_rgba(rgba), rgba)
    with pytest.raises(ValueError):
        alpha.as_rgba(np.zeros((2, 3, 4), np.uint16))
