"""oavif_amd._lib's signature tables against the prototypes of include/*.h: argument count, the class of every
argument and of the return type.  tests/test_abi.py compares names only; a wrong argtypes list would otherwise first
show as a corrupted argument on the GPU.  Needs no library and no device."""
import ctypes
import os
import re

import pytest

from oavif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_HEADERS, HOOK_HEADER = ("ssimu2_hip.h", "oavif_tq.h"), "ssimu2_hip_internal.h"

SCALARS = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
           "float": ctypes.c_float, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16}
STRUCTS = {"ssimu2_device_info": _lib.DeviceInfo, "oavif_tq_options": _lib.TQOptions, "oavif_tq_pass": _lib.TQPass,
           "oavif_tq_result": _lib.TQResult, "oavif_tq_spec_options": _lib.TQSpecOptions,
           "oavif_tq_spec_stats": _lib.TQSpecStats, "oavif_png_info": _lib.PngInfo}
CALLBACKS = {"oavif_tq_probe_fn": _lib.PROBE_FN, "oavif_tq_codec_fn": _lib.CODEC_FN,
             "oavif_tq_batch_probe_fn": _lib.BATCH_PROBE_FN}


def _code(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M)      # preprocessor lines, continuations included


def _split(args):
    args = args.strip()
    return [] if args in ("", "void") else [a.strip() for a in args.split(",")]


def prototypes(header):
    """{name: (return type, [parameter declarations])} of the functions a header declares."""
    found = re.findall(r"([A-Za-z_][\w \t\*]*?)\b((?:ssimu2|oavif)_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _code(header))
    return {name: (ret.strip(), _split(args)) for ret, name, args in found}


def callback_typedefs(header):
    found = re.findall(r"typedef\s+([\w \t\*]+?)\s*\(\s*\*\s*(\w+_fn)\s*\)\s*\(([^()]*)\)\s*;", _code(header))
    return {name: (ret.strip(), _split(args)) for ret, name, args in found}


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)))


def mismatch(decl, ctype, is_return=False):
    """None when the ctypes type is of the class the C declaration asks for, else what is wrong."""
    if "[" in decl:                                   # `double out[108]` is `double* out`
        decl = re.sub(r"\s*\w+\s*\[.*\]", "*", decl)
    elif not is_return:
        decl = re.sub(r"\b\w+$", "", decl)            # the parameter's name
    words = [w for w in re.sub(r"\*", " ", decl).split() if w != "const"]
    stars = decl.count("*")
    base = " ".join(words)
    if stars:
        if not _is_pointer(ctype):
            return f"`{decl.strip()}` is a pointer, bound as {ctype}"
        if stars == 1 and isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
            want = SCALARS.get(base) or STRUCTS.get(base)
            if want is not None and ctype._type_ is not want:
                return f"`{decl.strip()}` bound as a pointer to {ctype._type_}"
        return None
    if base in CALLBACKS:
        return None if ctype is CALLBACKS[base] else f"`{base}` bound as {ctype}"
    if base == "void" and is_return:
        return None if ctype is None else f"void bound as {ctype}"
    if base not in SCALARS:
        return f"unknown C type `{base}`"
    return None if ctype is SCALARS[base] else f"`{base}` bound as {ctype}"


def check(name, proto, restype, argtypes):
    ret, params = proto
    assert len(params) == len(argtypes), f"{name}: {len(params)} parameters in the header, {len(argtypes)} argtypes"
    for i, (decl, ctype) in enumerate(zip(params, argtypes)):
        why = mismatch(decl, ctype)
        assert why is None, f"{name}, argument {i}: {why}"
    why = mismatch(ret, restype, is_return=True)
    assert why is None, f"{name}, return type: {why}"


PUBLIC = {k: v for h in PUBLIC_HEADERS for k, v in prototypes(h).items()}
HOOKS = prototypes(HOOK_HEADER)


def test_the_tables_hold_exactly_the_declared_functions():
    assert (len(PUBLIC), len(HOOKS)) == (44, 14)
    assert set(_lib.PUBLIC_FUNCTIONS) == set(PUBLIC)
    assert set(_lib.HOOK_FUNCTIONS) == set(HOOKS)
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib.PUBLIC_FUNCTIONS) and _lib.INSTR_SYMBOLS == tuple(_lib.HOOK_FUNCTIONS)


@pytest.mark.parametrize("name", sorted(PUBLIC) + sorted(HOOKS))
def test_signature_matches_the_header(name):
    restype, argtypes = (_lib.PUBLIC_FUNCTIONS if name in PUBLIC else _lib.HOOK_FUNCTIONS)[name]
    check(name, PUBLIC[name] if name in PUBLIC else HOOKS[name], restype, argtypes)


def test_callback_types_match_their_typedefs():
    typedefs = callback_typedefs("oavif_tq.h")
    assert set(typedefs) == set(CALLBACKS)
    for name, proto in typedefs.items():
        check(name, proto, CALLBACKS[name]._restype_, list(CALLBACKS[name]._argtypes_))


def test_the_check_itself_sees_a_wrong_table():
    """The mutations a slip would make: an argument dropped, a uint32_t declared size_t, a scalar where a pointer
    belongs, a pointer to the wrong sample type, a void function given a return type."""
    name = "ssimu2_score_against_reference_strided"
    restype, argtypes = _lib.PUBLIC_FUNCTIONS[name]
    check(name, PUBLIC[name], restype, argtypes)
    wrong = [(restype, argtypes[:-1]),
             (restype, argtypes[:2] + [ctypes.c_size_t] + argtypes[3:]),
             (restype, argtypes[:4] + [ctypes.c_double]),
             (restype, argtypes[:1] + [ctypes.POINTER(ctypes.c_uint16)] + argtypes[2:]),
             (ctypes.c_uint32, argtypes)]
    for r, a in wrong:
        with pytest.raises(AssertionError):
            check(name, PUBLIC[name], r, a)
    with pytest.raises(AssertionError):
        check("ssimu2_ctx_destroy", PUBLIC["ssimu2_ctx_destroy"], ctypes.c_int, [ctypes.c_void_p])
