"""The batch library of every blur mode without a GPU (include/ssimu2_hip_rbatch.h): the header
against the binding table and the calls it mirrors, the library's exports (the YUVA library's and the four new calls,
nothing else) and the other seven libraries' (what their tables say, none of the new calls), the header as C, build.py's
tables (the four earlier ones as they were, the eighth library in a fifth), the new unit's device code (no kernel, no
constant block), the budgets of the batch kernels from the compiler's metadata -- held to the limits
tests/test_isa_budget.py holds their single-score counterparts to --, what every new call answers to a null context,
the Python flag, and the --blur option of oavif_amd.scorepairs against a stand-in scorer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import isa_text
from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes
from test_build_units import _includes

HEADER = "ssimu2_hip_rbatch.h"
UNIT = "ssimu2_rbatch.hip"
# each new call and the call of ssimu2_hip.h whose parameter list it has
MIRRORED = {"ssimu2_rbatch_score_rgb8": "ssimu2_score_batch_rgb8",
            "ssimu2_rbatch_score_against_reference": "ssimu2_score_batch_against_reference",
            "ssimu2_rbatch_score_rgb8_device": "ssimu2_score_batch_rgb8_device",
            "ssimu2_rbatch_score_against_reference_device": "ssimu2_score_batch_against_reference_device"}
NAMES = list(MIRRORED)


@pytest.fixture(scope="module")
def rbatch_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.rbatch_lib()


def _plain(path):
    return {s for s in _exported(path) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.RBATCH_FUNCTIONS) == NAMES                          # header order
    assert _lib.RBATCH_SYMBOLS == tuple(_lib.RBATCH_FUNCTIONS)
    assert set(_declared_functions(HEADER)) == set(NAMES)
    assert list(prototypes(HEADER)) == NAMES
    others = (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS) |
              set(_lib.MAP_FUNCTIONS) | set(_lib.CHROMA_FUNCTIONS) | set(_lib.YUVA_FUNCTIONS))
    assert not set(NAMES) & others
    assert os.path.basename(_lib.RBATCH_LIB_PATH) == "liboavif_hip_rbatch.so"


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header_and_the_call_it_mirrors(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.RBATCH_FUNCTIONS[name]
    ret, params = prototypes(HEADER)[name]
    check(name, (ret, params), restype, argtypes)
    old_ret, old_params = prototypes("ssimu2_hip.h")[MIRRORED[name]]
    norm = lambda ds: [re.sub(r"\s+", " ", d) for d in ds]   # noqa: E731
    assert ret == old_ret and norm(params) == norm(old_params), name
    assert (restype, argtypes) == _lib.PUBLIC_FUNCTIONS[MIRRORED[name]]


def test_the_library_exports_the_yuva_library_plus_the_four_calls(rbatch_lib):
    from oavif_amd import _lib
    plain, yuva_plain = _plain(_lib.RBATCH_LIB_PATH), _plain(_lib.YUVA_LIB_PATH)
    assert plain - yuva_plain == set(NAMES) and yuva_plain <= plain
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = (public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS) | set(_lib.CHROMA_SYMBOLS) |
            set(_lib.YUVA_SYMBOLS) | set(NAMES))
    assert plain == want, plain ^ want
    for name in want:
        assert hasattr(rbatch_lib, name), name


def test_the_other_seven_libraries_export_what_they_did(hip_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    ext, yuv, maps = set(_lib.EXT_SYMBOLS), set(_lib.YUV_SYMBOLS), set(_lib.MAP_SYMBOLS)
    chroma, yuva = set(_lib.CHROMA_SYMBOLS), set(_lib.YUVA_SYMBOLS)
    want = {_lib.LIB_PATH: public, _lib.INSTR_LIB_PATH: public | set(_lib.INSTR_SYMBOLS), _lib.EXT_LIB_PATH: public | ext,
            _lib.YUV_LIB_PATH: public | ext | yuv, _lib.MAP_LIB_PATH: public | ext | yuv | maps,
            _lib.CHROMA_LIB_PATH: public | ext | yuv | maps | chroma,
            _lib.YUVA_LIB_PATH: public | ext | yuv | maps | chroma | yuva}
    assert len(want) == 7
    for path, names in want.items():
        got = {s for s in _exported(path) if s.startswith(("ssimu2_", "oavif_"))}
        assert got == names, (path, got ^ names)
        assert not got & set(NAMES), path


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "ssimu2_hip_rbatch.h"\n'
                   "int main(void) {\n"
                   "    double out[1];\n"
                   "    int rc = ssimu2_rbatch_score_rgb8(0, 0, 0, 0, 8, 8, out);\n"
                   "    rc |= ssimu2_rbatch_score_against_reference(0, 0, 0, out);\n"
                   "    rc |= ssimu2_rbatch_score_rgb8_device(0, 0, 0, (size_t)0, 0, 8, 8, out);\n"
                   "    rc |= ssimu2_rbatch_score_against_reference_device(0, 0, (size_t)0, 0, out);\n"
                   "    return rc == 0 ? SSIMU2_MAX_BATCH : 0;\n"
                   "}\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(isa_text.ROOT, "include"), str(src)], check=True)


def test_build_keeps_its_four_tables_and_knows_the_eighth_library_in_a_fifth(hip_lib):
    from oavif_amd import _lib, build
    assert list(build.LIBRARIES) == [build.LIB_PATH, build.INSTR_LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH]
    assert build.MAP_LIBRARIES == {build.MAP_LIB_PATH: [*build.YUV_SOURCES, "ssimu2_map.hip"]}
    assert build.CHROMA_LIBRARIES == {build.CHROMA_LIB_PATH: [*build.MAP_SOURCES, "ssimu2_chroma.hip"]}
    assert build.YUVA_LIBRARIES == {build.YUVA_LIB_PATH: [*build.CHROMA_SOURCES, "ssimu2_yuva.hip"]}
    assert build.RBATCH_LIBRARIES == {build.RBATCH_LIB_PATH: build.RBATCH_SOURCES}
    assert build.RBATCH_SOURCES == [*build.YUVA_SOURCES, UNIT]
    for table in (build.LIBRARIES, build.MAP_LIBRARIES, build.CHROMA_LIBRARIES, build.YUVA_LIBRARIES):
        assert build.RBATCH_LIB_PATH not in table
    assert build.rbatch_units() == [UNIT]
    assert UNIT not in (*build.compile_units(), *build.map_units(), *build.chroma_units(), *build.yuva_units())
    assert os.path.samefile(os.path.dirname(build.RBATCH_LIB_PATH), os.path.dirname(_lib.RBATCH_LIB_PATH))
    assert os.path.basename(build.RBATCH_LIB_PATH) == "liboavif_hip_rbatch.so"
    assert os.path.exists(os.path.join(build.CSRC, UNIT)) and os.path.exists(build.RBATCH_LIB_PATH)   # built by build.build()


def test_build_rebuilds_when_the_eighth_library_is_missing(hip_lib, monkeypatch, tmp_path):
    from oavif_amd import build
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "RBATCH_LIBRARIES", {str(tmp_path / "liboavif_hip_rbatch.so"): build.RBATCH_SOURCES})
    assert build.libs_need_build()


def test_the_unit_has_no_kernel_and_no_constant_block():
    asm = isa_text.unit_asm(UNIT)
    assert not re.findall(r"^\s*\.amdhsa_kernel\b", asm, re.M)
    assert "c_k" not in asm
    from oavif_amd import build
    inc = _includes(os.path.join(build.CSRC, UNIT))
    assert "ssimu2_host.h" in inc and HEADER in inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_kernels.h", "ssimu2_recursive.h"}


# ---- budgets of the batch kernels, from the metadata of the scorer unit's one device-only compile --------------------
@pytest.fixture(scope="module")
def kernels():
    meta = {}
    for block in isa_text.scorer_asm().split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
                                "private_segment_fixed_size")}
    return meta


def _some(meta, fragment, count):
    hits = {k: v for k, v in meta.items() if fragment in k}
    assert len(hits) == count, (fragment, sorted(hits))
    return hits.values()


def test_the_batch_kernels_keep_the_budgets_of_their_single_score_counterparts(kernels):
    for k in _some(kernels, "k_rg_h_batchILb", 4):         # <FMA, REF>: as k_rg_h
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["vgpr_count"] <= 256, k
        assert 3 * k["group_segment_fixed_size"] <= 160 * 1024, k
    for k in _some(kernels, "k_rg_v_batchILb", 2):         # <FMA>: as k_rg_v
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["vgpr_count"] <= 128, k
    for frag, count in (("k_rg_v_emit_batchILb", 2), ("k_pyramid_bands_xyb_batch", 1)):
        for k in _some(kernels, frag, count):
            assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (frag, k)
    print("measured (VGPRs, LDS bytes):", {n: (v["vgpr_count"], v["group_segment_fixed_size"]) for n, v in kernels.items()
                                           if "k_rg_" in n and "_batch" in n or "xyb_batch" in n})


# ---- the calls and the Python side ---------------------------------------------------------------------------------
def test_null_context_is_an_invalid_argument(rbatch_lib):
    from oavif_amd import _lib
    L, E, out = rbatch_lib, _lib.ERR_INVALID_ARG, (ctypes.c_double * 2)()
    f = np.zeros((8, 8, 3), np.uint8)
    pp = (ctypes.POINTER(ctypes.c_uint8) * 2)(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))] * 2)
    assert L.ssimu2_rbatch_score_rgb8(None, pp, pp, 2, 8, 8, out) == E
    assert L.ssimu2_rbatch_score_against_reference(None, pp, 2, out) == E
    assert L.ssimu2_rbatch_score_rgb8_device(None, 4096, 8192, 192, 2, 8, 8, out) == E
    assert L.ssimu2_rbatch_score_against_reference_device(None, 4096, 192, 2, out) == E
    assert L.ssimu2_rbatch_score_rgb8(None, None, None, 0, 8, 8, None) == E   # the null context comes before n == 0


def test_same_version_as_the_product_library(hip_lib, rbatch_lib):
    assert rbatch_lib.ssimu2_version() == hip_lib.ssimu2_version()


class _Lib:
    """A stand-in library: every batch call answers with its own name."""

    def __getattr__(self, name):
        return lambda *a: name


def test_the_flag_chooses_the_calls_and_without_it_nothing_changes():
    from oavif_amd import Ssimu2
    from oavif_amd.scorer import _RBATCH_CALLS
    assert _RBATCH_CALLS == {old: new for new, old in MIRRORED.items()}
    assert Ssimu2.rbatch is False
    s = Ssimu2.__new__(Ssimu2)        # no library, no device
    s._L = _Lib()
    for old, new in _RBATCH_CALLS.items():
        s.rbatch = False
        assert s._batch_fn(old)() == old
        s.rbatch = True
        assert s._batch_fn(old)() == new
    with pytest.raises(ValueError) as ei:
        Ssimu2(0, instrumented=True, rbatch=True)
    assert "instrumented=True and rbatch=True are different libraries" in str(ei.value)


def test_no_cpu_fallback_without_device(rbatch_lib):
    """Without a GPU the library refuses as the product library does; with one the flag implies every earlier one."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    if torch.cuda.is_available():
        with Ssimu2(0, rbatch=True) as s:
            assert s.rbatch and s.yuva and s.chroma and s.maps and s.yuv and s.extended
        return
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, rbatch=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


# ---- command line --------------------------------------------------------------------------------------------------
class _FakeScorer:
    def score_batch(self, refs, dists):
        return np.array([float(int(r[0, 0, 0]) * 1000 + int(d[0, 0, 0])) for r, d in zip(refs, dists)])

    def close(self):
        self.closed = True


def test_scorepairs_blur_option(tmp_path, monkeypatch, capsys):
    from oavif_amd import pam, scorepairs
    for tag, name in ((1, "r.pam"), (2, "d.pam")):
        a = np.zeros((8, 16, 3), np.uint8)
        a[0, 0, 0] = tag
        (tmp_path / name).write_bytes(pam.write_pam(a))
    tsv, out = tmp_path / "pairs.tsv", tmp_path / "out.csv"
    tsv.write_text("r.pam\td.pam\n")
    made = []

    def stand_in(device, blur):
        made.append((device, blur, _FakeScorer()))
        return made[-1][2]
    monkeypatch.setattr(scorepairs, "make_scorer", stand_in)
    assert scorepairs.BLUR_MODES == ("fir", "recursive", "recursive_fma")
    assert scorepairs.main([str(tsv), str(out)]) == 0                       # the default: fir, as ever
    assert scorepairs.main([str(tsv), str(out), "--device", "3", "--blur", "recursive"]) == 0
    assert scorepairs.main(["--blur", "recursive_fma", str(tsv), str(out), "--batch", "2"]) == 0
    assert scorepairs.main([str(tsv), str(out), "--blur", "fir"]) == 0
    assert [(d, b) for d, b, _ in made] == [(0, "fir"), (3, "recursive"), (0, "recursive_fma"), (0, "fir")]
    assert all(s.closed for _, _, s in made)
    assert out.read_text().splitlines()[1].endswith(",16,8,1002.0")
    for bad in (["--blur"], ["--blur", "gauss"], ["--blur", "1"], ["--blur", "RECURSIVE"]):
        assert scorepairs.main([str(tsv), str(out), *bad]) == 2, bad
    assert "--blur needs one of fir, recursive, recursive_fma" in capsys.readouterr().err
    assert len(made) == 4                                                    # a bad option makes no scorer
    assert scorepairs.main([str(tsv)]) == 2 and "--blur" in capsys.readouterr().err


def test_scorepairs_binds_the_product_library_in_fir_and_the_batch_library_otherwise(monkeypatch):
    from oavif_amd import scorepairs, scorer
    made = []
    monkeypatch.setattr(scorer, "Ssimu2", lambda *a, **kw: made.append((a, kw)))
    for blur in scorepairs.BLUR_MODES:
        scorepairs.make_scorer(2, blur)
    assert made == [((2,), {}), ((2,), {"blur": 1, "rbatch": True}), ((2,), {"blur": 2, "rbatch": True})]
