"""ssimu2_alpha_table without a GPU (include/ssimu2_hip_ext.h): the table T of the 65,026
composite codes against the numpy fp64 expression, its tie to the 8-bit table, and its order."""
import numpy as np
import pytest

CODES = 255 * 255 + 1


@pytest.fixture(scope="module")
def table(hip_lib):
    from oavif_amd import scorer
    return scorer.alpha_table()


def expected_table():
    """(float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)), v = n / 65025 in fp64."""
    v = np.arange(CODES, dtype=np.float64) / 65025.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4).astype(np.float32)


def test_table_is_the_fp64_expression_rounded_once(table):
    assert table.shape == (CODES,) and table.dtype == np.float32
    exp = expected_table()
    bad = np.flatnonzero(table.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, (bad[:8].tolist(), table[bad[:8]].tolist(), exp[bad[:8]].tolist())
    assert table[0] == 0.0 and table[-1] == 1.0


def test_every_255th_entry_is_the_8bit_table(table, hip_lib):
    from oavif_amd import scorer
    t8 = scorer.linear_table(8)
    assert t8.shape == (256,)
    assert np.array_equal(table[255 * np.arange(256)].view(np.uint32), t8.view(np.uint32))


def test_table_is_strictly_increasing(table):
    assert (np.diff(table.astype(np.float64)) >= 0).all()
    assert np.unique(table).size == CODES


def test_every_code_occurs():
    """n = a*c + (255 - a)*b reaches every integer of 0 .. 65025 (the table has no unused entry)."""
    seen = np.zeros(CODES, bool)
    a = np.arange(256, dtype=np.int64)[:, None, None]
    c = np.arange(256, dtype=np.int64)[None, :, None]
    for b0 in range(0, 256, 32):
        b = np.arange(b0, b0 + 32, dtype=np.int64)[None, None, :]
        seen[(a * c + (255 - a) * b).ravel()] = True
    assert seen.all()


def test_null_out_is_an_invalid_argument(hip_lib):
    from oavif_amd import _lib
    assert _lib.ext_lib().ssimu2_alpha_table(None) == _lib.ERR_INVALID_ARG
