"""eon_kzg_mmcs_local_index, the index mapping of KzgMmcs::open_batch / verify_batch
(kzg/src/mmcs.rs:213-218, :272-277), against a restatement of those lines.  A pure host function:
needs the built library, no GPU."""

import pytest

from plonky3_eon_amd import _lib

HEIGHTS = [1, 2, 5, 8, 300, 512, 513]
MAX_HEIGHTS = [8, 513, 1024]


def _log2(x: int) -> int:
    """usize::next_power_of_two().trailing_zeros()"""
    return (max(x, 1) - 1).bit_length()


def reference_local_index(max_height: int, height: int, index: int) -> int:
    log2_max, log2_h = _log2(max_height), _log2(height)
    shifted = index >> (log2_max - log2_h) if log2_max >= log2_h else index
    return shifted % height


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        pytest.fail("libeonhip.so is not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.mark.parametrize("max_height", MAX_HEIGHTS)
@pytest.mark.parametrize("height", HEIGHTS)
def test_local_index_matches_the_reference_mapping(lib, max_height, height):
    for index in (0, max_height - 1, max_height, max_height + 3):
        got = lib.eon_kzg_mmcs_local_index(max_height, height, index)
        assert got == reference_local_index(max_height, height, index), (max_height, height, index)
        assert got < height


def test_local_index_covers_the_cases_the_mapping_has(lib):
    """Shift 0 (equal log2), a real shift, a non-power-of-two wrap, and height above max_height."""
    assert lib.eon_kzg_mmcs_local_index(513, 513, 512) == 512   # log2 10 == log2 10, no shift
    assert lib.eon_kzg_mmcs_local_index(513, 513, 1023) == 510  # ... and the modulo wrap
    assert lib.eon_kzg_mmcs_local_index(1024, 8, 1023) == 7     # shift by 7
    assert lib.eon_kzg_mmcs_local_index(1024, 5, 1023) == 2     # shift by 7, then 7 % 5
    assert lib.eon_kzg_mmcs_local_index(8, 300, 1027) == 127    # taller than max: index % height
    assert lib.eon_kzg_mmcs_local_index(1024, 1, 77) == 0


def test_local_index_height_zero(lib):
    """The reference divides by zero; the C function answers UINT64_MAX."""
    assert lib.eon_kzg_mmcs_local_index(8, 0, 3) == 2**64 - 1


def test_python_helper_goes_through_the_library():
    from plonky3_eon_amd.mmcs import local_index

    assert local_index(1024, 300, 1026) == reference_local_index(1024, 300, 1026)
