"""CPU: tests/char_dict_reference.py against plain Python, and its restated hash against qsx_char_dict_hash of the library
(host arithmetic: needs no GPU)."""
import ctypes as C
import time

import numpy as np
import pytest

import char_dict_reference as R

WIDTHS = (1, 9, 25, 255)


@pytest.mark.parametrize("width", (1, 3, 9, 10, 16, 25, 64, 255))
def test_the_partition_equals_a_python_dict_over_bytes(width):
    col = R.make_stripe(width, 3000, seed=50 + width)
    keep = np.random.default_rng(width).random(3000) < 0.7
    for mask in (None, keep):
        labels, distinct = R.intern(col, mask)
        seen, want = {}, []
        for i, row in enumerate(col):
            if mask is not None and not mask[i]:
                want.append(-1)
                continue
            text = bytes(row).split(b"\0")[0]
            want.append(seen.setdefault(text, len(seen)))
        assert distinct == len(seen)
        assert R.same_partition(labels, np.array(want))
        assert not R.same_partition(labels, np.zeros(3000, dtype=np.int64)) or distinct <= 1
    canon = R.canonical(col)
    for i in range(0, 3000, 97):
        text = bytes(col[i]).split(b"\0")[0]
        assert bytes(canon[i]) == text.ljust(width, b"\0")


def library_hashes(capi, col):
    width = col.shape[1]
    fn = capi.lib.qsx_char_dict_hash
    return np.array([fn(C.c_char_p(bytes(row)), width) for row in col], dtype=np.uint64)


@pytest.mark.parametrize("width", WIDTHS)
def test_the_restated_hash_equals_the_library_on_random_texts(capi, width):
    col = R.make_stripe(width, 10_000, seed=900 + width)
    col[0] = 0                                        # the empty text
    col[1] = np.arange(1, width + 1, dtype=np.int64) % 255 + 1   # a full-width text without a NUL
    assert R.lengths(col)[0] == 0 and R.lengths(col)[1] == width
    mine = R.hash_texts(col)
    assert np.array_equal(mine, library_hashes(capi, col))
    if width >= 9:
        assert np.unique(mine).size == np.unique(R.intern(col)[0]).size        # no 64-bit collision among 10^4 texts


def test_texts_that_differ_only_behind_a_nul_hash_equal(capi):
    a = R.field(b"ab", 9)
    b = a.copy()
    b[3:] = (7, 8, 9, 10, 11, 12)
    c = R.field(b"abb", 9)
    h = library_hashes(capi, np.stack([a, b, c]))
    assert h[0] == h[1] and h[0] != h[2]
    assert capi.char_dict_hash(b"ab", 9) == int(h[0]) == capi.char_dict_hash(b"ab\0zz", 9)
    assert capi.char_dict_hash(b"", 9) == int(R.hash_texts(np.zeros((1, 9), dtype=np.uint8))[0])
    # the same text in fields of different widths is the same text
    assert capi.char_dict_hash(b"ab", 25) == int(h[0])


def test_a_seeded_search_finds_the_committed_collision_pair(capi):
    began = time.monotonic()
    found = R.collision_search(seed=1)
    assert time.monotonic() - began < 30, "the search is meant to take a few seconds"
    assert found == R.COLLISION_PAIR


def test_the_committed_pair_collides_under_the_library_hash(capi):
    a, b = R.COLLISION_PAIR
    assert a != b
    ha, hb = capi.char_dict_hash(a, R.COLLISION_WIDTH), capi.char_dict_hash(b, R.COLLISION_WIDTH)
    assert ha != hb                                           # (different texts, different 64-bit hashes)
    assert R.fingerprint(ha) == R.fingerprint(hb)             # ... the same fingerprint
    assert R.home_slot(ha) == R.home_slot(hb)                 # ... and the same home slot in the smallest table
