"""What the device dictionary of CHAR(n) values (qsx_char_dict_*, include/qsx.h) has to compute, in numpy: a value's text is
its field up to the first NUL or `width` bytes, two rows share an id iff their texts are equal, and the canonical value is
the text zero-filled to `width`.  Also the library's 64-bit hash restated (qsx_char_dict_hash), and a pair of distinct texts
that the slot table cannot tell apart without comparing bytes."""
import numpy as np

MIN_SLOTS = 16          # the smallest slot table (csrc/char_dict.hip kMinSlots)

_K1 = np.uint64(0x9E3779B97F4A7C15)
_K2 = np.uint64(0xD6E8FEB86659FD93)
_SEED = np.uint64(0x243F6A8885A308D3)

# Two CHAR(9) texts with the same fingerprint (high 32 bits of the hash) AND the same home slot in a table of MIN_SLOTS
# slots (low bits): found by collision_search(seed=1), proven by tests/test_char_dict_reference.py.
COLLISION_WIDTH = 9
COLLISION_PAIR = (b"sseamtun", b"erlqnpnw")


def lengths(col):
    """Length of every row's text."""
    col = np.asarray(col, dtype=np.uint8)
    n, width = col.shape
    is_nul = col == 0
    return np.where(is_nul.any(axis=1), is_nul.argmax(axis=1), width).astype(np.int64)


def canonical(col):
    """The stripe with everything behind a row's first NUL zero-filled."""
    col = np.asarray(col, dtype=np.uint8)
    keep = np.arange(col.shape[1])[None, :] < lengths(col)[:, None]
    return np.where(keep, col, 0).astype(np.uint8)


def intern(col, keep=None):
    """The partition of the rows by canonical text: labels int64[n], equal label iff equal text, -1 outside `keep`.
    Returns (labels, number of distinct texts among the kept rows)."""
    canon = canonical(col)
    n, width = canon.shape
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    labels = np.full(n, -1, dtype=np.int64)
    if keep.any():
        rows = np.ascontiguousarray(canon[keep]).view(np.dtype((np.void, width))).reshape(-1)
        uniq, inverse = np.unique(rows, return_inverse=True)
        labels[keep] = inverse.reshape(-1)
        return labels, int(uniq.size)
    return labels, 0


def same_partition(ids, labels):
    """ids[i] == ids[j] iff labels[i] == labels[j] (both -1 together): the map between them is a bijection."""
    ids = np.asarray(ids, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    if not np.array_equal(ids < 0, labels < 0):
        return False
    pairs = np.unique(np.stack([ids, labels], axis=1), axis=0)
    return pairs.shape[0] == np.unique(ids).size == np.unique(labels).size


def hash_texts(col):
    """qsx_char_dict_hash of every row, vectorised: the text as little-endian 64-bit words, zero-filled, one multiply-xorshift
    round per word that holds text, then the length."""
    canon = canonical(col)
    n, width = canon.shape
    length = lengths(col)
    words = (width + 7) // 8
    padded = np.zeros((n, words * 8), dtype=np.uint8)
    padded[:, :width] = canon
    w = padded.view("<u8").reshape(n, words)
    h = np.full(n, _SEED, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(words):
            r = (h ^ w[:, j]) * _K1
            r ^= r >> np.uint64(32)
            h = np.where(length > 8 * j, r, h)
        h = (h ^ length.astype(np.uint64)) * _K2
        h ^= h >> np.uint64(29)
        h *= _K1
        h ^= h >> np.uint64(32)
    return h


def fingerprint(h):
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32)


def home_slot(h, slots=MIN_SLOTS):
    return (np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF) & np.uint64(slots - 1)).astype(np.int64)


def field(text, width):
    """bytes -> one CHAR(width) row."""
    return np.frombuffer(bytes(text)[:width].ljust(width, b"\0"), dtype=np.uint8).copy()


def collision_search(seed, count=3_000_000, width=COLLISION_WIDTH):
    """A pair of distinct 8-letter texts with equal fingerprint and equal home slot at MIN_SLOTS, or None: 36 bits have to
    agree, `count` random texts hold about count^2 / 2^37 such pairs (65 for three million)."""
    rng = np.random.default_rng(seed)
    col = np.zeros((count, width), dtype=np.uint8)
    col[:, :8] = rng.integers(ord("a"), ord("z") + 1, size=(count, 8), dtype=np.uint8)
    h = hash_texts(col)
    key = (h >> np.uint64(32) << np.uint64(4)) | (h & np.uint64(MIN_SLOTS - 1))
    order = np.argsort(key, kind="stable")
    sorted_key = key[order]
    for at in np.nonzero(sorted_key[1:] == sorted_key[:-1])[0]:
        a, b = col[order[at]], col[order[at + 1]]
        if not np.array_equal(a, b):
            return bytes(a[:8]), bytes(b[:8])
    return None


def make_stripe(width, n, seed, values=None):
    """n fields of CHAR(width).  values=None: random short texts and full-width texts; else rows drawn from `values`
    (bytes objects).  Whatever lies behind a row's NUL is random: it must never take part."""
    rng = np.random.default_rng(seed)
    col = rng.integers(1, 256, size=(n, width), dtype=np.uint8)     # the tails
    if values is None:
        text = rng.integers(ord("a"), ord("e") + 1, size=(n, width), dtype=np.uint8)
        kind = rng.random(n)
        length = np.where(kind < 0.6, rng.integers(0, 4, size=n), np.where(kind < 0.9, rng.integers(0, 13, size=n), width))
        length = np.minimum(length, width)
    else:
        table = np.stack([field(v, width) for v in values])
        text = table[rng.integers(0, len(values), size=n)]
        length = lengths(text)
    inside = np.arange(width)[None, :] < length[:, None]
    col = np.where(inside, text, col)
    rows = np.nonzero(length < width)[0]
    col[rows, length[rows]] = 0
    return np.ascontiguousarray(col.astype(np.uint8))
