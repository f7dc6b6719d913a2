"""A plain reference of the K9 partition scatter (quickstep_amd/csrc/partition.hip) and the checkers of its results.

Shares no code with the oracle: numpy uint64 arithmetic (which wraps modulo 2^64) written from the definitions —

  key image   INT: the 32-bit pattern zero-extended; LONG: the 64-bit pattern; packed: OR_k (zero-extended value of width_k) << shift_k
  mix64(k)    k ^= k >> 32; k *= C; k ^= k >> 29          hash = mix64(k) * C          C = 0x9E3779B97F4A7C15
  partition   mode 0: image & (P - 1) for a power of two, else image % P
              mode 1: hash >> (64 - log2 P)
              mode 2: (image >> shift) & 63
              modes 3, 4: (hash >> shift) & 63
  offsets     the exclusive prefix of the partitions' row counts, offsets[P] = n
  pieces      pieces[p] = exclusive prefix of the counts rounded up to `align`, pieces[P + p] = the count

tests/test_partition_reference.py pins these forms against Python-integer arithmetic and shows that every checker rejects a
result that is wrong in one count, one row or one column; tests/test_gpu_partition_forms.py runs the kernels through them.

A checker takes the input columns, the outputs and the position `rid` of the row-id column (arange(n)) among them, and raises
AssertionError with what differs.
"""
import numpy as np

C = np.uint64(0x9E3779B97F4A7C15)
_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _bits(col):
    """The column's bit patterns, zero-extended to uint64."""
    col = np.ascontiguousarray(col)
    return col.view(_UNSIGNED[col.itemsize]).astype(np.uint64)


def key_image(keys):
    assert keys.itemsize in (4, 8)
    return _bits(keys)


def packed_image(key_cols, shifts):
    code = np.zeros(key_cols[0].size, dtype=np.uint64)
    for col, shift in zip(key_cols, shifts):
        code |= _bits(col) << np.uint64(shift)
    return code


def mix64(k):
    k = k.astype(np.uint64, copy=True)
    k ^= k >> np.uint64(32)
    k *= C
    k ^= k >> np.uint64(29)
    return k


def hash64(image):
    return mix64(image) * C


def partition_ids(mode, image, num_partitions=64, shift=0):
    """Partition of every row (int64) from the rows' key images."""
    P = int(num_partitions)
    if mode == 0:
        if P & (P - 1) == 0:
            return (image & np.uint64(P - 1)).astype(np.int64)
        return (image % np.uint64(P)).astype(np.int64)
    if mode == 1:
        log2p = P.bit_length() - 1
        assert 1 << log2p == P and log2p >= 1
        return (hash64(image) >> np.uint64(64 - log2p)).astype(np.int64)
    if mode == 2:
        return ((image >> np.uint64(shift)) & np.uint64(63)).astype(np.int64)
    assert mode in (3, 4)
    return ((hash64(image) >> np.uint64(shift)) & np.uint64(63)).astype(np.int64)


def hash_bits12(image, shift):
    """The 12 hash bits two passes at shift - 6 and shift order the rows by."""
    return ((hash64(image) >> np.uint64(shift - 6)) & np.uint64(4095)).astype(np.int64)


def offsets_of(pid, num_partitions):
    counts = np.bincount(pid, minlength=num_partitions).astype(np.int64)
    assert counts.size == num_partitions
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def pieces_of(pid, num_partitions, align):
    counts = np.bincount(pid, minlength=num_partitions).astype(np.int64)
    padded = (counts + align - 1) // align * align
    starts = np.cumsum(padded) - padded
    return np.concatenate([starts, counts]).astype(np.int64)


# ---- checkers ------------------------------------------------------------------------------------------------------------
def _row_ids(cols, outs, rid, n):
    assert len(cols) == len(outs) and 0 <= rid < len(cols)
    assert np.array_equal(cols[rid], np.arange(n, dtype=cols[rid].dtype)), "the row-id column is not arange(n)"
    for c, (col, out) in enumerate(zip(cols, outs)):
        assert out.dtype == col.dtype and out.shape == col.shape, f"column {c}: {out.dtype}{out.shape} for {col.dtype}{col.shape}"
    ids = outs[rid].astype(np.int64)
    bad = np.flatnonzero((ids < 0) | (ids >= n))
    assert bad.size == 0, f"row id out of range at output rows {bad[:5].tolist()}: {ids[bad[:5]].tolist()}"
    return ids


def _columns_follow(cols, outs, ids, rid):
    for c, (col, out) in enumerate(zip(cols, outs)):
        if c == rid:
            continue
        bad = np.flatnonzero(out != col[ids])
        assert bad.size == 0, f"column {c} does not hold its row's value at output rows {bad[:5].tolist()} (rows {ids[bad[:5]].tolist()})"


def _offsets_equal(got, want, what="offsets"):
    got = np.asarray(got)[:want.size]
    assert got.size == want.size and np.array_equal(got, want), \
        f"{what} differ at {np.flatnonzero(got != want)[:5].tolist()}: got {got[got != want][:5].tolist()}, want {want[got != want][:5].tolist()}"


def check_stable(pid, num_partitions, cols, outs, got_offsets, rid=0):
    """A stable partitioning: the row ids are argsort(pid, stable), every other column col[row ids]."""
    n = pid.size
    _offsets_equal(got_offsets, offsets_of(pid, num_partitions))
    ids = _row_ids(cols, outs, rid, n)
    order = np.argsort(pid, kind="stable")
    bad = np.flatnonzero(ids != order)
    assert bad.size == 0, f"row order differs at output rows {bad[:5].tolist()}: got rows {ids[bad[:5]].tolist()}, want {order[bad[:5]].tolist()}"
    _columns_follow(cols, outs, ids, rid)


def _sets_equal(group_of_row, ids, group_of_output):
    """Per group, the row ids in the output are the group's rows (each once): sorted inside the groups they are the stable order."""
    inside = ids[np.lexsort((ids, group_of_output))]
    order = np.argsort(group_of_row, kind="stable")
    bad = np.flatnonzero(inside != order)
    assert bad.size == 0, f"a group holds other rows than its own: first at sorted position {bad[:5].tolist()}, rows {inside[bad[:5]].tolist()} for {order[bad[:5]].tolist()}"


def check_partitioned(pid, num_partitions, cols, outs, got_offsets, rid=0):
    """A partitioning in any order inside a partition: per partition the set of row ids, columns consistent with the row ids."""
    n = pid.size
    want = offsets_of(pid, num_partitions)
    _offsets_equal(got_offsets, want)
    ids = _row_ids(cols, outs, rid, n)
    _sets_equal(pid, ids, np.repeat(np.arange(num_partitions), np.diff(want)))
    _columns_follow(cols, outs, ids, rid)


def check_second_digit(image, shift, cols, outs, got_offsets, rid=0):
    """The stable pass at `shift` over an input ordered by the digit at shift - 6 (image: the key images of that input): the
    output is ordered by the 12 hash bits from shift - 6 up, and holds per 12-bit value that value's rows."""
    n = image.size
    low = partition_ids(4, image, 64, shift - 6)
    assert np.all(np.diff(low) >= 0), "the input is not ordered by the digit below"
    _offsets_equal(got_offsets, offsets_of(partition_ids(3, image, 64, shift), 64))
    ids = _row_ids(cols, outs, rid, n)
    v12 = hash_bits12(image, shift)
    got = v12[ids]
    bad = np.flatnonzero(np.diff(got) < 0)
    assert bad.size == 0, f"not ordered by the 12 hash bits at output rows {bad[:5].tolist()}"
    _sets_equal(v12, ids, got)
    _columns_follow(cols, outs, ids, rid)


def check_pieces(pid, num_partitions, align, cols, outs, got_pieces, sentinels, stable, rid=0):
    """Aligned pieces: starts and counts, every output row outside a piece still holds its sentinel, and the pieces laid end to
    end are the partitioning (stable or not)."""
    P = num_partitions
    want = pieces_of(pid, P, align)
    _offsets_equal(got_pieces, want, "pieces (P starts, P counts)")
    starts, counts = want[:P], want[P:]
    rows_out = outs[0].shape[0]
    inside = np.zeros(rows_out, dtype=bool)
    for p in range(P):
        assert starts[p] + counts[p] <= rows_out
        inside[starts[p]:starts[p] + counts[p]] = True
    packed = []
    for c, (out, sentinel) in enumerate(zip(outs, sentinels)):
        assert out.shape[0] == rows_out
        bad = np.flatnonzero(~inside & (out != sentinel))
        assert bad.size == 0, f"column {c}: a write into a gap at output rows {bad[:5].tolist()}"
        packed.append(out[inside])
    (check_stable if stable else check_partitioned)(pid, P, cols, packed, offsets_of(pid, P), rid)
