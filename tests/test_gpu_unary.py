"""GPU: qsx_eval_date_extract / qsx_eval_substring and their run forms against tests/unary_reference.py, byte for byte.  Every
output lies in a buffer with 64 guard bytes of 0xA5 behind it (and its offset in front of it), which must come back unchanged:
exactly n * 4 or n * m bytes are written.  Sizes cover the kernels' edges (csrc/unary_ops.hip): an EXTRACT lane takes four
dates and a tile 2048 rows; a SUBSTRING tile holds min(1024, 48 KiB / (w + m) rounded down to 64) rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import unary_reference as R
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

GUARD = 64
EXTRACT_SIZES = (0, 1, 3, 63, 64, 65, 4 * 256 + 3, 100_003)
WIDTHS = (1, 2, 15, 25, 64, 255)
LENGTHS = (1, 2, 3, 7, "w", 300)
ROWS = (0, 1, 1023, 1024, 1025, 5000)
OFFSETS = (0, 1, 5)


def guarded(nbytes, offset, dev):
    """A buffer of 0xA5 with `nbytes` of payload `offset` bytes behind a 16-byte boundary and GUARD bytes behind the payload."""
    buf = torch.full((offset + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def check_guarded(buf, nbytes, offset, want, what):
    got = buf.cpu().numpy()
    assert np.all(got[:offset] == 0xA5), what + ": bytes in front of the output were written"
    assert np.all(got[offset + nbytes:] == 0xA5), what + ": bytes behind the output were written"
    assert np.array_equal(got[offset:offset + nbytes], np.ascontiguousarray(want).view(np.uint8).reshape(-1)), what


# ---------------------------------------------------------------------------------------------------------------- EXTRACT
_dates = {}


def dates(dev):
    """(raw int64 dates on the host, the same at a 16-byte boundary, the same 8 bytes behind one, years, months) — made once."""
    if not _dates:
        n = max(EXTRACT_SIZES)
        rng = np.random.default_rng(20240901)
        year = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64)
        year[::3] = rng.integers(1992, 1999, size=year[::3].size)          # TPC-H's
        year[1::7] = rng.integers(32768, 1 << 20, size=year[1::7].size)    # above 32 767
        year[2::11] = rng.integers(-5000, 0, size=year[2::11].size)        # negative
        month = rng.integers(1, 13, size=n)
        month[:24] = np.tile(np.arange(1, 13), 2)
        day = rng.integers(1, 32, size=n)
        padding = rng.integers(0, 1 << 16, size=n)                         # never looked at
        raw = (year & 0xFFFFFFFF) | (month << 32) | (day << 40) | (padding << 48)
        raw = raw.astype(np.uint64).view(np.int64)
        aligned = torch.from_numpy(raw).to(dev)
        shifted = torch.zeros(n + 3, dtype=torch.int64, device=dev)
        shifted[1:1 + n] = aligned
        assert aligned.data_ptr() % 16 == 0 and shifted[1:].data_ptr() % 16 == 8
        want = {T.DATE_YEAR: R.date_extract(R.DATE_YEAR, raw), T.DATE_MONTH: R.date_extract(R.DATE_MONTH, raw)}
        assert np.array_equal(want[T.DATE_YEAR], year.astype(np.int32)) and np.array_equal(want[T.DATE_MONTH], month.astype(np.int32))
        assert (want[T.DATE_YEAR] < 0).any() and (want[T.DATE_YEAR] > 32767).any()
        _dates["all"] = (raw, aligned, shifted[1:1 + n], want)
    return _dates["all"]


@pytest.mark.parametrize("unit", (T.DATE_YEAR, T.DATE_MONTH), ids=("year", "month"))
def test_date_extract_matches_the_reference(capi, dev, unit):
    raw, aligned, shifted, want = dates(dev)
    pending = []
    for n in EXTRACT_SIZES:
        # the stripe at a 16-byte boundary and 8 bytes behind one; the output at every 4-byte phase of 16 bytes
        for stripe, out_offset in ((aligned, 0), (shifted, 0), (aligned, 4), (shifted, 12), (shifted, 8)):
            if out_offset not in (0, 4) and n not in (65, 4 * 256 + 3):
                continue
            buf = guarded(4 * n, out_offset, dev)
            out = buf[out_offset:out_offset + 4 * n].view(torch.int32)
            got = capi.eval_date_extract(unit, stripe[:n], out=out)
            assert got.data_ptr() == out.data_ptr()
            pending.append((buf, 4 * n, out_offset, want[unit][:n], "n=%d stripe%%16=%d out%%16=%d" % (n, stripe.data_ptr() % 16, out_offset)))
    for buf, nbytes, offset, expected, what in pending:
        check_guarded(buf, nbytes, offset, expected, what)


def test_date_extract_blocks_gives_the_answers_of_single_calls(capi, dev):
    raw, aligned, shifted, want = dates(dev)
    cuts = [(0, 1025), (1025, 1025), (1025, 1042)]       # 1025, 0 and 17 rows; the third block starts 8 mod 16
    for unit in (T.DATE_YEAR, T.DATE_MONTH):
        blocks = [aligned[a:b] for a, b in cuts]
        assert blocks[2].data_ptr() % 16 == 8
        bufs = [guarded(4 * (b - a), 0, dev) for a, b in cuts]
        outs = [buf[:4 * (b - a)].view(torch.int32) for buf, (a, b) in zip(bufs, cuts)]
        capi.eval_date_extract_blocks(unit, blocks, outs=outs)
        for buf, (a, b), block in zip(bufs, cuts, blocks):
            check_guarded(buf, 4 * (b - a), 0, want[unit][a:b], "block %d..%d" % (a, b))
            assert torch.equal(buf[:4 * (b - a)].view(torch.int32), capi.eval_date_extract(unit, block))
    assert capi.eval_date_extract_blocks(T.DATE_YEAR, []) == []


def test_date_extract_blocks_small_then_large_table_on_one_stream(capi, dev):
    """3 blocks, then 2000 blocks of 1..5 rows (a run table of ~96 KB: beyond the first 64 KiB of the stream's staging
    buffer, which is regrown between two calls), then 3 blocks again, all on one stream that no call has used before."""
    raw, aligned, shifted, want = dates(dev)
    rng = np.random.default_rng(7)
    small = np.array([0, 700, 705, 1800])
    large = np.concatenate(([0], np.cumsum(rng.integers(1, 6, size=2000))))
    runs = []
    for bounds in (small, large, small + 3):
        first, last = int(bounds[0]), int(bounds[-1])
        out = torch.full((last - first + GUARD // 4,), -1, dtype=torch.int32, device=dev)
        pairs = list(zip(bounds[:-1].tolist(), bounds[1:].tolist()))
        runs.append((out, first, last, [aligned[a:b] for a, b in pairs], [out[a - first:b - first] for a, b in pairs]))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for out, first, last, blocks, outs in runs:
        capi.eval_date_extract_blocks(T.DATE_YEAR, blocks, outs=outs, stream=stream)
    stream.synchronize()
    for out, a, b, _, _ in runs:
        got = out.cpu().numpy()
        assert np.array_equal(got[:b - a], want[T.DATE_YEAR][a:b]), "rows %d..%d" % (a, b)
        assert np.all(got[b - a:] == -1), "rows behind the output were written"


# -------------------------------------------------------------------------------------------------------------- SUBSTRING
ALPHABET = np.frombuffer(b"ab-0123456789 \x80\xc3\xff", dtype=np.uint8)


def make_stripe(width, n, seed):
    """n fields of CHAR(width): empty texts, short texts with a random tail behind the NUL (which must never take part), and
    texts that fill all `width` bytes without a NUL; bytes >= 0x80 among them."""
    rng = np.random.default_rng(seed)
    col = ALPHABET[rng.integers(0, ALPHABET.size, size=(n, width))]
    kind = rng.random(n)
    length = np.where(kind < 0.15, 0, np.where(kind < 0.65, rng.integers(0, width + 1, size=n), width))
    length[:4] = (0, width, max(width - 1, 0), min(1, width))
    rows = np.nonzero(length < width)[0]
    col[rows, length[rows]] = 0
    return np.ascontiguousarray(col), length


def substring_tile_rows(width, m):
    return max(64, min(1024, (48 * 1024 // (width + m)) // 64 * 64))


def combinations():
    """About 40 (width, start, length, rows, input offset, output offset): every value of every parameter occurs, for every
    width every valid start of {0, 1, w - 1}."""
    out = []
    for width in WIDTHS:
        for start in sorted({s for s in (0, 1, width - 1) if 0 <= s < width}):
            for _ in range(3 if width > 2 else 4):
                i = len(out)                              # the parameters advance at different paces, so that they mix
                length = LENGTHS[i % 6]
                out.append((width, start, width if length == "w" else length, ROWS[(i + i // 6) % 6], OFFSETS[(i + i // 3) % 3],
                            OFFSETS[(i // 2 + i // 7) % 3]))
    return out


COMBINATIONS = combinations()


def test_the_combinations_cover_every_value():
    assert 35 <= len(COMBINATIONS) <= 50
    assert {c[0] for c in COMBINATIONS} == set(WIDTHS)
    assert {c[3] for c in COMBINATIONS} == set(ROWS)
    assert {c[4] for c in COMBINATIONS} == set(OFFSETS) == {c[5] for c in COMBINATIONS}
    for width in WIDTHS:
        assert {c[1] for c in COMBINATIONS if c[0] == width} == {s for s in (0, 1, width - 1) if s < width}
    assert {1, 2, 3, 7, 300} <= {c[2] for c in COMBINATIONS} and any(c[2] == c[0] for c in COMBINATIONS)


@pytest.mark.parametrize("width", WIDTHS)
def test_substring_matches_the_reference(capi, dev, width):
    col, length = make_stripe(width, max(ROWS), seed=500 + width)
    flat = torch.from_numpy(col.reshape(-1)).to(dev)
    stripes = {}
    for off in OFFSETS:                                   # the stripe 0, 1 and 5 bytes behind a 16-byte boundary
        holder = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device=dev)
        holder[off:off + flat.numel()] = flat
        assert holder.data_ptr() % 16 == 0
        stripes[off] = holder
    pending, classes = [], set()
    for w, start, sub_length, n, in_off, out_off in COMBINATIONS:
        if w != width:
            continue
        m = R.substring_width(w, start, sub_length)
        stripe = stripes[in_off][in_off:in_off + n * w].reshape(n, w)
        buf = guarded(n * m, out_off, dev)
        out = buf[out_off:out_off + n * m].reshape(n, m)
        capi.eval_substring(stripe, start, sub_length, out=out)
        want = R.substring_fast(col[:n], start, sub_length)
        pending.append((buf, n * m, out_off, want, "w=%d start=%d length=%d n=%d in%%16=%d out%%16=%d" % (w, start, sub_length, n, in_off, out_off)))
        if n >= 1023:                                     # the text classes this window meets
            lens = length[:n]
            classes |= {"empty"} if (lens == 0).any() else set()
            classes |= {"ends before start"} if ((lens > 0) & (lens <= start)).any() and start > 0 else set()
            classes |= {"ends inside the window"} if ((lens > start) & (lens < start + m)).any() else set()
            classes |= {"fills the field"} if (lens == w).any() else set()
            classes |= {"high byte in the window"} if (want >= 0x80).any() else set()
    assert pending
    for buf, nbytes, offset, expected, what in pending:
        check_guarded(buf, nbytes, offset, expected, what)
    needed = {"empty", "fills the field", "high byte in the window"}
    if width > 2:
        needed |= {"ends before start", "ends inside the window"}
    assert needed <= classes, (width, needed - classes)


def test_substring_rows_against_the_row_by_row_reference(capi, dev):
    """CHAR(15) -> 2 (TPC-H Q22) and an odd window over more than one tile, against the row-by-row restatement."""
    col, _ = make_stripe(15, 2100, seed=77)
    for start, sub_length in ((0, 2), (4, 7)):
        got = capi.eval_substring(torch.from_numpy(col).to(dev), start, sub_length)
        assert np.array_equal(got.cpu().numpy(), R.substring(col, start, sub_length)), (start, sub_length)


def test_substring_blocks_gives_the_answers_of_single_calls(capi, dev):
    for width, start, sub_length, in_off, out_off in ((15, 0, 2, 0, 0), (25, 1, 7, 1, 5), (255, 254, 3, 5, 1)):
        col, _ = make_stripe(width, 1025 + 17, seed=900 + width)
        m = R.substring_width(width, start, sub_length)
        cuts = [(0, 1025), (1025, 1025), (1025, 1042)]   # 1025, 0 and 17 rows
        holders, blocks, bufs, outs = [], [], [], []
        for a, b in cuts:
            holder = torch.zeros((b - a) * width + 16, dtype=torch.uint8, device=dev)
            holder[in_off:in_off + (b - a) * width] = torch.from_numpy(col[a:b].reshape(-1)).to(dev)
            holders.append(holder)
            blocks.append(holder[in_off:in_off + (b - a) * width].reshape(b - a, width))
            bufs.append(guarded((b - a) * m, out_off, dev))
            outs.append(bufs[-1][out_off:out_off + (b - a) * m].reshape(b - a, m))
        capi.eval_substring_blocks(blocks, start, sub_length, outs=outs)
        for buf, (a, b), block in zip(bufs, cuts, blocks):
            check_guarded(buf, (b - a) * m, out_off, R.substring_fast(col[a:b], start, sub_length), "w=%d block %d..%d" % (width, a, b))
            single = capi.eval_substring(block, start, sub_length)
            assert torch.equal(buf[out_off:out_off + (b - a) * m].reshape(b - a, m), single)


def test_argument_checks(capi, dev):
    lib = capi.lib
    dates_dev = torch.zeros(8, dtype=torch.int64, device=dev)
    years = torch.zeros(8, dtype=torch.int32, device=dev)
    col = torch.zeros((8, 15), dtype=torch.uint8, device=dev)
    out = torch.zeros((8, 15), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d, y, c, o = (C.c_void_p(t.data_ptr()) for t in (dates_dev, years, col, out))
    for unit in (2, 3, 4, 5, -1):                                          # DAY / HOUR / MINUTE / SECOND belong to Datetime
        assert lib.qsx_eval_date_extract(unit, d, 8, y, stream) == T.ERR_UNSUPPORTED
    assert lib.qsx_eval_date_extract(T.DATE_YEAR, d, -1, y, stream) == T.ERR_INVALID_ARGUMENT
    assert lib.qsx_eval_date_extract(T.DATE_YEAR, None, 8, y, stream) == T.ERR_INVALID_ARGUMENT
    assert lib.qsx_eval_date_extract(T.DATE_YEAR, None, 0, None, stream) == T.OK
    assert lib.qsx_eval_date_extract_blocks(T.DATE_YEAR, 0, None, None, None, stream) == T.OK
    assert lib.qsx_eval_date_extract_blocks(T.DATE_YEAR, -1, None, None, None, stream) == T.ERR_INVALID_ARGUMENT
    for width, start, length in ((15, -1, 2), (15, 15, 2), (15, 0, 0), (15, 0, -3), (0, 0, 1), (256, 0, 1)):
        assert lib.qsx_eval_substring(c, width, 8, start, length, o, stream) == T.ERR_INVALID_ARGUMENT, (width, start, length)
        assert lib.qsx_eval_substring_blocks(width, 0, None, None, start, length, None, stream) == T.ERR_INVALID_ARGUMENT
    assert lib.qsx_eval_substring(None, 15, 8, 0, 2, o, stream) == T.ERR_INVALID_ARGUMENT
    assert lib.qsx_eval_substring(None, 15, 0, 0, 2, None, stream) == T.OK
    assert lib.qsx_eval_substring_blocks(15, 0, None, None, 0, 2, None, stream) == T.OK
    torch.cuda.synchronize()
    assert int(years.abs().sum().item()) == 0 and int(out.sum().item()) == 0   # a refused call writes nothing
