"""qsx_join_table_clear and the pair counter of a probe after it.

A directly addressed table is cleared by one kernel (head[] and the control words), and the probe that packs the table has the
pack kernel reset its pair counter; a table too small to be packed and a hashed table keep the counter's memset.  On every path
a caller may reuse `out` without resetting its count word: the count and the pairs are those of the table as rebuilt."""
import numpy as np
import pytest
import torch

from helpers import to_dev
from quickstep_amd import types as T

pytestmark = pytest.mark.gpu

# (key range of the build side or None = hashed table): a range whose 4-byte head[] is beyond 3.25 MiB and whose 3-byte copy is
# below 3.6 MiB is packed by the first probe after a build (sealed_pack in csrc/join.hip); 10 000 key values are not
TABLES = {"packed": 900_001, "too_small_to_pack": 10_000, "hashed": None}
BUILD_ROWS, PROBE_ROWS = 3_001, 5_003


def reference_pairs(probe, build):
    p, b = np.nonzero(probe[:, None] == build[None, :])
    return np.stack([p, b], 1)


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("kind", list(TABLES))
def test_clear_rebuild_probe_with_a_reused_out(capi, dev, kind):
    span = TABLES[kind]
    domain = span if span is not None else 50_000
    rng = np.random.default_rng(len(kind))
    table = capi.JoinTable(T.INT, BUILD_ROWS, key_range=None if span is None else (0, span - 1))
    out = (torch.empty(4 * PROBE_ROWS, dtype=torch.int32, device=dev), torch.empty(4 * PROBE_ROWS, dtype=torch.int32, device=dev),
           torch.full((1,), 0x0BADC0DE, dtype=torch.int64, device=dev))
    table.build(to_dev(rng.integers(0, domain, size=BUILD_ROWS).astype(np.int32), dev))
    assert table.size() == BUILD_ROWS
    for attempt in range(2):
        table.clear()
        assert table.size() == 0
        # other keys than before, some of them twice; the probe side draws half of its keys from the build side
        build = rng.integers(0, domain, size=BUILD_ROWS).astype(np.int32)
        build[-200:] = build[:200]
        probe = np.where(rng.random(PROBE_ROWS) < 0.5, rng.choice(build, size=PROBE_ROWS), rng.integers(0, domain, size=PROBE_ROWS)).astype(np.int32)
        table.build(to_dev(build, dev))
        assert table.size() == BUILD_ROWS
        want = reference_pairs(probe, build)
        assert 0 < want.shape[0] <= out[0].numel()
        _, _, count = table.probe(to_dev(probe, dev), out=out)          # the count word still holds the previous probe's count
        got_count = int(count.item())
        assert got_count == want.shape[0], f"attempt {attempt}: {got_count} pairs, want {want.shape[0]}"
        got = np.stack([out[0].cpu().numpy()[:got_count], out[1].cpu().numpy()[:got_count]], 1)
        assert np.array_equal(sorted_rows(got), sorted_rows(want)), f"attempt {attempt}: wrong pairs"
    table.clear()
    assert table.size() == 0
