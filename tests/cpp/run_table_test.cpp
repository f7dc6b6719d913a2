// run_table_test.cpp — the host side of a run table (quickstep_amd/csrc/run_table.hpp) against a plain loop: the tile index
// (first_tile[], the tile total, the `uniform` shortcut that the kernels' run_locate divides by), the named array
// positions, the coding arrays and the words a caller appends.  No device: run_locate is redone here on the host table, once
// by the division and once by the binary search, exactly as block_runs.hpp does it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../quickstep_amd/csrc/run_table.hpp"

using qsx::RunTable;

static int g_failures = 0;
#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_case); \
      ++g_failures;                                                                       \
    }                                                                                     \
  } while (0)
static const char *g_case = "";

// the layout the kernels read (block_runs.hpp): these numbers are the device ABI of the table
static_assert(qsx::kRunHeaderWords == 4, "header words");
static_assert(qsx::kRunRows == 0 && qsx::kRunIn == 1 && qsx::kRunFilter == 2 && qsx::kRunOut == 3 && qsx::kRunBase == 4 &&
                  qsx::kRunCodeWidth == 5 && qsx::kRunDictionary == 6,
              "array positions");

struct Located {
  int block, tile_in_block;
};
// run_locate of block_runs.hpp, its two branches apart
static Located locate_by_division(const long long *table, int tile) {
  const int uniform = static_cast<int>(table[1]);
  const int b = static_cast<int>(static_cast<unsigned>(tile) / static_cast<unsigned>(uniform));
  return Located{b, tile - b * uniform};
}
static Located locate_by_search(const long long *table, int tile) {
  const int nb = static_cast<int>(table[0]);
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[4 + mid] <= tile) lo = mid; else hi = mid - 1;
  }
  return Located{lo, tile - static_cast<int>(table[4 + lo])};
}

// header, first_tile[] and rows[] of `table` against a plain loop over `rows`; every tile located both ways
static void check_index(const long long *table, long long tiles, long long tile_rows, const std::vector<int64_t> &rows) {
  const size_t nb = rows.size();
  std::vector<long long> block_tiles(nb), first(nb + 1, 0);
  for (size_t b = 0; b < nb; ++b) {
    block_tiles[b] = rows[b] / tile_rows + (rows[b] % tile_rows != 0 ? 1 : 0);
    first[b + 1] = first[b] + block_tiles[b];
  }
  bool same = block_tiles[0] > 0 && block_tiles[nb - 1] <= block_tiles[0];
  for (size_t b = 1; b + 1 < nb; ++b) same = same && block_tiles[b] == block_tiles[0];
  const long long uniform = same ? block_tiles[0] : 0;

  CHECK(tiles == first[nb]);
  CHECK(table[0] == static_cast<long long>(nb));
  CHECK(table[1] == uniform);
  CHECK(table[2] == first[nb]);
  for (size_t b = 0; b <= nb; ++b) CHECK(table[4 + b] == first[b]);
  for (size_t b = 0; b < nb; ++b) CHECK(table[4 + (nb + 1) + b] == rows[b]);
  int tile = 0;
  for (size_t b = 0; b < nb; ++b) {
    for (long long t = 0; t < block_tiles[b]; ++t, ++tile) {
      const Located s = locate_by_search(table, tile);
      CHECK(s.block == static_cast<int>(b) && s.tile_in_block == t);
      if (table[1] > 0) {
        const Located d = locate_by_division(table, tile);
        CHECK(d.block == static_cast<int>(b) && d.tile_in_block == t);
      }
    }
  }
}

static void check_run(const char *name, long long tile_rows, const std::vector<int64_t> &rows, int expect_uniform /* -1: any */) {
  g_case = name;
  const size_t nb = rows.size();
  const long long header = 4 + static_cast<long long>(nb) + 1;
  std::vector<const void *> in(nb), filters(nb), dictionaries(nb);
  std::vector<void *> out(nb);
  std::vector<int64_t> base(nb);
  std::vector<int32_t> widths(nb);
  for (size_t b = 0; b < nb; ++b) {
    in[b] = reinterpret_cast<const void *>(0x10000 + 16 * b);
    filters[b] = reinterpret_cast<const void *>(0x20000 + 16 * b);
    out[b] = reinterpret_cast<void *>(0x30000 + 16 * b);
    base[b] = 1000 + static_cast<int64_t>(b);
    widths[b] = b % 2 == 0 ? 2 : 0;
    dictionaries[b] = b % 2 == 0 ? reinterpret_cast<const void *>(0x40000 + 16 * b) : nullptr;
  }
  for (int coded = 0; coded < 2; ++coded) {
    RunTable table;
    const long long tiles = table.build(tile_rows, static_cast<long long>(nb), rows.data(), in.data(), filters.data(), out.data(), base.data(),
                                        coded ? widths.data() : nullptr, coded ? dictionaries.data() : nullptr);
    const long long *t = table.words();
    check_index(t, tiles, tile_rows, rows);
    if (expect_uniform >= 0) CHECK((t[1] != 0) == (expect_uniform != 0));
    // the coding arrays are there exactly when a coding is passed, and header word 3 says so
    CHECK(t[3] == coded);
    CHECK(static_cast<long long>(table.size()) == header + (coded ? 7 : 5) * static_cast<long long>(nb));
    for (size_t b = 0; b < nb; ++b) {
      const long long nbl = static_cast<long long>(nb), bl = static_cast<long long>(b);
      CHECK(t[header + qsx::kRunRows * nbl + bl] == rows[b]);
      CHECK(t[header + qsx::kRunIn * nbl + bl] == 0x10000 + 16 * bl);
      CHECK(t[header + qsx::kRunFilter * nbl + bl] == 0x20000 + 16 * bl);
      CHECK(t[header + qsx::kRunOut * nbl + bl] == 0x30000 + 16 * bl);
      CHECK(t[header + qsx::kRunBase * nbl + bl] == 1000 + bl);
      CHECK(QSX_RUN_WORD(nbl, qsx::kRunBase, bl) == header + 4 * nbl + bl);
      if (coded) {
        CHECK(t[header + qsx::kRunCodeWidth * nbl + bl] == widths[b]);
        CHECK(t[header + qsx::kRunDictionary * nbl + bl] == (b % 2 == 0 ? 0x40000 + 16 * bl : 0));
      }
    }
    // appended words sit at the returned offset, behind everything before them
    const long long before = static_cast<long long>(table.size());
    const long long three[3] = {7, 8, 9};
    const long long at = table.append(3, three);
    const long long zeros = table.append(2);
    CHECK(at == before && zeros == before + 3 && static_cast<long long>(table.size()) == before + 5);
    CHECK(table.words()[at] == 7 && table.words()[at + 1] == 8 && table.words()[at + 2] == 9);
    CHECK(table.words()[zeros] == 0 && table.words()[zeros + 1] == 0);
    check_index(table.words(), tiles, tile_rows, rows);   // (the index did not move)
  }
  {   // absent arrays stay 0
    RunTable table;
    table.build(tile_rows, static_cast<long long>(nb), rows.data(), in.data(), nullptr, nullptr, nullptr);
    for (size_t b = 0; b < nb; ++b) {
      for (int position = qsx::kRunFilter; position <= qsx::kRunBase; ++position) {
        CHECK(table.words()[header + position * static_cast<long long>(nb) + static_cast<long long>(b)] == 0);
      }
    }
  }
  {   // the index-only form (the CASE run: its own pointer sets of kSet words per block behind rows[])
    constexpr size_t kSet = 11;
    RunTable table;
    const long long tiles = table.index(tile_rows, static_cast<long long>(nb), rows.data(), kSet);
    check_index(table.words(), tiles, tile_rows, rows);
    CHECK(table.words()[3] == 0);
    CHECK(table.size() == static_cast<size_t>(header) + nb + kSet * nb);
    CHECK(table.at(qsx::kRunIn) == table.words() + header + static_cast<long long>(nb));
    for (size_t w = static_cast<size_t>(header) + nb; w < table.size(); ++w) CHECK(table.words()[w] == 0);
  }
}

int main() {
  for (const long long T : {64ll, 2048ll}) {
    check_run("a single block", T, {5 * T + 3}, 1);
    check_run("four equal blocks", T, {3 * T, 3 * T, 3 * T, 3 * T}, 1);
    check_run("a shorter last block", T, {3 * T, 3 * T - 1, 2 * T + 1, T + 1}, 1);
    check_run("a longer last block", T, {2 * T, 2 * T, 2 * T, 2 * T + 1}, 0);
    check_run("unequal blocks in the middle", T, {2 * T, 5 * T - 1, 2 * T, 2 * T}, 0);
    check_run("zero-row blocks in the middle and at the end", T, {2 * T, 0, 2 * T, 0}, 0);
    check_run("all blocks empty", T, {0, 0, 0}, 0);
    {
      g_case = "too many tiles";
      const std::vector<int64_t> rows = {0x40000000ll * T, 0x40000000ll * T};   // 2^31 tiles
      const std::vector<const void *> in(2, nullptr);
      RunTable table;
      CHECK(table.build(T, 2, rows.data(), in.data(), nullptr, nullptr, nullptr) == -1);
      CHECK(table.index(T, 2, rows.data(), 3) == -1);
      const std::vector<int64_t> fits = {0x40000000ll * T, (0x3FFFFFF0ll) * T};   // exactly the limit
      CHECK(table.index(T, 2, fits.data(), 0) == 0x7FFFFFF0ll);
    }
  }
  {   // the argument checks of the `_blocks` entry points
    g_case = "argument checks";
    const int64_t rows[3] = {4, 0, 2};
    const void *const p = &g_failures;
    const void *present[3] = {p, nullptr, p}, *missing[3] = {p, p, nullptr};
    CHECK(qsx::run_blocks_ok(3, rows, present, present));
    CHECK(qsx::run_blocks_ok(3, rows, nullptr, nullptr));
    CHECK(!qsx::run_blocks_ok(3, rows, missing, present));
    CHECK(!qsx::run_blocks_ok(3, rows, present, missing));
    const int64_t negative[2] = {1, -1};
    CHECK(!qsx::run_blocks_ok(2, negative, nullptr, nullptr));
    bool any = true;
    const int32_t plain[3] = {0, 0, 0}, mixed[3] = {0, 4, 1}, bad[3] = {0, 3, 0};
    const void *dict_on_values[3] = {p, nullptr, nullptr}, *dicts[3] = {nullptr, p, nullptr};
    CHECK(qsx::run_code_widths_ok(3, plain, nullptr, &any) && !any);
    CHECK(qsx::run_code_widths_ok(3, mixed, dicts, &any) && any);
    CHECK(!qsx::run_code_widths_ok(3, bad, nullptr, &any));
    CHECK(!qsx::run_code_widths_ok(3, mixed, dict_on_values, &any));
  }
  if (g_failures == 0) {
    std::printf("[  PASSED  ] run_table_test\n");
    return 0;
  }
  std::printf("[  FAILED  ] run_table_test (%d failures)\n", g_failures);
  return 1;
}
