// run_table.hpp — the layout of a run table (block_runs.hpp says what it is for) and the host code that builds one.
// No HIP here: the device accessors of block_runs.hpp and the host entry points share the positions below, and
// tests/cpp/run_table_test.cpp checks the builder with plain g++.
//
// Table (64-bit words):
//   [0] number of blocks   [1] tiles per block when every block but the last has the same number of tiles, else 0
//   [2] tiles in the run   [3] 1 when the coding arrays are present, else 0
//   first_tile[nb + 1], then one array of nb words per RunArray position, then whatever the caller appended.
#ifndef QSX_CSRC_RUN_TABLE_HPP_
#define QSX_CSRC_RUN_TABLE_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

namespace qsx {

constexpr int kRunHeaderWords = 4;
constexpr long long kRunMaxTiles = 0x7FFFFFF0ll;   // tile numbers are 32-bit on the device

// The per-block arrays behind first_tile[], in the order they lie.  in / filter / out / dictionary are device addresses
// (0 = absent), base is a row number added to emitted tuple ids, code_width is 0 / 1 / 2 / 4.
enum RunArray { kRunRows = 0, kRunIn, kRunFilter, kRunOut, kRunBase, kRunCodeWidth, kRunDictionary };
constexpr int kRunPlainArrays = kRunBase + 1, kRunCodedArrays = kRunDictionary + 1;

// Word of block b in array `position` of a table over nb blocks.  A macro, so that the device accessors expand to the very
// expression they were written as (an inline function leaves the kernels a different order of the same additions).
#define QSX_RUN_WORD(nb, position, b) (::qsx::kRunHeaderWords + ((nb) + 1) + (position) * (nb) + (b))

// Table word [1]: what run_locate divides a tile number by.  Every block but the last has that many tiles and the last no
// more (a longer last block would spill into a block that does not exist); 0 when the blocks differ or hold no tiles.
template <typename Rows>
inline long long run_uniform_tiles(long long tile_rows, size_t nb, const Rows *rows) {
  if (nb == 0) return 0;
  const long long per_block = (rows[0] + tile_rows - 1) / tile_rows;
  for (size_t b = 1; b < nb; ++b) {
    const long long bt = (rows[b] + tile_rows - 1) / tile_rows;
    if (b + 1 < nb ? bt != per_block : bt > per_block) return 0;
  }
  return per_block;
}

// Per-block arguments of a `_blocks` entry point: no negative row count, and where a block holds rows its input and its
// output are there (in / out == nullptr: the entry point has no such array).
inline bool run_blocks_ok(long long nb, const int64_t *rows, const void *const *in, const void *const *out) {
  for (long long b = 0; b < nb; ++b) {
    if (rows[b] < 0) return false;
    if (rows[b] > 0 && ((in != nullptr && in[b] == nullptr) || (out != nullptr && out[b] == nullptr))) return false;
  }
  return true;
}
// Code widths of key stripes: 0 (values) / 1 / 2 / 4, and no dictionary where the stripe holds values.  *any_coded: some
// stripe is coded (when none is, the run is the plain one).
inline bool run_code_widths_ok(long long n, const int32_t *widths, const void *const *dictionaries, bool *any_coded) {
  *any_coded = false;
  for (long long e = 0; e < n; ++e) {
    const int w = widths[e];
    if (w != 0 && w != 1 && w != 2 && w != 4) return false;
    if (w == 0 && dictionaries != nullptr && dictionaries[e] != nullptr) return false;
    *any_coded = *any_coded || w != 0;
  }
  return true;
}

class RunTable {
 public:
  // Header, first_tile[] and rows[] of a run whose tiles hold tile_rows rows, and `arrays` zeroed per-block arrays behind
  // rows[].  Returns the number of tiles (0: nothing to do), -1 when the run is too long for 32-bit tile numbers.
  long long index(long long tile_rows, long long num_blocks, const int64_t *rows, size_t arrays) {
    const size_t nb = static_cast<size_t>(num_blocks);
    nb_ = num_blocks;
    words_.assign(static_cast<size_t>(QSX_RUN_WORD(num_blocks, kRunIn, 0)) + arrays * nb, 0);
    long long *first = words_.data() + kRunHeaderWords, *t_rows = at(kRunRows);
    long long tiles = 0;
    for (size_t b = 0; b < nb; ++b) {
      first[b] = tiles;
      tiles += (rows[b] + tile_rows - 1) / tile_rows;
      t_rows[b] = rows[b];
    }
    first[nb] = tiles;
    words_[0] = num_blocks;
    words_[1] = run_uniform_tiles(tile_rows, nb, rows);
    words_[2] = tiles;
    return tiles > kRunMaxTiles ? -1 : tiles;
  }
  // The standard table.  filters / out / base may be nullptr.  code_widths != nullptr: a run of key stripes with their
  // coding (dictionaries may be nullptr, and so may its entries: truncated values).
  long long build(long long tile_rows, long long num_blocks, const int64_t *rows, const void *const *in, const void *const *filters,
                  void *const *out, const int64_t *base, const int32_t *code_widths = nullptr, const void *const *dictionaries = nullptr) {
    const long long tiles = index(tile_rows, num_blocks, rows, (code_widths != nullptr ? kRunCodedArrays : kRunPlainArrays) - 1);
    for (long long b = 0; b < num_blocks; ++b) {
      at(kRunIn)[b] = word_of(in[b]);
      if (filters != nullptr) at(kRunFilter)[b] = word_of(filters[b]);
      if (out != nullptr) at(kRunOut)[b] = word_of(out[b]);
      if (base != nullptr) at(kRunBase)[b] = base[b];
      if (code_widths != nullptr) {
        at(kRunCodeWidth)[b] = code_widths[b];
        if (dictionaries != nullptr) at(kRunDictionary)[b] = word_of(dictionaries[b]);
      }
    }
    words_[3] = code_widths != nullptr ? 1 : 0;
    return tiles;
  }
  // n more words behind everything so far (copied from src, or zero for the caller to fill through words()); returns
  // their word offset: the kernel finds them at table + offset, the host at dev() + offset.
  long long append(size_t n, const long long *src = nullptr) {
    const size_t offset = words_.size();
    if (src != nullptr) words_.insert(words_.end(), src, src + n);
    else words_.resize(offset + n, 0);
    return static_cast<long long>(offset);
  }
  static long long word_of(const void *p) { return static_cast<long long>(reinterpret_cast<uintptr_t>(p)); }
  long long *at(int position) { return words_.data() + QSX_RUN_WORD(nb_, position, 0); }   // array `position`, or what lies there
  long long *words() { return words_.data(); }
  size_t size() const { return words_.size(); }
  // The whole table into the stream's staging buffer (common.hpp staged_table: one per call and stream, so everything
  // the call's kernels read was appended first).  Defined in block_runs.hpp, where HIP is; `stream` is a hipStream_t.
  int upload(void *stream);
  const long long *dev() const { return dev_; }

 private:
  std::vector<long long> words_;
  long long nb_ = 0;
  const long long *dev_ = nullptr;
};

}  // namespace qsx

#endif  // QSX_CSRC_RUN_TABLE_HPP_
