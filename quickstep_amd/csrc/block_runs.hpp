// block_runs.hpp — a run of storage blocks presented to ONE launch of a tile-walking kernel (K1 select, K4 probe).
//
// The reference hands an operator one work order per block (RelationalOperator::getAllWorkOrders,
// relational_operators/RelationalOperator.hpp:117-119; SelectOperator.cpp:83-150, HashJoinOperator.cpp:203-260); at its
// 2-4 MB blocks a launch per block is launch-bound by an order of magnitude on this device (DESIGN.md "Work-order
// granularity").  A run keeps every block's own stripes / bitmaps where they are and gives the kernel a table to find
// them: the kernel walks the tiles of the whole run, a tile never straddles two blocks.
//
// The table lies in device memory as 64-bit words and is read through the kernel's `const __restrict__` argument with
// workgroup- or wave-uniform indices, i.e. scalar loads.  run_table.hpp names its words — the header, first_tile[], the
// per-block arrays rows | in | filter | out | base and, for a run of JOIN KEY stripes some of which are compressed,
// code_width | dictionary — and builds it on the host (RunTable: the tile index, the standard arrays, words the caller
// appends, the upload); the accessors below read it by the same names.
//
// Coded key stripes (storage/CompressedColumnStoreTupleStorageSubBlock.cpp, CompressedTupleStorageSubBlock.hpp:225-300
// getAttributeValue): the reference compresses every block on its own — an INT / LONG attribute of one block may lie as
// values, as 1 / 2 / 4-byte truncated values, or as 1 / 2 / 4-byte codes into the block's own sorted dictionary.  A block of
// the run with code_width != 0 presents that stripe as it lies; the kernels read the code and widen it (truncation) or look
// it up in the block's dictionary (a few KB, read through L2), per tile — a tile never straddles two blocks.
#ifndef QSX_CSRC_BLOCK_RUNS_HPP_
#define QSX_CSRC_BLOCK_RUNS_HPP_

#include "device_common.hpp"
#include "run_table.hpp"

namespace qsx {

struct RunTile {
  int block;
  int tile_in_block;
};

// `tile` must be uniform over the lanes that call this (make it so with readfirstlane where the compiler cannot see it).
__device__ __forceinline__ RunTile run_locate(const long long *__restrict__ table, int tile) {
  const int nb = static_cast<int>(table[0]);
  const int uniform = static_cast<int>(table[1]);
  int b;
  if (uniform > 0) {
    b = static_cast<int>(static_cast<unsigned>(tile) / static_cast<unsigned>(uniform));
    return RunTile{b, tile - b * uniform};
  }
  int lo = 0, hi = nb - 1;   // last block whose first tile <= tile
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[kRunHeaderWords + mid] <= tile) lo = mid; else hi = mid - 1;
  }
  return RunTile{lo, tile - static_cast<int>(table[kRunHeaderWords + lo])};
}
__device__ __forceinline__ long long run_rows(const long long *__restrict__ t, int b) {
  return t[QSX_RUN_WORD(t[0], kRunRows, b)];
}
template <typename T>
__device__ __forceinline__ const T *run_in(const long long *__restrict__ t, int b) {
  return as_global(reinterpret_cast<const T *>(t[QSX_RUN_WORD(t[0], kRunIn, b)]));
}
__device__ __forceinline__ const uint64_t *run_filter(const long long *__restrict__ t, int b) {
  return as_global(reinterpret_cast<const uint64_t *>(t[QSX_RUN_WORD(t[0], kRunFilter, b)]));
}
template <typename T>
__device__ __forceinline__ T *run_out(const long long *__restrict__ t, int b) {
  return as_global(reinterpret_cast<T *>(t[QSX_RUN_WORD(t[0], kRunOut, b)]));
}
__device__ __forceinline__ long long run_base(const long long *__restrict__ t, int b) {
  return t[QSX_RUN_WORD(t[0], kRunBase, b)];
}
__device__ __forceinline__ bool run_has_coding(const long long *__restrict__ t) { return t[3] != 0; }
__device__ __forceinline__ int run_code_width(const long long *__restrict__ t, int b) {
  return static_cast<int>(t[QSX_RUN_WORD(t[0], kRunCodeWidth, b)]);
}
__device__ __forceinline__ const void *run_dictionary(const long long *__restrict__ t, int b) {
  return as_global(reinterpret_cast<const unsigned char *>(t[QSX_RUN_WORD(t[0], kRunDictionary, b)]));
}

// ---- a tile of a stripe, or of a run of blocks (block_runs.hpp) -----------------------------------------------------------
template <typename KeyT>
struct ProbeTileSource {
  const KeyT *keys;
  int64_t n;                 // rows of the block
  int64_t base;              // first row of the tile within the block
  int32_t base_tid;
  const uint64_t *filter;
  uint64_t *out_bitmap;
  int block;                 // position of the block in the run (0 without a run)
  int code_width;            // 0: `keys` are values; 1 / 2 / 4: `keys` is a stripe of codes that wide (coded_key below)
  const void *dictionary;    // the block's dictionary of KeyT values, or nullptr: the codes are truncated values
};
// Row `row` of a coded stripe (src.code_width != 0) as the key it stands for.
template <typename KeyT>
__device__ __forceinline__ KeyT coded_key(const ProbeTileSource<KeyT> &src, int64_t row) {
  const void *codes = src.keys;
  uint32_t code;
  if (src.code_width == 1) code = load_global_nt(&static_cast<const uint8_t *>(codes)[row]);
  else if (src.code_width == 2) code = load_global_nt(&static_cast<const uint16_t *>(codes)[row]);
  else code = load_global_nt(&static_cast<const uint32_t *>(codes)[row]);
  if (src.dictionary == nullptr) return static_cast<KeyT>(code);   // (truncation keeps non-negative values only: zero-extension)
  return load_global(&static_cast<const KeyT *>(src.dictionary)[code]);
}
// R rows of a coded stripe at once — row_of(r) = the (clamped) row of step r: the width is chosen once, outside the reads (a
// choice per read puts every read into a basic block of its own and the tile pays R memory round trips instead of one), and a
// dictionary's lookups follow the codes as a second batch.
template <typename KeyT, int R, typename RowOf>
__device__ __forceinline__ void coded_keys(const ProbeTileSource<KeyT> &src, KeyT (&k)[R], RowOf row_of) {
  const void *codes = src.keys;
  uint32_t code[R];
  if (src.code_width == 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) code[r] = load_global_nt(&static_cast<const uint8_t *>(codes)[row_of(r)]);
  } else if (src.code_width == 2) {
#pragma unroll
    for (int r = 0; r < R; ++r) code[r] = load_global_nt(&static_cast<const uint16_t *>(codes)[row_of(r)]);
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) code[r] = load_global_nt(&static_cast<const uint32_t *>(codes)[row_of(r)]);
  }
  if (src.dictionary == nullptr) {
#pragma unroll
    for (int r = 0; r < R; ++r) k[r] = static_cast<KeyT>(code[r]);
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) k[r] = load_global(&static_cast<const KeyT *>(src.dictionary)[code[r]]);
  }
}
template <typename KeyT, int kTileRows, bool kRuns>
__device__ __forceinline__ ProbeTileSource<KeyT> probe_tile_source(const long long *__restrict__ runs, int64_t tile,
                                                                   const KeyT *keys, int64_t n, int32_t base_tid,
                                                                   const uint64_t *filter, uint64_t *out_bitmap) {
  if (!kRuns) return ProbeTileSource<KeyT>{keys, n, tile * kTileRows, base_tid, filter, out_bitmap, 0, 0, nullptr};
  const RunTile at = run_locate(runs, static_cast<int>(tile));
  const bool coded = run_has_coding(runs);
  return ProbeTileSource<KeyT>{run_in<KeyT>(runs, at.block), run_rows(runs, at.block),
                               static_cast<int64_t>(at.tile_in_block) * kTileRows, static_cast<int32_t>(run_base(runs, at.block)),
                               run_filter(runs, at.block), run_out<uint64_t>(runs, at.block), at.block,
                               coded ? run_code_width(runs, at.block) : 0, coded ? run_dictionary(runs, at.block) : nullptr};
}

}  // namespace qsx

#ifndef __HIPCC_RTC__
#include "common.hpp"

namespace qsx {

inline int RunTable::upload(void *stream) {
  return staged_table(static_cast<hipStream_t>(stream), words_.data(), words_.size() * sizeof(long long), &dev_);
}

}  // namespace qsx
#endif  // __HIPCC_RTC__

#endif  // QSX_CSRC_BLOCK_RUNS_HPP_
