// like.hip — LIKE / NOT LIKE on CHAR(width) stripes, and the code-membership scan that carries a LIKE (or any set of values)
// over a dictionary-coded attribute.
//
// Replaces the scan loops of PatternMatchingUncheckedComparator (types/operations/comparisons/
// PatternMatchingComparators-inl.hpp:190-268: the pattern compiled once, matched against every value of the accessor) as
// reached from ComparisonPredicate::getAllMatches, i.e. the same getMatchesForPredicate loop qsx_select_cmp_char replaces.
//
// Semantics (PatternMatchingComparators.hpp:60-232): the text is the field's bytes up to its first NUL or `width` bytes,
// '%' is any run of bytes, '_' is one byte, nothing escapes them, the match is anchored at both ends.  '_' is one BYTE here
// (CHAR comparisons of this library are byte-wise); the reference's re2 runs in UTF-8 mode and lets it take a code point.
//
// The matcher needs no backtracking: the pattern is cut at its '%' into segments of fixed length.  The first is anchored at
// the start of the text, the last at its end, every one in between takes its leftmost fit behind the one before.  A lane
// walks its row once: the text's length is only looked for when a last segment has to be placed (`lit%` reads no further
// than the literal, `%lit%` stops at its first fit).
#include <vector>

#include "common.hpp"
#include "block_runs.hpp"
#include "like_match.hpp"

namespace qsx {
namespace like {

// One tile (rows [row0, row0 + tile_rows) of a stripe): the tile's bytes go to LDS with 16-byte streaming loads (a row per
// lane straight from HBM would read `width`-strided bytes), then one lane matches one row and a ballot makes the bitmap
// word.  The tile lies in LDS at the stripe's own offset within 16 bytes, so a stripe that starts anywhere is still read
// with aligned 16-byte loads (its first and last few bytes one by one).  tile_rows is a multiple of 64.
__device__ __forceinline__ void like_tile(const unsigned char *__restrict__ col, int width, int64_t n, const LikePattern &pat, bool negate,
                                          const uint64_t *__restrict__ filter, uint64_t *__restrict__ out, int64_t row0, int tile_rows,
                                          unsigned char *s_tile, unsigned long long &count) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int rows = static_cast<int>(n - row0 < tile_rows ? n - row0 : tile_rows);
  const unsigned char *src = col + row0 * width;
  const int bytes = rows * width;
  const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15);
  unsigned char *data = s_tile + shift;   // data[o] = src[o]; data + o is 16-byte aligned where src + o is
  int head = shift != 0 ? 16 - shift : 0;
  if (head > bytes) head = bytes;
  const int full = (bytes - head) & ~15;
  __syncthreads();   // every wave is done with the previous tile
  for (int o = threadIdx.x; o < head; o += kBlock) data[o] = src[o];
  for (int o = head + threadIdx.x * 16; o < head + full; o += kBlock * 16) {
    *reinterpret_cast<uint4 *>(data + o) = stream_load16(src + o);
  }
  for (int o = head + full + threadIdx.x; o < bytes; o += kBlock) data[o] = src[o];
  __syncthreads();
  for (int w = wave; w * 64 < rows; w += kWavesPerBlock) {
    const int r = w * 64 + lane;
    const bool pred = r < rows && (like_match(data + r * width, width, pat) != negate);   // rows past the end: 0 also under NOT LIKE
    uint64_t word = msb_first(__ballot(pred));
    const int64_t word_index = (row0 >> 6) + w;
    if (filter != nullptr) word &= filter[word_index];
    if (lane == 0) {
      out[word_index] = word;
      count += __popcll(word);
    }
  }
}

__global__ __launch_bounds__(kBlock) void like_kernel(const unsigned char *__restrict__ col, int width, int64_t n, LikePattern pat, int negate,
                                                     const uint64_t *__restrict__ filter, uint64_t *__restrict__ out,
                                                     unsigned long long *__restrict__ out_count, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  __shared__ LikePattern s_pat;
  stage_pattern(pat, &s_pat);
  const int lane = lane_id();
  const int64_t num_tiles = (n + tile_rows - 1) / tile_rows;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    like_tile(col, width, n, s_pat, negate != 0, filter, out, tile * tile_rows, tile_rows, s_tile, count);
  }
  if (out_count != nullptr) {
    __shared__ unsigned long long block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    if (lane == 0 && count != 0) atomicAdd(&block_count, count);
    __syncthreads();
    if (threadIdx.x == 0 && block_count != 0) atomicAdd(out_count, block_count);
  }
}

// The same over a run of blocks (block_runs.hpp): a workgroup takes a contiguous range of the run's tiles, a wave adds its
// matches to a block's counter when the workgroup moves on to another block (as select_char_runs_kernel).
__global__ __launch_bounds__(kBlock) void like_runs_kernel(const long long *__restrict__ runs, int width, LikePattern pat, int negate,
                                                          unsigned long long *__restrict__ out_counts, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  __shared__ LikePattern s_pat;
  stage_pattern(pat, &s_pat);
  const int lane = lane_id();
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  unsigned long long count = 0;
  int counted_block = -1;
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    if (at.block != counted_block) {
      if (out_counts != nullptr && counted_block >= 0 && lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
      count = 0;
      counted_block = at.block;
    }
    like_tile(run_in<unsigned char>(runs, at.block), width, run_rows(runs, at.block), s_pat, negate != 0, run_filter(runs, at.block),
              run_out<uint64_t>(runs, at.block), static_cast<int64_t>(at.tile_in_block) * tile_rows, tile_rows, s_tile, count);
  }
  if (out_counts != nullptr && counted_block >= 0 && lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
}

// ---------------------------------------------------------------------------
// Code membership: out[i] = set[codes[i]] over a stripe of 1/2/4-byte codes, the set a bitmap of num_codes bits in the
// TupleIdSequence layout (bit i = bit 63 - (i & 63) of word i >> 6) — e.g. what like_kernel wrote over the block's dictionary.
// A code stripe scan as select.hip's packed kernels: a lane reads 16 bytes = K codes, the 64 / K lanes of a bitmap word merge
// their K-bit masks with xor-shuffles.  The set is read as 32-bit words (word (i >> 5) ^ 1 of the little-endian 64-bit
// layout) from LDS when it fits kSetLdsBytes there (every 1- and 2-byte code: 8 KiB at most), else through L2.
// ---------------------------------------------------------------------------
constexpr int kSetLdsBytes = 32 * 1024;
constexpr int kSetLoads = 4;   // 16-byte reads in flight per lane and tile
template <typename T>
constexpr int set_tile_rows() { return kBlock * (16 / static_cast<int>(sizeof(T))) * kSetLoads; }

__device__ __forceinline__ long long set_words32(long long num_codes) { return ((num_codes + 63) >> 6) * 2; }

template <bool kLds>
__device__ __forceinline__ bool in_set(const uint32_t *set, unsigned long long num_codes, uint32_t code) {
  if (code >= num_codes) return false;   // (the reference's NULL code = num_codes among them)
  const uint32_t word = kLds ? set[(code >> 5) ^ 1u] : load_global(&set[(code >> 5) ^ 1u]);
  return ((word >> (31 - (code & 31))) & 1u) != 0;
}

// One tile of set_tile_rows<T>() rows from row0 on, by the whole workgroup.  `aligned`: the stripe starts on a 16-byte boundary.
template <typename T, bool kLds>
__device__ __forceinline__ void codes_in_set_tile(const T *__restrict__ codes, int64_t n, bool aligned, const uint32_t *set,
                                                  unsigned long long num_codes, const uint64_t *__restrict__ filter,
                                                  uint64_t *__restrict__ out, int64_t row0, unsigned long long &count) {
  constexpr int K = 16 / static_cast<int>(sizeof(T));   // rows per lane and load
  constexpr int G = kWave / K;                          // lanes per bitmap word
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t num_words = (n + 63) >> 6;
  uint4 raw[kSetLoads];
#pragma unroll
  for (int r = 0; r < kSetLoads; ++r) {
    const int64_t at = row0 + (static_cast<int64_t>(wave * kSetLoads + r) * kWave + lane) * K;
    raw[r] = make_uint4(0, 0, 0, 0);
    if (aligned && at + K <= n) {
      raw[r] = stream_load16(codes + at);
    } else if (at < n) {   // an unaligned stripe, or the last partial 16 bytes: code by code
      T tmp[K];
#pragma unroll
      for (int i = 0; i < K; ++i) tmp[i] = at + i < n ? codes[at + i] : T();
      __builtin_memcpy(&raw[r], tmp, 16);
    }
  }
#pragma unroll
  for (int r = 0; r < kSetLoads; ++r) {
    const int64_t at = row0 + (static_cast<int64_t>(wave * kSetLoads + r) * kWave + lane) * K;
    T v[K];
    __builtin_memcpy(v, &raw[r], 16);
    unsigned long long m = 0;   // K-bit mask, first row = most significant bit
#pragma unroll
    for (int i = 0; i < K; ++i) m = (m << 1) | ((at + i < n && in_set<kLds>(set, num_codes, v[i])) ? 1ull : 0ull);
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {   // after step d the lower lane of every 2d-group holds 2d * K bits
      const unsigned long long other = __shfl_xor(m, d, kWave);
      m = (m << (d * K)) | other;
    }
    const int64_t word = (at >> 6);
    if ((lane % G) == 0 && word < num_words) {
      if (filter != nullptr) m &= filter[word];
      out[word] = m;
      count += __popcll(m);
    }
  }
}

// Brings a set that fits into LDS; returns whether it did.  Called by the whole workgroup.
__device__ __forceinline__ bool stage_set(const uint32_t *__restrict__ set, long long num_codes, uint32_t *s_set) {
  const long long words = set_words32(num_codes);
  if (words * 4 > kSetLdsBytes) return false;
  __syncthreads();   // every wave is done with the set that was there
  for (int i = threadIdx.x; i < static_cast<int>(words); i += kBlock) s_set[i] = load_global(&set[i]);
  __syncthreads();
  return true;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void codes_in_set_kernel(const T *__restrict__ codes, int64_t n, const uint32_t *__restrict__ set,
                                                             long long num_codes, const uint64_t *__restrict__ filter,
                                                             uint64_t *__restrict__ out, unsigned long long *__restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_set[];
  constexpr int kRows = set_tile_rows<T>();
  const bool aligned = (reinterpret_cast<uintptr_t>(codes) & 15) == 0;
  const bool lds = stage_set(set, num_codes, s_set);
  const int64_t num_tiles = (n + kRows - 1) / kRows;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    if (lds) codes_in_set_tile<T, true>(codes, n, aligned, s_set, num_codes, filter, out, tile * kRows, count);
    else codes_in_set_tile<T, false>(codes, n, aligned, set, num_codes, filter, out, tile * kRows, count);
  }
  if (out_count != nullptr) {
    __shared__ unsigned long long block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    count = wave_reduce_add(count);
    if (lane_id() == 0 && count != 0) atomicAdd(&block_count, count);
    __syncthreads();
    if (threadIdx.x == 0 && block_count != 0) atomicAdd(out_count, block_count);
  }
}

// Over a run of blocks, every block with its own set: block b's set address and number of codes sit behind the run table at
// words extra + 2 b.  A workgroup walks a contiguous range of the run's tiles and brings a block's set to LDS when it enters
// the block.
template <typename T>
__global__ __launch_bounds__(kBlock) void codes_in_set_runs_kernel(const long long *__restrict__ runs, long long extra,
                                                                  unsigned long long *__restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_set[];
  constexpr int kRows = set_tile_rows<T>();
  const int lane = lane_id();
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  unsigned long long count = 0;
  int counted_block = -1;
  bool lds = false, aligned = false;
  const uint32_t *set = nullptr;
  long long num_codes = 0;
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    if (at.block != counted_block) {
      if (out_counts != nullptr && counted_block >= 0) {
        count = wave_reduce_add(count);
        if (lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
      }
      count = 0;
      counted_block = at.block;
      set = as_global(reinterpret_cast<const uint32_t *>(runs[extra + 2 * at.block]));
      num_codes = runs[extra + 2 * at.block + 1];
      aligned = (reinterpret_cast<uintptr_t>(run_in<T>(runs, at.block)) & 15) == 0;
      lds = stage_set(set, num_codes, s_set);
    }
    const int64_t row0 = static_cast<int64_t>(at.tile_in_block) * kRows;
    if (lds) {
      codes_in_set_tile<T, true>(run_in<T>(runs, at.block), run_rows(runs, at.block), aligned, s_set, num_codes, run_filter(runs, at.block),
                                 run_out<uint64_t>(runs, at.block), row0, count);
    } else {
      codes_in_set_tile<T, false>(run_in<T>(runs, at.block), run_rows(runs, at.block), aligned, set, num_codes, run_filter(runs, at.block),
                                  run_out<uint64_t>(runs, at.block), row0, count);
    }
  }
  if (out_counts != nullptr && counted_block >= 0) {
    count = wave_reduce_add(count);
    if (lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
  }
}

// rows per tile: a multiple of 64 (whole bitmap words), at most 48 KiB of LDS (as qsx_select_cmp_char)
static int like_tile_rows(int width) {
  int tile_rows = (48 * 1024 / width) / 64 * 64;
  if (tile_rows > 1024) tile_rows = 1024;
  if (tile_rows < 64) tile_rows = 64;
  return tile_rows;
}
static size_t like_lds_bytes(int tile_rows, int width) { return (static_cast<size_t>(tile_rows) * width + 15) / 16 * 16 + 16; }

}  // namespace like
}  // namespace qsx

using namespace qsx;
using namespace qsx::like;

extern "C" {

int qsx_select_like(const void *col_dev, int width, int64_t n, const void *pattern, int pattern_length, int negate,
                    const uint64_t *filter_dev, uint64_t *out_bitmap_dev, int64_t *out_count_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || width < 1 || width > 255 || pattern_length < 0 || (pattern_length > 0 && pattern == nullptr) || (negate != 0 && negate != 1) ||
      (n > 0 && (col_dev == nullptr || out_bitmap_dev == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (pattern_length > QSX_MAX_LIKE_PATTERN) return QSX_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return QSX_OK;
  const LikePattern pat = clean_pattern(pattern, pattern_length);
  const int tile_rows = like_tile_rows(width);
  const int64_t tiles = (n + tile_rows - 1) / tile_rows;
  const int grid = tile_grid(tiles);
  hipLaunchKernelGGL(like_kernel, dim3(grid), dim3(kBlock), like_lds_bytes(tile_rows, width), s, static_cast<const unsigned char *>(col_dev),
                     width, n, pat, negate, filter_dev, out_bitmap_dev, reinterpret_cast<unsigned long long *>(out_count_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_like_blocks(int width, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols, const void *pattern,
                           int pattern_length, int negate, const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps,
                           int64_t *out_counts_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || width < 1 || width > 255 || pattern_length < 0 || (pattern_length > 0 && pattern == nullptr) ||
      (negate != 0 && negate != 1) || (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (pattern_length > QSX_MAX_LIKE_PATTERN) return QSX_ERR_UNSUPPORTED;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_out_bitmaps))) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  const LikePattern pat = clean_pattern(pattern, pattern_length);
  const int tile_rows = like_tile_rows(width);
  RunTable table;
  const long long tiles = table.build(tile_rows, num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_filters),
                                      reinterpret_cast<void *const *>(block_out_bitmaps), nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  const long long *runs_dev = table.dev();
  const int grid = tile_grid(tiles);
  hipLaunchKernelGGL(like_runs_kernel, dim3(grid), dim3(kBlock), like_lds_bytes(tile_rows, width), s, runs_dev, width, pat, negate,
                     reinterpret_cast<unsigned long long *>(out_counts_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_codes_in_set(int code_width, const void *codes_dev, int64_t n, const uint64_t *set_dev, int64_t num_codes,
                            const uint64_t *filter_dev, uint64_t *out_bitmap_dev, int64_t *out_count_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || num_codes < 0 || (num_codes > 0 && set_dev == nullptr) || (n > 0 && (codes_dev == nullptr || out_bitmap_dev == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (code_width != 1 && code_width != 2 && code_width != 4) return QSX_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return QSX_OK;
  const size_t set_bytes = static_cast<size_t>((num_codes + 63) / 64) * 8;
  const size_t lds = set_bytes <= static_cast<size_t>(kSetLdsBytes) ? set_bytes : 0;
  const uint32_t *set = reinterpret_cast<const uint32_t *>(set_dev);
  unsigned long long *count = reinterpret_cast<unsigned long long *>(out_count_dev);
  const long long tile_rows = code_width == 1 ? set_tile_rows<uint8_t>() : code_width == 2 ? set_tile_rows<uint16_t>() : set_tile_rows<uint32_t>();
  const int grid = grid_for((n + tile_rows - 1) / tile_rows, 1);
  switch (code_width) {
    case 1:
      hipLaunchKernelGGL(codes_in_set_kernel<uint8_t>, dim3(grid), dim3(kBlock), lds, s, static_cast<const uint8_t *>(codes_dev), n, set,
                         static_cast<long long>(num_codes), filter_dev, out_bitmap_dev, count);
      break;
    case 2:
      hipLaunchKernelGGL(codes_in_set_kernel<uint16_t>, dim3(grid), dim3(kBlock), lds, s, static_cast<const uint16_t *>(codes_dev), n, set,
                         static_cast<long long>(num_codes), filter_dev, out_bitmap_dev, count);
      break;
    default:
      hipLaunchKernelGGL(codes_in_set_kernel<uint32_t>, dim3(grid), dim3(kBlock), lds, s, static_cast<const uint32_t *>(codes_dev), n, set,
                         static_cast<long long>(num_codes), filter_dev, out_bitmap_dev, count);
      break;
  }
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_codes_in_set_blocks(int code_width, int64_t num_blocks, const int64_t *block_rows, const void *const *block_codes,
                                   const uint64_t *const *block_sets, const int64_t *block_num_codes,
                                   const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps, int64_t *out_counts_dev,
                                   qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || (num_blocks > 0 && (block_rows == nullptr || block_codes == nullptr || block_sets == nullptr || block_num_codes == nullptr ||
                                            block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (code_width != 1 && code_width != 2 && code_width != 4) return QSX_ERR_UNSUPPORTED;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_codes, reinterpret_cast<const void *const *>(block_out_bitmaps))) return QSX_ERR_INVALID_ARGUMENT;
  size_t lds = 0;
  for (int64_t b = 0; b < num_blocks; ++b) {
    if (block_num_codes[b] < 0 || (block_num_codes[b] > 0 && block_sets[b] == nullptr)) return QSX_ERR_INVALID_ARGUMENT;
    const size_t set_bytes = static_cast<size_t>((block_num_codes[b] + 63) / 64) * 8;
    if (set_bytes <= static_cast<size_t>(kSetLdsBytes) && set_bytes > lds) lds = set_bytes;
  }
  hipStream_t s = as_stream(stream);
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  const long long tile_rows = code_width == 1 ? set_tile_rows<uint8_t>() : code_width == 2 ? set_tile_rows<uint16_t>() : set_tile_rows<uint32_t>();
  RunTable table;
  const long long tiles = table.build(tile_rows, num_blocks, block_rows, block_codes, reinterpret_cast<const void *const *>(block_filters),
                                      reinterpret_cast<void *const *>(block_out_bitmaps), nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const long long extra = table.append(2 * static_cast<size_t>(num_blocks));
  for (int64_t b = 0; b < num_blocks; ++b) {
    table.words()[extra + 2 * b] = RunTable::word_of(block_sets[b]);
    table.words()[extra + 2 * b + 1] = block_num_codes[b];
  }
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  const long long *runs_dev = table.dev();
  const int grid = grid_for(tiles, 1);
  unsigned long long *counts = reinterpret_cast<unsigned long long *>(out_counts_dev);
  switch (code_width) {
    case 1: hipLaunchKernelGGL(codes_in_set_runs_kernel<uint8_t>, dim3(grid), dim3(kBlock), lds, s, runs_dev, extra, counts); break;
    case 2: hipLaunchKernelGGL(codes_in_set_runs_kernel<uint16_t>, dim3(grid), dim3(kBlock), lds, s, runs_dev, extra, counts); break;
    default: hipLaunchKernelGGL(codes_in_set_runs_kernel<uint32_t>, dim3(grid), dim3(kBlock), lds, s, runs_dev, extra, counts); break;
  }
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

}  // extern "C"
