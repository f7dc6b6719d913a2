// varchar.hip — VARCHAR attributes of adopted CompressedColumnStore blocks: LIKE / NOT LIKE over a variable-length
// compression dictionary, and the decoding of a code stripe into NUL-padded fields.
//
// A variable-length dictionary (compression/CompressionDictionary.hpp:46-58, CompressionDictionaryLite.hpp:248-290,
// CompressionDictionaryBuilder.cpp:53-66) is {uint32 num_codes; uint32 null_code; uint32 offset[num_codes]; value bytes}: the
// values lie back to back in code order, entry c is [offset[c], offset[c + 1]) and the last entry ends where the dictionary
// does.  A VARCHAR value carries its terminating NUL (types/VarCharType.hpp:42,112), so every entry is at least one byte
// long and ends in 0.  The entry points take the offset array (4-byte aligned: the host layer copies it when the image
// leaves it elsewhere) and the value bytes, which are read where they lie, at any alignment.
//
// qsx_select_like_var(_blocks) replaces the loop of PatternMatchingUncheckedComparator (types/operations/comparisons/
// PatternMatchingComparators-inl.hpp:190-268) over the CompressedColumnStoreValueAccessor of such an attribute: the reference
// decompresses every row and matches it; here the pattern is matched once against every dictionary entry and the rows test
// membership (qsx_select_codes_in_set).  For a nearly unique attribute (o_comment) the dictionary is most of the block, and
// matching it is bound by reading it.  The kernel is like.hip's like_tile with rows of varying length: a workgroup takes a
// range of consecutive entries, stages their offsets and their contiguous bytes [offset[e0], offset[e1]) into LDS (aligned
// 16-byte streaming loads, the range's first and last few bytes one by one, the tile at the source's own offset within 16
// bytes), then one lane matches one entry from LDS and a ballot makes the bitmap word.
//
// qsx_decode_codes_var replaces CompressedTupleStorageSubBlock::getAttributeValue (storage/CompressedTupleStorageSubBlock.hpp:
// 225-300) over a variable-length dictionary, as qsx_decode_codes does for fixed ones: a lane gathers its row's entry into
// an LDS tile of output rows, and the workgroup writes the tile with 16-byte stores.
#include "common.hpp"
#include "block_runs.hpp"
#include "like_match.hpp"

namespace qsx {
namespace varchar {

using like::kBlock;
using like::kWavesPerBlock;
using like::LikePattern;

// What the host guarantees and the kernels still never trust: offsets beyond value_bytes or out of order are cut to the
// dictionary and to the tile, so a malformed dictionary gives wrong bits, never an access outside `values` or the tile.
struct VarDict {
  const uint32_t *offsets;
  const unsigned char *values;
  long long num_entries;
  long long value_bytes;
  const uint64_t *filter;
  uint64_t *out;
};

// LDS of the LIKE kernel: [offsets of the tile's entries and the end of its last: tile_entries + 1 words, rounded to 16
// bytes | the tile's bytes, at most tile_entries * (max_length + 1), at the source's offset within 16 bytes].
__host__ __device__ constexpr int offsets_lds_bytes(int tile_entries) { return ((tile_entries + 1) * 4 + 15) / 16 * 16; }

// Entries [e0, e0 + tile_entries) of a dictionary.  tile_entries is a multiple of 64; tile_cap = tile_entries * (max_length + 1).
__device__ __forceinline__ void like_var_tile(const VarDict &d, const LikePattern &pat, bool negate, int64_t e0, int tile_entries,
                                              int tile_cap, unsigned char *s_mem, unsigned long long &count) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  uint32_t *s_off = reinterpret_cast<uint32_t *>(s_mem);
  unsigned char *s_tile = s_mem + offsets_lds_bytes(tile_entries);
  const int entries = static_cast<int>(d.num_entries - e0 < tile_entries ? d.num_entries - e0 : tile_entries);
  const uint32_t limit = static_cast<uint32_t>(d.value_bytes);
  __syncthreads();   // every wave is done with the previous tile
  for (int i = threadIdx.x; i <= entries; i += kBlock) {
    const int64_t e = e0 + i;
    const uint32_t o = e < d.num_entries ? load_global(&d.offsets[e]) : limit;   // the last entry ends where the dictionary does
    s_off[i] = o < limit ? o : limit;
  }
  __syncthreads();
  const uint32_t lo = s_off[0];
  const uint32_t hi = s_off[entries] > lo ? s_off[entries] : lo;
  const int bytes = static_cast<int>(hi - lo < static_cast<uint32_t>(tile_cap) ? hi - lo : static_cast<uint32_t>(tile_cap));
  const unsigned char *src = d.values + lo;
  const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15);
  unsigned char *data = s_tile + shift;   // data[o] = src[o]; data + o is 16-byte aligned where src + o is
  int head = shift != 0 ? 16 - shift : 0;
  if (head > bytes) head = bytes;
  const int full = (bytes - head) & ~15;
  for (int o = threadIdx.x; o < head; o += kBlock) data[o] = load_global(src + o);
  for (int o = head + threadIdx.x * 16; o < head + full; o += kBlock * 16) {
    *reinterpret_cast<uint4 *>(data + o) = stream_load16(src + o);
  }
  for (int o = head + full + threadIdx.x; o < bytes; o += kBlock) data[o] = load_global(src + o);
  __syncthreads();
  for (int w = wave; w * 64 < entries; w += kWavesPerBlock) {
    const int i = w * 64 + lane;
    bool pred = false;
    if (i < entries) {
      const uint32_t a = s_off[i], b = s_off[i + 1];
      int start = a > lo ? static_cast<int>(a - lo < static_cast<uint32_t>(bytes) ? a - lo : static_cast<uint32_t>(bytes)) : 0;
      int end = b > lo ? static_cast<int>(b - lo < static_cast<uint32_t>(bytes) ? b - lo : static_cast<uint32_t>(bytes)) : 0;
      if (end < start) end = start;
      // the text ends at the entry's NUL: like_match stops there, and at the entry's end in any case
      pred = like::like_match(data + start, end - start, pat) != negate;   // entries past the end: 0 also under NOT LIKE
    }
    uint64_t word = msb_first(__ballot(pred));
    const int64_t word_index = (e0 >> 6) + w;
    if (d.filter != nullptr) word &= load_global(&d.filter[word_index]);
    if (lane == 0) {
      store_global(word, &d.out[word_index]);
      count += __popcll(word);
    }
  }
}

__global__ __launch_bounds__(kBlock) void like_var_kernel(VarDict d, LikePattern pat, int negate, unsigned long long *__restrict__ out_count,
                                                         int tile_entries, int tile_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  __shared__ LikePattern s_pat;
  like::stage_pattern(pat, &s_pat);
  const int lane = lane_id();
  const int64_t num_tiles = (d.num_entries + tile_entries - 1) / tile_entries;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    like_var_tile(d, s_pat, negate != 0, tile * tile_entries, tile_entries, tile_cap, s_mem, count);
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

// The same over the dictionaries of a run of blocks (block_runs.hpp: rows = entries, in = value bytes, filter, out); block
// b's offset array and number of value bytes sit behind the run table at words extra + 2 b.  A workgroup takes a contiguous
// range of the run's tiles, a wave adds its matches to a block's counter when the workgroup moves on (as like_runs_kernel).
__global__ __launch_bounds__(kBlock) void like_var_runs_kernel(const long long *__restrict__ runs, long long extra, LikePattern pat, int negate,
                                                              unsigned long long *__restrict__ out_counts, int tile_entries, int tile_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  __shared__ LikePattern s_pat;
  like::stage_pattern(pat, &s_pat);
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
    const VarDict d{as_global(reinterpret_cast<const uint32_t *>(runs[extra + 2 * at.block])), run_in<unsigned char>(runs, at.block),
                    run_rows(runs, at.block), runs[extra + 2 * at.block + 1], run_filter(runs, at.block), run_out<uint64_t>(runs, at.block)};
    like_var_tile(d, s_pat, negate != 0, static_cast<int64_t>(at.tile_in_block) * tile_entries, tile_entries, tile_cap, s_mem, count);
  }
  if (out_counts != nullptr && counted_block >= 0 && lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
}

// ---------------------------------------------------------------------------
// Decoding: out[i] = the text of entry codes[i], NUL-padded to out_width bytes (cut there without a terminator, like
// CHAR(n)); all NUL for a code >= num_entries (the NULL code).  A lane gathers its row — the entry's first bytes up to a
// 4-byte boundary, then aligned words, then the rest: nothing outside the entry is read — into an LDS tile of output rows
// that lies at the destination's own offset within 16 bytes; the workgroup then writes the tile with 16-byte stores.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void put_text_byte(unsigned char *row, int j, uint32_t c, bool &alive) {
  alive = alive && c != 0;   // behind the terminator every byte of the field is 0, whatever the dictionary holds there
  row[j] = alive ? static_cast<unsigned char>(c) : static_cast<unsigned char>(0);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(u32x4 v, unsigned char *p) {   // p is 16-byte aligned, in device memory
  *(__attribute__((address_space(1))) u32x4 *)reinterpret_cast<uintptr_t>(p) = v;
}

template <typename CodeT>
__global__ __launch_bounds__(kBlock) void decode_var_kernel(const CodeT *__restrict__ codes, int64_t n, const uint32_t *__restrict__ offsets,
                                                           const unsigned char *__restrict__ values, long long num_entries, long long value_bytes,
                                                           int out_width, unsigned char *__restrict__ out, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const int64_t num_tiles = (n + tile_rows - 1) / tile_rows;
  const uint32_t limit = static_cast<uint32_t>(value_bytes);
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * tile_rows;
    const int rows = static_cast<int>(n - row0 < tile_rows ? n - row0 : tile_rows);
    unsigned char *dst = out + row0 * out_width;
    const int bytes = rows * out_width;
    const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
    unsigned char *data = s_tile + shift;   // data + o is 16-byte aligned where dst + o is
    __syncthreads();   // the previous tile has been written out
    for (int r = threadIdx.x; r < rows; r += kBlock) {
      const uint32_t code = load_global_nt(&codes[row0 + r]);
      unsigned char *row = data + r * out_width;
      int j = 0;
      if (code < static_cast<unsigned long long>(num_entries)) {
        uint32_t a = load_global(&offsets[code]);
        uint32_t b = static_cast<long long>(code) + 1 < num_entries ? load_global(&offsets[code + 1]) : limit;
        if (a > limit) a = limit;
        if (b > limit) b = limit;
        if (b < a) b = a;
        const int len = static_cast<int>(b - a < static_cast<uint32_t>(out_width) ? b - a : static_cast<uint32_t>(out_width));
        const unsigned char *src = values + a;
        bool alive = true;
        for (; j < len && (reinterpret_cast<uintptr_t>(src + j) & 3) != 0; ++j) put_text_byte(row, j, load_global(src + j), alive);
        for (; j + 4 <= len; j += 4) {
          const uint32_t w = load_global(reinterpret_cast<const uint32_t *>(src + j));
#pragma unroll
          for (int k = 0; k < 4; ++k) put_text_byte(row, j + k, (w >> (8 * k)) & 0xFFu, alive);
        }
        for (; j < len; ++j) put_text_byte(row, j, load_global(src + j), alive);
      }
      for (; j < out_width; ++j) row[j] = 0;
    }
    __syncthreads();
    int head = shift != 0 ? 16 - shift : 0;
    if (head > bytes) head = bytes;
    const int full = (bytes - head) & ~15;
    for (int o = threadIdx.x; o < head; o += kBlock) store_global(data[o], dst + o);
    for (int o = head + threadIdx.x * 16; o < head + full; o += kBlock * 16) {
      store16(*reinterpret_cast<const u32x4 *>(data + o), dst + o);
    }
    for (int o = head + full + threadIdx.x; o < bytes; o += kBlock) store_global(data[o], dst + o);
  }
}

// Entries per tile of the LIKE kernel: a multiple of 64 (whole bitmap words), sized from the longest entry (max_length + 1
// bytes) so that the tile's bytes fit 48 KiB of LDS whatever the entries hold, 1024 at most (as like.hip's like_tile_rows:
// three workgroups, 12 waves, per CU at the full 48 KiB).
static int like_var_tile_entries(int max_length) {
  int tile_entries = (48 * 1024 / (max_length + 1)) / 64 * 64;
  if (tile_entries > 1024) tile_entries = 1024;
  if (tile_entries < 64) tile_entries = 64;
  return tile_entries;
}
static size_t like_var_lds_bytes(int tile_entries, int max_length) {
  return offsets_lds_bytes(tile_entries) + (static_cast<size_t>(tile_entries) * (max_length + 1) + 15) / 16 * 16 + 16;
}

// Output rows per tile of the decoder: a multiple of 64, at most 32 KiB of LDS (five workgroups per CU) and 1024 rows.
static int decode_var_tile_rows(int out_width) {
  int tile_rows = (32 * 1024 / out_width) / 64 * 64;
  if (tile_rows > 1024) tile_rows = 1024;
  if (tile_rows < 64) tile_rows = 64;
  return tile_rows;
}

template <typename CodeT>
static int launch_decode_var(const void *codes_dev, int64_t n, const uint32_t *offsets_dev, const void *values_dev, int64_t num_entries,
                             int64_t value_bytes, int out_width, void *out_dev, hipStream_t s) {
  const int tile_rows = decode_var_tile_rows(out_width);
  const int64_t tiles = (n + tile_rows - 1) / tile_rows;
  const size_t lds = (static_cast<size_t>(tile_rows) * out_width + 15) / 16 * 16 + 16;
  hipLaunchKernelGGL(decode_var_kernel<CodeT>, dim3(tile_grid(tiles)), dim3(kBlock), lds, s, static_cast<const CodeT *>(codes_dev), n, offsets_dev,
                     static_cast<const unsigned char *>(values_dev), static_cast<long long>(num_entries), static_cast<long long>(value_bytes),
                     out_width, static_cast<unsigned char *>(out_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

// The arguments every dictionary comes with: entries of at least one byte each, offsets of 32 bits.
static bool dictionary_ok(const uint32_t *offsets, const void *values, int64_t num_entries, int64_t value_bytes) {
  if (num_entries < 0 || value_bytes < num_entries || value_bytes > static_cast<int64_t>(UINT32_MAX)) return false;
  // (the offsets are read as 32-bit words; a dictionary without entries needs neither array)
  return num_entries == 0 || (offsets != nullptr && values != nullptr && (reinterpret_cast<uintptr_t>(offsets) & 3) == 0);
}

}  // namespace varchar
}  // namespace qsx

using namespace qsx;
using namespace qsx::varchar;

extern "C" {

int qsx_select_like_var(const uint32_t *offsets_dev, const void *values_dev, int64_t num_entries, int64_t value_bytes, int max_length,
                        const void *pattern, int pattern_length, int negate, const uint64_t *filter_dev, uint64_t *out_bitmap_dev,
                        int64_t *out_count_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (!dictionary_ok(offsets_dev, values_dev, num_entries, value_bytes) || max_length < 1 || pattern_length < 0 ||
      (pattern_length > 0 && pattern == nullptr) || (negate != 0 && negate != 1) || (num_entries > 0 && out_bitmap_dev == nullptr)) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (pattern_length > QSX_MAX_LIKE_PATTERN || max_length > QSX_MAX_VARCHAR_LENGTH) return QSX_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (num_entries == 0) return QSX_OK;
  const LikePattern pat = like::clean_pattern(pattern, pattern_length);
  const int tile_entries = like_var_tile_entries(max_length);
  const int64_t tiles = (num_entries + tile_entries - 1) / tile_entries;
  const VarDict d{offsets_dev, static_cast<const unsigned char *>(values_dev), num_entries, value_bytes, filter_dev, out_bitmap_dev};
  hipLaunchKernelGGL(like_var_kernel, dim3(tile_grid(tiles)), dim3(kBlock), like_var_lds_bytes(tile_entries, max_length), s, d, pat, negate,
                     reinterpret_cast<unsigned long long *>(out_count_dev), tile_entries, tile_entries * (max_length + 1));
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_like_var_blocks(int max_length, int64_t num_blocks, const int64_t *block_entries, const uint32_t *const *block_offsets,
                               const void *const *block_values, const int64_t *block_value_bytes, const void *pattern, int pattern_length,
                               int negate, const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps, int64_t *out_counts_dev,
                               qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || max_length < 1 || pattern_length < 0 || (pattern_length > 0 && pattern == nullptr) || (negate != 0 && negate != 1) ||
      (num_blocks > 0 && (block_entries == nullptr || block_offsets == nullptr || block_values == nullptr || block_value_bytes == nullptr ||
                          block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (pattern_length > QSX_MAX_LIKE_PATTERN || max_length > QSX_MAX_VARCHAR_LENGTH) return QSX_ERR_UNSUPPORTED;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_entries, block_values, reinterpret_cast<const void *const *>(block_out_bitmaps))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  for (int64_t b = 0; b < num_blocks; ++b) {
    if (!dictionary_ok(block_offsets[b], block_values[b], block_entries[b], block_value_bytes[b])) return QSX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = as_stream(stream);
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  const LikePattern pat = like::clean_pattern(pattern, pattern_length);
  const int tile_entries = like_var_tile_entries(max_length);
  RunTable table;
  const long long tiles = table.build(tile_entries, num_blocks, block_entries, block_values, reinterpret_cast<const void *const *>(block_filters),
                                      reinterpret_cast<void *const *>(block_out_bitmaps), nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const long long extra = table.append(2 * static_cast<size_t>(num_blocks));
  for (int64_t b = 0; b < num_blocks; ++b) {
    table.words()[extra + 2 * b] = RunTable::word_of(block_offsets[b]);
    table.words()[extra + 2 * b + 1] = block_value_bytes[b];
  }
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  hipLaunchKernelGGL(like_var_runs_kernel, dim3(tile_grid(tiles)), dim3(kBlock), like_var_lds_bytes(tile_entries, max_length), s, table.dev(), extra,
                     pat, negate, reinterpret_cast<unsigned long long *>(out_counts_dev), tile_entries, tile_entries * (max_length + 1));
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_decode_codes_var(int code_width, const void *codes_dev, int64_t n, const uint32_t *offsets_dev, const void *values_dev,
                         int64_t num_entries, int64_t value_bytes, int out_width, void *out_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || !dictionary_ok(offsets_dev, values_dev, num_entries, value_bytes) || out_width < 1 || out_width > QSX_MAX_VARCHAR_LENGTH ||
      (n > 0 && (codes_dev == nullptr || out_dev == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (code_width != 1 && code_width != 2 && code_width != 4) return QSX_ERR_UNSUPPORTED;
  if (n == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  switch (code_width) {
    case 1: return launch_decode_var<uint8_t>(codes_dev, n, offsets_dev, values_dev, num_entries, value_bytes, out_width, out_dev, s);
    case 2: return launch_decode_var<uint16_t>(codes_dev, n, offsets_dev, values_dev, num_entries, value_bytes, out_width, out_dev, s);
    default: return launch_decode_var<uint32_t>(codes_dev, n, offsets_dev, values_dev, num_entries, value_bytes, out_width, out_dev, s);
  }
}

}  // extern "C"
