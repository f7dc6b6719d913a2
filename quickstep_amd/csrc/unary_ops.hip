// unary_ops.hip — the unary operations of the reference (types/operations/unary_operations/) that TPC-H needs:
// EXTRACT(YEAR | MONTH FROM date) and SUBSTRING(char FROM start FOR length).
//
// Date extract replaces DateExtractUncheckedOperator::applyToColumnVector / applyToValueAccessor
// (DateExtractOperation.cpp:117-142, 277-286): an INT per DateLit, its yearField() or monthField().  A bandwidth-bound map of
// 8 bytes in and 4 bytes out per row: a lane reads four dates with two 16-byte loads and writes their four INTs with one
// 16-byte store.
//
// Substring replaces SubstringUncheckedOperator::computeSubstring (SubstringOperation.cpp:74-91) over CHAR(w): CHAR(m) with
// m = min(w - start, length) (SubstringOperation.hpp:174-182), the text's bytes from `start` (0-based) on, zero-filled to m.
// Row-to-lane from an LDS tile as like.hip's like_tile; the m-byte results are staged in LDS too and leave as 16-byte stores.
//
// Neither kernel sees a null bitmap: the result inherits the operand's (DateExtractOperation.cpp:117-142 copies the NULL).
//
// A predicate over one of these operations (qsx_select_cmp_unary, qsx_select_in_unary: ComparisonPredicate.cpp:209-240 over
// ScalarUnaryExpression::getAllValues, ScalarUnaryExpression.cpp:92-115) is one pass of its own further down: the operation's
// result stays in registers and a bit per row leaves.
#include <vector>

#include "common.hpp"
#include "block_runs.hpp"
#include "char_predicates.hpp"

namespace qsx {
namespace unary {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// EXTRACT
// ---------------------------------------------------------------------------
constexpr int kGroupRows = 4;                                 // dates per lane and group: 32 bytes in, 16 bytes out
constexpr int kGroupsPerLane = 2;                             // groups of a lane in flight per tile: four 16-byte loads
constexpr int kTileGroups = kBlock * kGroupsPerLane;
constexpr int kExtractTileRows = kTileGroups * kGroupRows;    // 2048

// a 16-byte store to an address that is only known to be 4-byte aligned (a stripe whose head was peeled)
typedef unsigned int u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int kUnit>
__device__ __forceinline__ uint32_t field_of(uint32_t lo, uint32_t hi) {
  return kUnit == QSX_DATE_YEAR ? lo : (hi & 0xFFu);          // year: the low dword; month: byte 4
}
template <int kUnit>
__device__ __forceinline__ void extract_row(const unsigned long long *__restrict__ in, int32_t *__restrict__ out, int64_t row) {
  const unsigned long long raw = load_global_nt(&in[row]);
  store_global_nt(static_cast<int32_t>(field_of<kUnit>(static_cast<uint32_t>(raw), static_cast<uint32_t>(raw >> 32))), &out[row]);
}

// Tile `tile` of a stripe of n dates, by the whole workgroup.  The stripe is cut into a head (one row, when the stripe
// starts 8 mod 16), groups of four rows from the first 16-byte boundary on, and a tail of fewer than four rows.  Tile t owns
// the groups [t * kTileGroups, (t + 1) * kTileGroups); the head belongs to tile 0 and the tail to the last tile.  Every group
// lies inside a tile that exists: group g starts at row head + 4 g <= n - 4, i.e. in tile <= (n - 1) / kExtractTileRows.
template <int kUnit>
__device__ __forceinline__ void extract_tile(const unsigned long long *__restrict__ in, int32_t *__restrict__ out, int64_t n, int64_t tile) {
  const int head = static_cast<int>((reinterpret_cast<uintptr_t>(in) >> 3) & 1);
  const int64_t groups = n > head ? (n - head) / kGroupRows : 0;
  const int64_t g0 = tile * kTileGroups + threadIdx.x;
  if (tile * kTileGroups < groups) {   // (uniform) every lane reads: a lane past the last group reads that group again, so
    uint4 raw[kGroupsPerLane][2];      // that all loads of the tile are issued before the first store waits for one
#pragma unroll
    for (int u = 0; u < kGroupsPerLane; ++u) {
      const int64_t g = g0 + u * kBlock < groups ? g0 + u * kBlock : groups - 1;
      const unsigned long long *src = in + head + g * kGroupRows;
      raw[u][0] = stream_load16(src);
      raw[u][1] = stream_load16(src + 2);
    }
#pragma unroll
    for (int u = 0; u < kGroupsPerLane; ++u) {
      const int64_t g = g0 + u * kBlock;
      if (g < groups) {
        u32x4_a4 v;
        v.x = field_of<kUnit>(raw[u][0].x, raw[u][0].y);
        v.y = field_of<kUnit>(raw[u][0].z, raw[u][0].w);
        v.z = field_of<kUnit>(raw[u][1].x, raw[u][1].y);
        v.w = field_of<kUnit>(raw[u][1].z, raw[u][1].w);
        __builtin_nontemporal_store(v, (__attribute__((address_space(1))) u32x4_a4 *)reinterpret_cast<uintptr_t>(out + head + g * kGroupRows));
      }
    }
  }
  if (tile == 0 && static_cast<int>(threadIdx.x) < head && n > 0) extract_row<kUnit>(in, out, 0);
  if (tile == (n - 1) / kExtractTileRows) {
    const int64_t row = head + groups * kGroupRows + threadIdx.x;   // (n >= 1 here: a stripe without rows has no tile)
    if (row < n) extract_row<kUnit>(in, out, row);
  }
}

template <int kUnit>
__global__ __launch_bounds__(kBlock) void date_extract_kernel(const unsigned long long *__restrict__ in, int64_t n, int32_t *__restrict__ out) {
  const int64_t num_tiles = (n + kExtractTileRows - 1) / kExtractTileRows;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) extract_tile<kUnit>(in, out, n, tile);
}

// Over a run of blocks (block_runs.hpp): a workgroup takes a contiguous range of the run's tiles.
template <int kUnit>
__global__ __launch_bounds__(kBlock) void date_extract_runs_kernel(const long long *__restrict__ runs) {
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    extract_tile<kUnit>(run_in<unsigned long long>(runs, at.block), run_out<int32_t>(runs, at.block), run_rows(runs, at.block), at.tile_in_block);
  }
}

// ---------------------------------------------------------------------------
// SUBSTRING
// ---------------------------------------------------------------------------
// The bytes [src, src + bytes) of a stripe -> LDS, by the whole workgroup; returns `data` with data[o] = src[o].  The image lies
// at the stripe's own offset within 16 bytes, so that data + o is 16-byte aligned where src + o is: the partial 16 bytes at
// either end travel byte by byte, everything between as 16-byte streaming loads.  Begins and ends with a barrier.
__device__ __forceinline__ unsigned char *stage_tile(const unsigned char *__restrict__ src, int bytes, unsigned char *s_in) {
  const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15);
  unsigned char *data = s_in + shift;
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
  return data;
}

// One tile (rows [row0, row0 + tile_rows) of a stripe).  The tile's bytes go to LDS as in like_tile: 16-byte streaming
// loads, the tile placed at the stripe's own offset within 16 bytes.  One lane computes one row; it looks for a NUL in bytes
// [0, start + m) only.  The results are written to a second LDS image, placed at the OUTPUT's own offset within 16 bytes, and
// leave the same way the input came: the partial 16 bytes at either end of the tile's output byte by byte (m is often 2, 3
// or 7: a tile's output neither starts nor ends on 16 bytes, and the neighbouring bytes are another tile's or not the
// stripe's at all), everything between as 16-byte stores.
__device__ __forceinline__ void substring_tile(const unsigned char *__restrict__ col, int width, int64_t n, int start, int m,
                                               unsigned char *__restrict__ out, int64_t row0, int tile_rows, unsigned char *s_in,
                                               unsigned char *s_out) {
  const int rows = static_cast<int>(n - row0 < tile_rows ? n - row0 : tile_rows);
  const unsigned char *data = stage_tile(col + row0 * width, rows * width, s_in);

  unsigned char *dst = out + row0 * m;
  const int out_bytes = rows * m;
  const int out_shift = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
  unsigned char *res = s_out + out_shift;   // res[o] -> dst[o]
  for (int r = threadIdx.x; r < rows; r += kBlock) {
    const unsigned char *t = data + r * width;
    bool ended = false;                       // the text ends in front of the byte looked at
    for (int j = 0; j < start; ++j) ended |= t[j] == 0;
    unsigned char *o = res + r * m;
    for (int j = 0; j < m; ++j) {
      const unsigned char c = ended ? static_cast<unsigned char>(0) : t[start + j];   // (bytes >= 0x80 as they are)
      ended |= c == 0;
      o[j] = c;
    }
  }
  __syncthreads();
  int out_head = out_shift != 0 ? 16 - out_shift : 0;
  if (out_head > out_bytes) out_head = out_bytes;
  const int out_full = (out_bytes - out_head) & ~15;
  for (int o = threadIdx.x; o < out_head; o += kBlock) dst[o] = res[o];
  for (int o = out_head + threadIdx.x * 16; o < out_head + out_full; o += kBlock * 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(res + o);
    u32x4 bits;
    bits.x = v.x, bits.y = v.y, bits.z = v.z, bits.w = v.w;
    __builtin_nontemporal_store(bits, (__attribute__((address_space(1))) u32x4 *)reinterpret_cast<uintptr_t>(dst + o));
  }
  for (int o = out_head + out_full + threadIdx.x; o < out_bytes; o += kBlock) dst[o] = res[o];
}

// LDS: the input image (in_bytes, a multiple of 16) followed by the output image.
__global__ __launch_bounds__(kBlock) void substring_kernel(const unsigned char *__restrict__ col, int width, int64_t n, int start, int m,
                                                          unsigned char *__restrict__ out, int tile_rows, int in_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const int64_t num_tiles = (n + tile_rows - 1) / tile_rows;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    substring_tile(col, width, n, start, m, out, tile * tile_rows, tile_rows, s_tile, s_tile + in_bytes);
  }
}

__global__ __launch_bounds__(kBlock) void substring_runs_kernel(const long long *__restrict__ runs, int width, int start, int m, int tile_rows,
                                                               int in_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    substring_tile(run_in<unsigned char>(runs, at.block), width, run_rows(runs, at.block), start, m, run_out<unsigned char>(runs, at.block),
                   static_cast<int64_t>(at.tile_in_block) * tile_rows, tile_rows, s_tile, s_tile + in_bytes);
  }
}

// rows per tile: a multiple of 64, at most 1024, input and output image together at most 48 KiB of LDS
static int substring_tile_rows(int width, int m) {
  int tile_rows = (48 * 1024 / (width + m)) / 64 * 64;
  if (tile_rows > 1024) tile_rows = 1024;
  if (tile_rows < 64) tile_rows = 64;
  return tile_rows;
}
// an image of `bytes` bytes placed up to 15 bytes into its buffer, in whole 16 bytes
static int image_bytes(int tile_rows, int row_bytes) { return (tile_rows * row_bytes + 15) / 16 * 16 + 16; }

static bool substring_arguments_ok(int width, int start, int length) {
  return width >= 1 && width <= 255 && start >= 0 && start < width && length >= 1;
}
static int substring_width(int width, int start, int length) { return width - start < length ? width - start : length; }

static bool extract_aligned(const void *dates, const void *out) {
  return (reinterpret_cast<uintptr_t>(dates) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
}

// ---------------------------------------------------------------------------
// PREDICATES OVER A UNARY OPERATION (qsx_select_cmp_unary, qsx_select_in_unary and their run forms)
// ---------------------------------------------------------------------------
// `EXTRACT(..) OP literal`, `SUBSTRING(..) IN (..)`: the reference evaluates the operand into a column vector
// (ScalarUnaryExpression::getAllValues, ScalarUnaryExpression.cpp:92-115) and compares that with the static value
// (ComparisonPredicate.cpp:209-240).  Here the operand's value of a row lives in registers only: one pass over the stripe,
// one bit per row out.
constexpr int kWavesPerBlock = kBlock / kWave;

// ---- a date's field ---------------------------------------------------------------------------------------------------------
// A lane reads 16 bytes = two dates per load and has kFieldLoads loads in flight; a wave's load covers 128 rows = two bitmap
// words.  The first dates of the lanes give one ballot (rows 0, 2, 4, ...), the second dates another (rows 1, 3, 5, ...):
// a bitmap word is the two ballots' halves interleaved — scalar work on wave-uniform values, no cross-lane traffic.
// A wave's unit of work (its "tile") is one group of kFieldLoads loads: 512 rows, eight bitmap words, which eight lanes
// write as one 64-byte store.
constexpr int kFieldLoads = 4;
constexpr int kFieldRowsPerLoad = 2 * kWave;
constexpr int kFieldTileRows = kFieldLoads * kFieldRowsPerLoad;   // 512
constexpr int kFieldTileWords = kFieldTileRows / 64;

// The six comparisons of an INT against a literal as one closed range and a negation: nothing overflows, and the kernel has one
// form for all of them.
struct FieldRange {
  int32_t lo, hi;
  bool negate;
  __device__ __forceinline__ bool operator()(int32_t v) const { return (v >= lo && v <= hi) != negate; }
};
static FieldRange field_range(int op, int32_t lit) {
  constexpr int32_t kMin = INT32_MIN, kMax = INT32_MAX;
  switch (op) {
    case QSX_EQ: return FieldRange{lit, lit, false};
    case QSX_NE: return FieldRange{lit, lit, true};
    case QSX_LT: return FieldRange{lit, kMax, true};    // not (v >= lit)
    case QSX_LE: return FieldRange{kMin, lit, false};
    case QSX_GT: return FieldRange{kMin, lit, true};    // not (v <= lit)
    default: return FieldRange{lit, kMax, false};       // QSX_GE
  }
}

// bit i of x -> bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t half) {
  uint64_t x = half;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// Tile `tile` of a stripe of n dates, by one wave; the matches are added to count (the same value in every lane).
template <int kUnit, typename Pred>
__device__ __forceinline__ void field_select_tile(const unsigned long long *__restrict__ in, int64_t n, const Pred &pred,
                                                  const uint64_t *__restrict__ filter, uint64_t *__restrict__ out, int64_t tile, int lane,
                                                  unsigned long long &count) {
  const int64_t row_base = tile * kFieldTileRows;
  const int64_t num_words = (n + 63) >> 6;
  const bool full = row_base + kFieldTileRows <= n;   // (uniform) every row of the tile exists: all tiles of a stripe but its last
  uint4 raw[kFieldLoads];
  if (full) {
#pragma unroll
    for (int r = 0; r < kFieldLoads; ++r) raw[r] = stream_load16(in + row_base + r * kFieldRowsPerLoad + 2 * lane);
  } else {
#pragma unroll
    for (int r = 0; r < kFieldLoads; ++r) {
      const int64_t row0 = row_base + r * kFieldRowsPerLoad + 2 * lane;
      raw[r] = make_uint4(0, 0, 0, 0);
      if (row0 + 2 <= n) {
        raw[r] = stream_load16(in + row0);
      } else if (row0 < n) {   // the stripe's last date stands alone
        const unsigned long long one = load_global_nt(&in[row0]);
        raw[r].x = static_cast<uint32_t>(one);
        raw[r].y = static_cast<uint32_t>(one >> 32);
      }
    }
  }
  const int64_t word_base = row_base >> 6;
  uint64_t mine = 0;
#pragma unroll
  for (int r = 0; r < kFieldLoads; ++r) {
    const int64_t row0 = row_base + r * kFieldRowsPerLoad + 2 * lane;
    bool first = pred(static_cast<int32_t>(field_of<kUnit>(raw[r].x, raw[r].y)));
    bool second = pred(static_cast<int32_t>(field_of<kUnit>(raw[r].z, raw[r].w)));
    if (!full) {
      first = first && row0 < n;
      second = second && row0 + 1 < n;
    }
    const uint64_t even = __ballot(first), odd = __ballot(second);   // bit l: row 2 l / row 2 l + 1 of the load
    uint64_t word0 = msb_first(spread_bits(static_cast<uint32_t>(even)) | (spread_bits(static_cast<uint32_t>(odd)) << 1));
    uint64_t word1 = msb_first(spread_bits(static_cast<uint32_t>(even >> 32)) | (spread_bits(static_cast<uint32_t>(odd >> 32)) << 1));
    if (filter != nullptr) {
      const int64_t w = word_base + 2 * r;
      if (full || w < num_words) word0 &= filter[w];
      if (full || w + 1 < num_words) word1 &= filter[w + 1];
    }
    count += __popcll(word0) + __popcll(word1);
    if (lane == 2 * r) mine = word0;
    if (lane == 2 * r + 1) mine = word1;
  }
  if (lane < kFieldTileWords && word_base + lane < num_words) out[word_base + lane] = mine;
}

template <int kUnit, typename Pred>
__global__ __launch_bounds__(kBlock) void field_select_kernel(const unsigned long long *__restrict__ in, int64_t n, Pred pred,
                                                             const uint64_t *__restrict__ filter, uint64_t *__restrict__ out,
                                                             unsigned long long *__restrict__ out_count) {
  const int lane = lane_id();
  const int64_t num_tiles = (n + kFieldTileRows - 1) / kFieldTileRows;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t num_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  unsigned long long count = 0;
  for (int64_t tile = wave; tile < num_tiles; tile += num_waves) field_select_tile<kUnit, Pred>(in, n, pred, filter, out, tile, lane, count);
  if (out_count != nullptr) {
    __shared__ unsigned long long block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    if (lane == 0 && count != 0) atomicAdd(&block_count, count);
    __syncthreads();
    if (threadIdx.x == 0 && block_count != 0) atomicAdd(out_count, block_count);
  }
}

// Over a run of blocks, as select.hip's select_packed_runs_kernel: a workgroup takes a contiguous range of the run's tiles,
// its waves interleaved inside it; a wave adds its matches to a block's counter when it moves on to another block, and the
// counts of the range's last block meet in LDS first.
template <int kUnit, typename Pred>
__global__ __launch_bounds__(kBlock) void field_select_runs_kernel(const long long *__restrict__ runs, Pred pred,
                                                                  unsigned long long *__restrict__ out_counts) {
  __shared__ unsigned long long s_last_count;
  const int lane = lane_id();
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (threadIdx.x == 0) s_last_count = 0;
  unsigned long long count = 0;
  int counted_block = -1;
  for (int tile = first + wave; tile < end; tile += kWavesPerBlock) {
    const RunTile at = run_locate(runs, tile);
    if (at.block != counted_block) {
      if (out_counts != nullptr && counted_block >= 0 && lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
      count = 0;
      counted_block = at.block;
    }
    field_select_tile<kUnit, Pred>(run_in<unsigned long long>(runs, at.block), run_rows(runs, at.block), pred, run_filter(runs, at.block),
                                   run_out<uint64_t>(runs, at.block), at.tile_in_block, lane, count);
  }
  if (out_counts == nullptr) return;
  const int last_block = end > first ? run_locate(runs, end - 1).block : -1;
  __syncthreads();   // s_last_count is zero
  if (lane == 0 && count != 0 && counted_block >= 0) {
    if (counted_block == last_block) atomicAdd(&s_last_count, count);
    else atomicAdd(&out_counts[counted_block], count);
  }
  __syncthreads();
  if (threadIdx.x == 0 && last_block >= 0 && s_last_count != 0) atomicAdd(&out_counts[last_block], s_last_count);
}

// ---- a substring ------------------------------------------------------------------------------------------------------------
// The window [start, start + m) of a CHAR(width) field as computeSubstring leaves it (SubstringOperation.cpp:74-91): the
// field's text ends at its first NUL, a window that begins behind the text's end is the empty string.  The tests below take a
// row's field in LDS; a window of up to 16 bytes becomes two big-endian 64-bit numbers in registers (zero behind the text's
// end: strcmpHelper on zero-padded strings is an unsigned compare of these numbers), a longer one is walked byte by byte.
__device__ __forceinline__ bool text_ends_before(const unsigned char *t, int start) {
  bool ended = false;
  for (int j = 0; j < start; ++j) ended |= t[j] == 0;
  return ended;
}
__device__ __forceinline__ void window16(const unsigned char *t, int start, int m, bool ended, unsigned long long &first,
                                         unsigned long long &second) {
  first = second = 0;
  for (int j = 0; j < m; ++j) {
    const unsigned long long c = ended ? 0u : t[start + j];   // (bytes >= 0x80 as they are)
    ended |= c == 0;
    if (j < 8) first |= c << (8 * (7 - j));
    else second |= c << (8 * (15 - j));
  }
}
// `window OP literal`, AsciiStringUncheckedComparator::strcmpHelper (AsciiStringComparators.hpp:218-251) between the CHAR(m)
// window and the literal: both end at their first NUL or at their maximum length, a proper prefix is smaller.
struct WindowCompare {
  int op;
  const CharLiteral &lit;
  unsigned long long key_first, key_second;   // the literal's bytes 0-7 / 8-15, big-endian, zero-padded
  __device__ __forceinline__ WindowCompare(int op_, const CharLiteral &lit_) : op(op_), lit(lit_), key_first(0), key_second(0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      key_first |= static_cast<unsigned long long>(i < lit.length ? lit.bytes[i] : 0) << (8 * (7 - i));
      key_second |= static_cast<unsigned long long>(8 + i < lit.length ? lit.bytes[8 + i] : 0) << (8 * (7 - i));
    }
  }
  __device__ __forceinline__ bool operator()(const unsigned char *t, int start, int m) const {
    const bool ended = text_ends_before(t, start);
    int res = 0;
    if (m <= 16) {
      unsigned long long first, second;
      window16(t, start, m, ended, first, second);
      // sixteen equal bytes and the literal goes on: the window is a proper prefix of it
      res = first != key_first ? (first < key_first ? -1 : 1) : (second != key_second ? (second < key_second ? -1 : 1) : (lit.length > 16 ? -1 : 0));
    } else {
      const int longest = m > lit.length ? m : lit.length;
      for (int i = 0; i < longest; ++i) {
        const unsigned char a = i < m && !ended ? t[start + i] : 0;
        const unsigned char b = i < lit.length ? lit.bytes[i] : 0;
        if (a != b) {
          res = a < b ? -1 : 1;
          break;
        }
        if (a == 0) break;
      }
    }
    return compare_op<int>(res, op, 0);
  }
};
// `window IN (list)`: the list as select_in_char_kernel holds it, made by the host for fields of width m.
struct WindowInList {
  const CharInList *__restrict__ list;
  __device__ __forceinline__ bool operator()(const unsigned char *t, int start, int m) const {
    const bool ended = text_ends_before(t, start);
    if (m <= 16) {
      unsigned long long first, second;
      window16(t, start, m, ended, first, second);
      return CharInCompare{list}.match16(CharInCompare::Key16{}, first, second);
    }
    int len = 0;   // of the window's text
    if (!ended) {
      while (len < m && t[start + len] != 0) ++len;
    }
    bool any = false;
    const int count = static_cast<int>(list->count);
    for (int i = 0; i < count && !any; ++i) {
      bool same = static_cast<int>(list->length[i]) == len;
      for (int j = 0; j < len && same; ++j) same = t[start + j] == list->bytes[i][j];
      any = same;
    }
    return any != (list->negate != 0);
  }
};

// One tile (rows [row0, row0 + tile_rows) of a stripe) by the whole workgroup: the tile's bytes go to LDS (stage_tile), a lane
// tests a row, a wave's ballot is a bitmap word; lane 0 of every wave adds its words' bits to count.
template <typename Test>
__device__ __forceinline__ void substring_select_tile(const unsigned char *__restrict__ col, int width, int64_t n, int start, int m,
                                                      const Test &test, const uint64_t *__restrict__ filter, uint64_t *__restrict__ out,
                                                      int64_t row0, int tile_rows, unsigned char *s_in, unsigned long long &count) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int rows = static_cast<int>(n - row0 < tile_rows ? n - row0 : tile_rows);
  const unsigned char *data = stage_tile(col + row0 * width, rows * width, s_in);
  for (int w = wave; w * 64 < rows; w += kWavesPerBlock) {
    const int r = w * 64 + lane;
    bool pred = false;
    if (r < rows) pred = test(data + r * width, start, m);
    uint64_t word = msb_first(__ballot(pred));
    const int64_t word_index = (row0 >> 6) + w;
    if (filter != nullptr) word &= filter[word_index];
    if (lane == 0) {
      out[word_index] = word;
      count += __popcll(word);
    }
  }
}

// the counts of a workgroup's waves (lane 0 of each holds one) -> *out_count
__device__ __forceinline__ void add_block_count(unsigned long long count, unsigned long long *__restrict__ out_count) {
  if (out_count == nullptr) return;
  __shared__ unsigned long long block_count;
  if (threadIdx.x == 0) block_count = 0;
  __syncthreads();
  if (lane_id() == 0 && count != 0) atomicAdd(&block_count, count);
  __syncthreads();
  if (threadIdx.x == 0 && block_count != 0) atomicAdd(out_count, block_count);
}

__global__ __launch_bounds__(kBlock) void substring_cmp_kernel(const unsigned char *__restrict__ col, int width, int64_t n, int start, int m,
                                                              int op, CharLiteral lit, const uint64_t *__restrict__ filter,
                                                              uint64_t *__restrict__ out, unsigned long long *__restrict__ out_count,
                                                              int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const WindowCompare test(op, lit);
  const int64_t num_tiles = (n + tile_rows - 1) / tile_rows;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    substring_select_tile(col, width, n, start, m, test, filter, out, tile * tile_rows, tile_rows, s_tile, count);
  }
  add_block_count(count, out_count);
}
__global__ __launch_bounds__(kBlock) void substring_in_kernel(const unsigned char *__restrict__ col, int width, int64_t n, int start, int m,
                                                             const CharInList *__restrict__ list, const uint64_t *__restrict__ filter,
                                                             uint64_t *__restrict__ out, unsigned long long *__restrict__ out_count,
                                                             int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const int64_t num_tiles = (n + tile_rows - 1) / tile_rows;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    substring_select_tile(col, width, n, start, m, WindowInList{list}, filter, out, tile * tile_rows, tile_rows, s_tile, count);
  }
  add_block_count(count, out_count);
}

// Over a run of blocks (as select.hip's select_char_runs_kernel): a workgroup takes a contiguous range of the run's tiles, a
// wave adds its matches to a block's counter when the workgroup moves on to another block.  kIn: the list lies behind the run
// table at word `extra`.
template <bool kIn>
__global__ __launch_bounds__(kBlock) void substring_select_runs_kernel(const long long *__restrict__ runs, int width, int start, int m, int op,
                                                                      CharLiteral lit, long long extra,
                                                                      unsigned long long *__restrict__ out_counts, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_tile[];
  const int lane = lane_id();
  const WindowCompare compare(op, lit);
  const WindowInList in_list{reinterpret_cast<const CharInList *>(runs + extra)};
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
    const unsigned char *col = run_in<unsigned char>(runs, at.block);
    const int64_t row0 = static_cast<int64_t>(at.tile_in_block) * tile_rows;
    if constexpr (kIn) {
      substring_select_tile(col, width, run_rows(runs, at.block), start, m, in_list, run_filter(runs, at.block),
                            run_out<uint64_t>(runs, at.block), row0, tile_rows, s_tile, count);
    } else {
      substring_select_tile(col, width, run_rows(runs, at.block), start, m, compare, run_filter(runs, at.block),
                            run_out<uint64_t>(runs, at.block), row0, tile_rows, s_tile, count);
    }
  }
  if (out_counts != nullptr && counted_block >= 0 && lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static bool comparison_ok(int op) { return op >= QSX_EQ && op <= QSX_GE; }
static bool in_list_ok(const void *literals, int num_literals, int negate) {
  return literals != nullptr && num_literals >= 1 && num_literals <= QSX_MAX_IN_LIST && (negate == 0 || negate == 1);
}
// The operand and the stripe's width: QSX_OK, or the status of the composed calls (qsx_eval_date_extract / qsx_eval_substring).
static int unary_operand_status(const qsx_unary_operand_t *operand, int width) {
  if (operand == nullptr) return QSX_ERR_INVALID_ARGUMENT;
  if (operand->kind == QSX_UNARY_DATE_FIELD) {
    if (width != 8) return QSX_ERR_INVALID_ARGUMENT;
    return operand->unit == QSX_DATE_YEAR || operand->unit == QSX_DATE_MONTH ? QSX_OK : QSX_ERR_UNSUPPORTED;
  }
  if (operand->kind == QSX_UNARY_SUBSTRING) return substring_arguments_ok(width, operand->start, operand->length) ? QSX_OK : QSX_ERR_INVALID_ARGUMENT;
  return QSX_ERR_UNSUPPORTED;
}
static bool date_aligned(const void *dates) { return (reinterpret_cast<uintptr_t>(dates) & 7) == 0; }

template <typename Pred>
static int launch_field_select(int unit, const void *col, int64_t n, const Pred &pred, const uint64_t *filter, uint64_t *out, int64_t *out_count,
                               hipStream_t s) {
  const int grid = grid_for((n + kFieldTileRows - 1) / kFieldTileRows, kWavesPerBlock);
  const unsigned long long *in = static_cast<const unsigned long long *>(col);
  unsigned long long *count = reinterpret_cast<unsigned long long *>(out_count);
  if (unit == QSX_DATE_YEAR) hipLaunchKernelGGL((field_select_kernel<QSX_DATE_YEAR, Pred>), dim3(grid), dim3(kBlock), 0, s, in, n, pred, filter, out, count);
  else hipLaunchKernelGGL((field_select_kernel<QSX_DATE_MONTH, Pred>), dim3(grid), dim3(kBlock), 0, s, in, n, pred, filter, out, count);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}
template <typename Pred>
static int launch_field_select_runs(int unit, const long long *runs_dev, long long tiles, const Pred &pred, int64_t *out_counts, hipStream_t s) {
  const int grid = grid_for(tiles, kWavesPerBlock);
  unsigned long long *counts = reinterpret_cast<unsigned long long *>(out_counts);
  if (unit == QSX_DATE_YEAR) hipLaunchKernelGGL((field_select_runs_kernel<QSX_DATE_YEAR, Pred>), dim3(grid), dim3(kBlock), 0, s, runs_dev, pred, counts);
  else hipLaunchKernelGGL((field_select_runs_kernel<QSX_DATE_MONTH, Pred>), dim3(grid), dim3(kBlock), 0, s, runs_dev, pred, counts);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}
// The run table of a `_blocks` call (inputs, filters, output bitmaps), its counters zeroed; *tiles == 0: nothing to launch.
static int select_run_table(RunTable *table, long long tile_rows, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols,
                            const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps, int64_t *out_counts_dev, hipStream_t s,
                            long long *tiles) {
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  *tiles = table->build(tile_rows, num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_filters),
                        reinterpret_cast<void *const *>(block_out_bitmaps), nullptr);
  return *tiles < 0 ? QSX_ERR_INVALID_ARGUMENT : QSX_OK;
}

}  // namespace unary
}  // namespace qsx

using namespace qsx;
using namespace qsx::unary;

extern "C" {

int qsx_eval_date_extract(int unit, const void *dates_dev, int64_t n, int32_t *out_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || (n > 0 && (dates_dev == nullptr || out_dev == nullptr)) || !extract_aligned(dates_dev, out_dev)) return QSX_ERR_INVALID_ARGUMENT;
  if (unit != QSX_DATE_YEAR && unit != QSX_DATE_MONTH) return QSX_ERR_UNSUPPORTED;
  if (n == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  const int grid = grid_for(n, kExtractTileRows);
  const unsigned long long *in = static_cast<const unsigned long long *>(dates_dev);
  if (unit == QSX_DATE_YEAR) hipLaunchKernelGGL(date_extract_kernel<QSX_DATE_YEAR>, dim3(grid), dim3(kBlock), 0, s, in, n, out_dev);
  else hipLaunchKernelGGL(date_extract_kernel<QSX_DATE_MONTH>, dim3(grid), dim3(kBlock), 0, s, in, n, out_dev);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_eval_date_extract_blocks(int unit, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols,
                                 int32_t *const *block_out, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  if (unit != QSX_DATE_YEAR && unit != QSX_DATE_MONTH) return QSX_ERR_UNSUPPORTED;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_out))) return QSX_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < num_blocks; ++b) {
    if (!extract_aligned(block_cols[b], block_out[b])) return QSX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = as_stream(stream);
  RunTable table;
  const long long tiles = table.build(kExtractTileRows, num_blocks, block_rows, block_cols, nullptr, reinterpret_cast<void *const *>(block_out), nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  const long long *runs_dev = table.dev();
  const int grid = grid_for(tiles, 1);
  if (unit == QSX_DATE_YEAR) hipLaunchKernelGGL(date_extract_runs_kernel<QSX_DATE_YEAR>, dim3(grid), dim3(kBlock), 0, s, runs_dev);
  else hipLaunchKernelGGL(date_extract_runs_kernel<QSX_DATE_MONTH>, dim3(grid), dim3(kBlock), 0, s, runs_dev);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_eval_substring(const void *col_dev, int width, int64_t n, int start, int length, void *out_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || !substring_arguments_ok(width, start, length) || (n > 0 && (col_dev == nullptr || out_dev == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  if (n == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  const int m = substring_width(width, start, length);
  const int tile_rows = substring_tile_rows(width, m);
  const int in_bytes = image_bytes(tile_rows, width);
  const int64_t tiles = (n + tile_rows - 1) / tile_rows;
  const int grid = tile_grid(tiles);
  hipLaunchKernelGGL(substring_kernel, dim3(grid), dim3(kBlock), static_cast<size_t>(in_bytes + image_bytes(tile_rows, m)), s,
                     static_cast<const unsigned char *>(col_dev), width, n, start, m, static_cast<unsigned char *>(out_dev), tile_rows, in_bytes);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_eval_substring_blocks(int width, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols, int start, int length,
                              void *const *block_out, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || !substring_arguments_ok(width, start, length) ||
      (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, block_out)) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  const int m = substring_width(width, start, length);
  const int tile_rows = substring_tile_rows(width, m);
  const int in_bytes = image_bytes(tile_rows, width);
  RunTable table;
  const long long tiles = table.build(tile_rows, num_blocks, block_rows, block_cols, nullptr, block_out, nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  const long long *runs_dev = table.dev();
  const int grid = tile_grid(tiles);
  hipLaunchKernelGGL(substring_runs_kernel, dim3(grid), dim3(kBlock), static_cast<size_t>(in_bytes + image_bytes(tile_rows, m)), s, runs_dev,
                     width, start, m, tile_rows, in_bytes);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_cmp_unary(const qsx_unary_operand_t *operand, const void *col_dev, int width, int64_t n, int op, const void *literal,
                         int literal_length, const uint64_t *filter_dev, uint64_t *out_bitmap_dev, int64_t *out_count_dev,
                         qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || !comparison_ok(op) || (n > 0 && (col_dev == nullptr || out_bitmap_dev == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  const int status = unary_operand_status(operand, width);
  if (status == QSX_ERR_INVALID_ARGUMENT) return status;
  hipStream_t s = as_stream(stream);
  if (operand->kind == QSX_UNARY_DATE_FIELD) {
    if (literal == nullptr || !date_aligned(col_dev)) return QSX_ERR_INVALID_ARGUMENT;
    if (status != QSX_OK) return status;
    if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
    if (n == 0) return QSX_OK;
    int32_t lit;
    std::memcpy(&lit, literal, sizeof(lit));
    return launch_field_select(operand->unit, col_dev, n, field_range(op, lit), filter_dev, out_bitmap_dev, out_count_dev, s);
  }
  if (status != QSX_OK) return status;
  if (literal_length < 0 || (literal_length > 0 && literal == nullptr)) return QSX_ERR_INVALID_ARGUMENT;
  if (literal_length > QSX_MAX_CHAR_LITERAL) return QSX_ERR_UNSUPPORTED;
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return QSX_OK;
  const int tile_rows = char_tile_rows(width);
  const int64_t tiles = (n + tile_rows - 1) / tile_rows;
  hipLaunchKernelGGL(substring_cmp_kernel, dim3(tile_grid(tiles)), dim3(kBlock), static_cast<size_t>(image_bytes(tile_rows, width)), s,
                     static_cast<const unsigned char *>(col_dev), width, n, operand->start, substring_width(width, operand->start, operand->length),
                     op, char_literal(literal, literal_length), filter_dev, out_bitmap_dev, reinterpret_cast<unsigned long long *>(out_count_dev),
                     tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_in_unary(const qsx_unary_operand_t *operand, const void *col_dev, int width, int64_t n, const void *literals,
                        const int32_t *literal_lengths, int num_literals, int negate, const uint64_t *filter_dev, uint64_t *out_bitmap_dev,
                        int64_t *out_count_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || !in_list_ok(literals, num_literals, negate) || (n > 0 && (col_dev == nullptr || out_bitmap_dev == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  const int status = unary_operand_status(operand, width);
  if (status == QSX_ERR_INVALID_ARGUMENT) return status;
  hipStream_t s = as_stream(stream);
  if (operand->kind == QSX_UNARY_DATE_FIELD) {
    if (!date_aligned(col_dev)) return QSX_ERR_INVALID_ARGUMENT;
    if (status != QSX_OK) return status;
    if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
    if (n == 0) return QSX_OK;
    return launch_field_select(operand->unit, col_dev, n, in_list_pred<int32_t>(literals, num_literals, negate), filter_dev, out_bitmap_dev,
                               out_count_dev, s);
  }
  if (status != QSX_OK) return status;
  if (literal_lengths == nullptr) return QSX_ERR_INVALID_ARGUMENT;
  const int m = substring_width(width, operand->start, operand->length);
  CharInList list;
  int rc = char_in_list(m, literals, literal_lengths, num_literals, negate, &list);
  if (rc != QSX_OK) return rc;
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return QSX_OK;
  const CharInList *list_dev = nullptr;
  rc = staged_table(s, &list, sizeof(list), &list_dev);
  if (rc != QSX_OK) return rc;
  const int tile_rows = char_tile_rows(width);
  const int64_t tiles = (n + tile_rows - 1) / tile_rows;
  hipLaunchKernelGGL(substring_in_kernel, dim3(tile_grid(tiles)), dim3(kBlock), static_cast<size_t>(image_bytes(tile_rows, width)), s,
                     static_cast<const unsigned char *>(col_dev), width, n, operand->start, m, list_dev, filter_dev, out_bitmap_dev,
                     reinterpret_cast<unsigned long long *>(out_count_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_cmp_unary_blocks(const qsx_unary_operand_t *operand, int width, int64_t num_blocks, const int64_t *block_rows,
                                const void *const *block_cols, int op, const void *literal, int literal_length,
                                const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps, int64_t *out_counts_dev,
                                qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || !comparison_ok(op) || (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  const int status = unary_operand_status(operand, width);
  if (status == QSX_ERR_INVALID_ARGUMENT) return status;
  const bool dates = operand->kind == QSX_UNARY_DATE_FIELD;
  if (dates ? literal == nullptr : (literal_length < 0 || (literal_length > 0 && literal == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  if (status != QSX_OK) return status;
  if (!dates && literal_length > QSX_MAX_CHAR_LITERAL) return QSX_ERR_UNSUPPORTED;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_out_bitmaps))) return QSX_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < num_blocks && dates; ++b) {
    if (!date_aligned(block_cols[b])) return QSX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = as_stream(stream);
  const int tile_rows = dates ? kFieldTileRows : char_tile_rows(width);
  RunTable table;
  long long tiles = 0;
  int rc = select_run_table(&table, tile_rows, num_blocks, block_rows, block_cols, block_filters, block_out_bitmaps, out_counts_dev, s, &tiles);
  if (rc != QSX_OK || tiles == 0) return rc;
  rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  if (dates) {
    int32_t lit;
    std::memcpy(&lit, literal, sizeof(lit));
    return launch_field_select_runs(operand->unit, table.dev(), tiles, field_range(op, lit), out_counts_dev, s);
  }
  hipLaunchKernelGGL(substring_select_runs_kernel<false>, dim3(tile_grid(tiles)), dim3(kBlock), static_cast<size_t>(image_bytes(tile_rows, width)), s,
                     table.dev(), width, operand->start, substring_width(width, operand->start, operand->length), op,
                     char_literal(literal, literal_length), 0ll, reinterpret_cast<unsigned long long *>(out_counts_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_select_in_unary_blocks(const qsx_unary_operand_t *operand, int width, int64_t num_blocks, const int64_t *block_rows,
                               const void *const *block_cols, const void *literals, const int32_t *literal_lengths, int num_literals,
                               int negate, const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps,
                               int64_t *out_counts_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || !in_list_ok(literals, num_literals, negate) ||
      (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  const int status = unary_operand_status(operand, width);
  if (status == QSX_ERR_INVALID_ARGUMENT) return status;
  const bool dates = operand->kind == QSX_UNARY_DATE_FIELD;
  if (!dates && literal_lengths == nullptr) return QSX_ERR_INVALID_ARGUMENT;
  if (status != QSX_OK) return status;
  CharInList list;
  int m = 0;
  if (!dates) {
    m = substring_width(width, operand->start, operand->length);
    const int rc = char_in_list(m, literals, literal_lengths, num_literals, negate, &list);
    if (rc != QSX_OK) return rc;
  }
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_out_bitmaps))) return QSX_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < num_blocks && dates; ++b) {
    if (!date_aligned(block_cols[b])) return QSX_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = as_stream(stream);
  const int tile_rows = dates ? kFieldTileRows : char_tile_rows(width);
  RunTable table;
  long long tiles = 0;
  int rc = select_run_table(&table, tile_rows, num_blocks, block_rows, block_cols, block_filters, block_out_bitmaps, out_counts_dev, s, &tiles);
  if (rc != QSX_OK || tiles == 0) return rc;
  const long long extra = dates ? 0 : table.append(sizeof(CharInList) / 8, reinterpret_cast<const long long *>(&list));
  rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  if (dates) {
    return launch_field_select_runs(operand->unit, table.dev(), tiles, in_list_pred<int32_t>(literals, num_literals, negate), out_counts_dev, s);
  }
  hipLaunchKernelGGL(substring_select_runs_kernel<true>, dim3(tile_grid(tiles)), dim3(kBlock), static_cast<size_t>(image_bytes(tile_rows, width)), s,
                     table.dev(), width, operand->start, m, static_cast<int>(QSX_EQ), CharLiteral{}, extra,
                     reinterpret_cast<unsigned long long *>(out_counts_dev), tile_rows);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

}  // extern "C"
