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
#include <vector>

#include "common.hpp"
#include "block_runs.hpp"

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
  const unsigned char *src = col + row0 * width;
  const int bytes = rows * width;
  const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15);
  unsigned char *data = s_in + shift;   // data[o] = src[o]; data + o is 16-byte aligned where src + o is
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

}  // extern "C"
