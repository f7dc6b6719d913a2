// cmp_columns.hip — attribute OP attribute over a run of blocks, every operand read as its block holds it
// (qsx_select_cmp_columns_blocks): values, 1 / 2 / 4-byte truncated values or 1 / 2 / 4-byte codes into the block's own dictionary.
//
// Replaces LiteralUncheckedComparator<Functor, LeftCppType, .., RightCppType, ..>::compareSingleValueAccessor / compareColumnVectors
// (types/operations/comparisons/LiteralComparators-inl.hpp:52-125) as reached from ComparisonPredicate::getAllMatches
// (expressions/predicate/ComparisonPredicate.cpp:243-333), one SelectWorkOrder per block in the reference.  The functor is the C++
// expression `left OP right` on the two C++ types (LiteralComparators.hpp:37-80), so an operand pair is compared in the type C++'s
// usual arithmetic conversions give it: INT with LONG in int64, INT or LONG with FLOAT in float, anything with DOUBLE in double.
//
// ONE kernel for every pair of types: what differs between them is a conversion of registers after the loads (as_long / as_float /
// as_double below), chosen by wave-uniform selects.  What the kernel is specialised on is how the two operands LIE — 1, 2, 4 or 8 bytes an element —
// because that decides the loads: sixteen instances of load_pair, one of which a tile takes.
//
// A tile is 4096 rows of ONE block (block_runs.hpp); its workgroup's four waves take the tile's eight batches of 512 rows in turn.
// A lane owns 8 rows of a batch, as K consecutive rows in each of 8 / K steps: K = 8 where an operand lies 1 or 2 bytes wide (a lane
// then reads 8 or 16 bytes of it at once), K = 2 where both lie 4 or 8 bytes wide (8 or 16 bytes again, the wave's loads contiguous).
// The form of the operands is the same for the whole tile and is chosen once, outside the loads: a batch issues all loads of both
// operands in one basic block, then the dictionary lookups as a second batch (through the cache: a block's date dictionary is about
// 20 KB), then converts and compares.  The lanes that share a bitmap word merge their K-bit masks with xor shuffles (as
// select_packed_group, select.hip).
#include <vector>

#include "common.hpp"
#include "block_runs.hpp"

namespace qsx {
namespace cmp_columns {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kLaneRows = 8;                          // rows of a batch a lane owns
constexpr int kBatchRows = kWave * kLaneRows;         // 512: 8 bitmap words
constexpr int kTileBatches = 8;
constexpr long long kTileRows = static_cast<long long>(kBatchRows) * kTileBatches;   // 4096
// the words behind the run table, per block: the right operand's stripe, code width, dictionary and code count, then the left
// operand's code count (its stripe, code width and dictionary are the table's own in / code_width / dictionary arrays)
enum ExtraArray { kRhsIn = 0, kRhsCodeWidth, kRhsDictionary, kRhsNumCodes, kLhsNumCodes, kExtraArrays };
// the type the pair is compared in: int64 (INT / LONG pairs; DATE pairs by their ordered key), float, double
enum CompareClass { kClassLong = 0, kClassFloat, kClassDouble };

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct Operand {              // uniform over the tile
  uintptr_t stripe;
  uintptr_t dictionary;       // 0: values, or truncated values
  unsigned long long num_codes;
  int type;
};
struct Compare {              // uniform over the launch
  int cls;
  bool lt, eq, gt, negate;    // a OP b == ((lt && a < b) || (eq && a == b) || (gt && a > b)) != negate; a NaN: all three false, only != holds
};

// The 8 rows of a lane as zero-extended elements of W bytes: rows [row_base, row_base + 512) all exist.  The address is the
// batch's (uniform) plus a 32-bit lane offset.
template <int W, int K>
__device__ __forceinline__ void issue_loads(uintptr_t stripe, int64_t row_base, int lane, uint32_t (&raw)[kLaneRows / K][K * W / 4]) {
  constexpr int S = kLaneRows / K;
  constexpr int kBytes = K * W;        // of a lane in a step: 8, 16, 32 or 64
  static_assert(kBytes == 8 || kBytes % 16 == 0, "a lane reads 8 bytes or whole 16-byte pieces");
  const uintptr_t batch = stripe + static_cast<uintptr_t>(row_base) * W;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uintptr_t p = batch + static_cast<uint32_t>((s * (kWave * K) + lane * K) * W);
    if constexpr (kBytes == 8) {
      const u32x2 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x2 *)p);
      raw[s][0] = v.x;
      raw[s][1] = v.y;
    } else {
#pragma unroll
      for (int c = 0; c < kBytes / 16; ++c) {
        const u32x4 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4 *)(p + 16 * c));
        raw[s][4 * c] = v.x;
        raw[s][4 * c + 1] = v.y;
        raw[s][4 * c + 2] = v.z;
        raw[s][4 * c + 3] = v.w;
      }
    }
  }
}
template <int W, int K>
__device__ __forceinline__ void unpack(const uint32_t (&raw)[kLaneRows / K][K * W / 4], uint64_t (&bits)[kLaneRows]) {
#pragma unroll
  for (int s = 0; s < kLaneRows / K; ++s) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint64_t e;
      if constexpr (W == 1) e = (raw[s][j / 4] >> (8 * (j % 4))) & 0xFFu;
      else if constexpr (W == 2) e = (raw[s][j / 2] >> (16 * (j % 2))) & 0xFFFFu;
      else if constexpr (W == 4) e = raw[s][j];
      else e = static_cast<uint64_t>(raw[s][2 * j]) | (static_cast<uint64_t>(raw[s][2 * j + 1]) << 32);
      bits[s * K + j] = e;
    }
  }
}
// The same for the last batch of a block, element by element: a row behind the block reads the block's last row (its bit is
// masked out of the word).
template <int W, int K>
__device__ __forceinline__ void load_clamped(uintptr_t stripe, int64_t row_base, int lane, int64_t n, uint64_t (&bits)[kLaneRows]) {
  typedef typename BitsOfSize<W>::type Bits;
#pragma unroll
  for (int i = 0; i < kLaneRows; ++i) {
    const int64_t row = row_base + (i / K) * (kWave * K) + lane * K + (i % K);
    bits[i] = load_global_nt(reinterpret_cast<const Bits *>(stripe) + (row < n ? row : n - 1));
  }
}

// Codes -> dictionary indices; bit i of the result: element i is not the NULL code.  A code >= num_codes is the reference's NULL
// code (CompressedTupleStorageSubBlock.hpp:225-300: the code past the dictionary): the dictionary is not read for it — the lookup
// goes to entry 0 and its value is never looked at.  (num_codes >= 1 here.)
__device__ __forceinline__ uint32_t clamp_codes(unsigned long long num_codes, uint64_t (&bits)[kLaneRows]) {
  uint32_t valid = 0;
#pragma unroll
  for (int i = 0; i < kLaneRows; ++i) {
    const bool ok = bits[i] < num_codes;
    valid |= ok ? 1u << i : 0u;
    bits[i] = ok ? bits[i] : 0ull;
  }
  return valid;
}
template <typename Bits>
__device__ __forceinline__ void lookup(uintptr_t dictionary, uint64_t (&bits)[kLaneRows]) {
#pragma unroll
  for (int i = 0; i < kLaneRows; ++i) bits[i] = load_global(reinterpret_cast<const Bits *>(dictionary) + bits[i]);
}
__device__ __forceinline__ bool wide(int type) { return type != QSX_INT && type != QSX_FLOAT; }   // 8-byte values (LONG, DOUBLE, DATE)
// One operand's codes -> the values they stand for (a truncated value is its own zero-extended code).
__device__ __forceinline__ uint32_t resolve_codes(const Operand &o, uint64_t (&bits)[kLaneRows]) {
  if (o.dictionary == 0) return 0xFFu;
  if (o.num_codes == 0) return 0u;                    // every code of the block is the NULL code; there is no entry 0
  const uint32_t valid = clamp_codes(o.num_codes, bits);
  if (wide(o.type)) lookup<uint64_t>(o.dictionary, bits);
  else lookup<uint32_t>(o.dictionary, bits);
  return valid;
}

// An element of an operand (the bits of a value of `type`, a 4-byte one zero-extended) as a value of the class's type.  The
// choices are uniform selects, element by element, so that no second copy of the operands' registers is alive anywhere.
// A DATE becomes year * 65536 + month * 256 + day (DateLit's order, types/DatetimeLit.hpp:65-90; the padding is never looked at).
__device__ __forceinline__ int32_t low_int(uint64_t bits) { return static_cast<int32_t>(static_cast<uint32_t>(bits)); }
__device__ __forceinline__ int64_t as_long(uint64_t bits, int type) {
  return type == QSX_INT ? static_cast<int64_t>(low_int(bits)) : type == QSX_DATE ? static_cast<int64_t>(date_ordered(bits)) : static_cast<int64_t>(bits);
}
__device__ __forceinline__ float as_float(uint64_t bits, int type) {
  return type == QSX_INT ? static_cast<float>(low_int(bits)) : type == QSX_LONG ? static_cast<float>(static_cast<int64_t>(bits))
                                                                                 : __uint_as_float(static_cast<uint32_t>(bits));
}
__device__ __forceinline__ double as_double(uint64_t bits, int type) {
  return type == QSX_INT ? static_cast<double>(low_int(bits)) : type == QSX_LONG ? static_cast<double>(static_cast<int64_t>(bits))
         : type == QSX_FLOAT ? static_cast<double>(__uint_as_float(static_cast<uint32_t>(bits))) : __longlong_as_double(static_cast<long long>(bits));
}
template <typename C>
__device__ __forceinline__ bool holds(const Compare &c, C x, C y) {
  return ((c.lt && x < y) || (c.eq && x == y) || (c.gt && x > y)) != c.negate;
}
// bit i: element i of a OP element i of b
__device__ __forceinline__ uint32_t compare_all(const Compare &c, int lhs_type, int rhs_type, const uint64_t (&a)[kLaneRows],
                                                const uint64_t (&b)[kLaneRows]) {
  uint32_t hits = 0;
  if (c.cls == kClassLong) {
#pragma unroll
    for (int i = 0; i < kLaneRows; ++i) hits |= holds(c, as_long(a[i], lhs_type), as_long(b[i], rhs_type)) ? 1u << i : 0u;
  } else if (c.cls == kClassFloat) {
#pragma unroll
    for (int i = 0; i < kLaneRows; ++i) hits |= holds(c, as_float(a[i], lhs_type), as_float(b[i], rhs_type)) ? 1u << i : 0u;
  } else {
#pragma unroll
    for (int i = 0; i < kLaneRows; ++i) hits |= holds(c, as_double(a[i], lhs_type), as_double(b[i], rhs_type)) ? 1u << i : 0u;
  }
  return hits;
}

// The lane's 8 rows of both operands, which lie LW and RW bytes an element: rows [row_base, row_base + 512) of a block of n rows
// (row_base < n).  All loads of the two operands stand in one basic block.
template <int LW, int RW>
__device__ __forceinline__ void load_pair(uintptr_t lhs, uintptr_t rhs, int64_t n, int64_t row_base, int lane, uint64_t (&a)[kLaneRows],
                                          uint64_t (&b)[kLaneRows]) {
  constexpr int K = (LW <= 2 || RW <= 2) ? 8 : 2;
  constexpr int S = kLaneRows / K;
  if (row_base + kBatchRows <= n) {
    uint32_t raw_a[S][K * LW / 4], raw_b[S][K * RW / 4];
    issue_loads<LW, K>(lhs, row_base, lane, raw_a);
    issue_loads<RW, K>(rhs, row_base, lane, raw_b);
    unpack<LW, K>(raw_a, a);
    unpack<RW, K>(raw_b, b);
  } else {
    load_clamped<LW, K>(lhs, row_base, lane, n, a);
    load_clamped<RW, K>(rhs, row_base, lane, n, b);
  }
}

// The rest of a batch, the same for every form with the same K: codes to values, values to the class's type, the comparison,
// and the bitmap words row_base / 64 ...
template <int K>
__device__ __forceinline__ void finish_batch(const Operand &lhs, const Operand &rhs, const Compare &cmp, int64_t n, int64_t row_base,
                                             uint64_t (&a)[kLaneRows], uint64_t (&b)[kLaneRows], const uint64_t *__restrict__ filter,
                                             uint64_t *__restrict__ out, int lane, unsigned long long &count) {
  constexpr int S = kLaneRows / K;
  constexpr int G = kWave / K;               // lanes per bitmap word
  uint32_t valid;
  if (lhs.dictionary != 0 && rhs.dictionary != 0 && lhs.num_codes != 0 && rhs.num_codes != 0 && wide(lhs.type) && wide(rhs.type)) {
    // both sides through dictionaries of 8-byte values (dates): the sixteen lookups as one batch
    valid = clamp_codes(lhs.num_codes, a) & clamp_codes(rhs.num_codes, b);
    lookup<uint64_t>(lhs.dictionary, a);
    lookup<uint64_t>(rhs.dictionary, b);
  } else {
    valid = resolve_codes(lhs, a);
    valid &= resolve_codes(rhs, b);
  }
  const uint32_t hits = compare_all(cmp, lhs.type, rhs.type, a, b) & valid;
  const int64_t num_words = (n + 63) >> 6;
  const int tail = static_cast<int>(n & 63);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    // the K bits of this step, first row = most significant bit
    unsigned long long m = __brev((hits >> (s * K)) & ((1u << K) - 1u)) >> (32 - K);
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {        // after step d the lower lane of every 2d-group holds 2d * K bits
      const unsigned long long other = __shfl_xor(m, d, kWave);
      m = (m << (d * K)) | other;
    }
    const int64_t word = (row_base >> 6) + s * K + lane / G;
    if ((lane % G) == 0 && word < num_words) {
      if (filter != nullptr) m &= filter[word];
      if (word == num_words - 1 && tail != 0) m &= ~0ull << (64 - tail);   // rows behind the block stay zero
      out[word] = m;
      count += __popcll(m);
    }
  }
}

// A workgroup takes a contiguous range of the run's tiles; a wave adds its matches to a block's counter when it moves on to
// another block (as bitmap_eval_runs_kernel, predicate_tree.hip).
__global__ __launch_bounds__(kBlock) void cmp_columns_runs_kernel(const long long *__restrict__ runs, long long extra, int lhs_type, int rhs_type,
                                                                 Compare cmp, unsigned long long *__restrict__ out_counts) {
  const int lane_of_wave = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long nb = runs[0];
  const long long num_tiles = runs[2];
  // (the 64-bit division runs on the vector unit: without the readfirstlane the tile number, and with it every row number,
  // address and branch below, stays a per-lane value)
  const int first = __builtin_amdgcn_readfirstlane(static_cast<int>(num_tiles * blockIdx.x / gridDim.x));
  const int end = __builtin_amdgcn_readfirstlane(static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x));
  unsigned long long count = 0;
  int counted_block = -1;
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    if (at.block != counted_block) {
      if (out_counts != nullptr && counted_block >= 0) {
        count = wave_reduce_add(count);
        if (lane_of_wave == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
      }
      count = 0;
      counted_block = at.block;
    }
    const int64_t n = run_rows(runs, at.block);
    const long long *mine = runs + extra + at.block;
    const Operand lhs{static_cast<uintptr_t>(runs[QSX_RUN_WORD(nb, kRunIn, at.block)]),
                      static_cast<uintptr_t>(runs[QSX_RUN_WORD(nb, kRunDictionary, at.block)]),
                      static_cast<unsigned long long>(mine[kLhsNumCodes * nb]), lhs_type};
    const Operand rhs{static_cast<uintptr_t>(mine[kRhsIn * nb]), static_cast<uintptr_t>(mine[kRhsDictionary * nb]),
                      static_cast<unsigned long long>(mine[kRhsNumCodes * nb]), rhs_type};
    int lw = run_code_width(runs, at.block), rw = static_cast<int>(mine[kRhsCodeWidth * nb]);
    if (lw == 0) lw = wide(lhs_type) ? 8 : 4;
    if (rw == 0) rw = wide(rhs_type) ? 8 : 4;
    const uint64_t *filter = run_filter(runs, at.block);
    uint64_t *out = run_out<uint64_t>(runs, at.block);
    const int64_t tile_row0 = static_cast<int64_t>(at.tile_in_block) * kTileRows;
    for (int batch = wave; batch < kTileBatches; batch += kWavesPerBlock) {
      const int64_t row_base = tile_row0 + static_cast<int64_t>(batch) * kBatchRows;
      if (row_base >= n) break;
      // (a fresh value to the compiler in every batch: otherwise it computes every form's lane offsets, 64 bits wide, in front of
      // the tile loop and keeps some sixty registers for them)
      int lane = lane_of_wave;
      asm volatile("" : "+v"(lane));
#define QSX_CMP_COLUMNS_FORM(LW, RW) \
  case LW * 16 + RW: load_pair<LW, RW>(lhs.stripe, rhs.stripe, n, row_base, lane, a, b); break;
      uint64_t a[kLaneRows] = {}, b[kLaneRows] = {};
      switch (lw * 16 + rw) {
        QSX_CMP_COLUMNS_FORM(1, 1) QSX_CMP_COLUMNS_FORM(1, 2) QSX_CMP_COLUMNS_FORM(1, 4) QSX_CMP_COLUMNS_FORM(1, 8)
        QSX_CMP_COLUMNS_FORM(2, 1) QSX_CMP_COLUMNS_FORM(2, 2) QSX_CMP_COLUMNS_FORM(2, 4) QSX_CMP_COLUMNS_FORM(2, 8)
        QSX_CMP_COLUMNS_FORM(4, 1) QSX_CMP_COLUMNS_FORM(4, 2) QSX_CMP_COLUMNS_FORM(4, 4) QSX_CMP_COLUMNS_FORM(4, 8)
        QSX_CMP_COLUMNS_FORM(8, 1) QSX_CMP_COLUMNS_FORM(8, 2) QSX_CMP_COLUMNS_FORM(8, 4) QSX_CMP_COLUMNS_FORM(8, 8)
        default: break;
      }
#undef QSX_CMP_COLUMNS_FORM
      if (lw <= 2 || rw <= 2) finish_batch<8>(lhs, rhs, cmp, n, row_base, a, b, filter, out, lane, count);
      else finish_batch<2>(lhs, rhs, cmp, n, row_base, a, b, filter, out, lane, count);
    }
  }
  if (out_counts != nullptr && counted_block >= 0) {
    count = wave_reduce_add(count);
    if (lane_of_wave == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
  }
}

static bool numeric(int type) { return type == QSX_INT || type == QSX_LONG || type == QSX_FLOAT || type == QSX_DOUBLE; }

// One operand's coding: widths 0 / 1 / 2 / 4, a dictionary only where there are codes, truncation on INT / LONG only, no
// negative code count where a dictionary is read.
static bool coding_ok(int type, int64_t nb, const int64_t *rows, const qsx_operand_coding_t *coding) {
  if (coding == nullptr || coding->block_code_width == nullptr) return coding == nullptr || coding->block_dictionaries == nullptr;
  for (int64_t b = 0; b < nb; ++b) {
    const int w = coding->block_code_width[b];
    const void *dictionary = coding->block_dictionaries != nullptr ? coding->block_dictionaries[b] : nullptr;
    if (w != 0 && w != 1 && w != 2 && w != 4) return false;
    if (w == 0 && dictionary != nullptr) return false;
    if (w != 0 && dictionary == nullptr && type != QSX_INT && type != QSX_LONG) return false;
    if (w != 0 && dictionary != nullptr && rows[b] > 0 && (coding->block_num_codes == nullptr || coding->block_num_codes[b] < 0)) return false;
  }
  return true;
}

}  // namespace cmp_columns
}  // namespace qsx

using namespace qsx;
using namespace qsx::cmp_columns;

extern "C" {

int qsx_select_cmp_columns_blocks(int lhs_type, int rhs_type, int64_t num_blocks, const int64_t *block_rows, const void *const *block_lhs,
                                  const qsx_operand_coding_t *lhs_coding, const void *const *block_rhs, const qsx_operand_coding_t *rhs_coding,
                                  int op, const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps, int64_t *out_counts_dev,
                                  qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  const bool dates = lhs_type == QSX_DATE && rhs_type == QSX_DATE;
  if (!dates && !(numeric(lhs_type) && numeric(rhs_type))) return QSX_ERR_UNSUPPORTED;   // CHAR, DATE against a non-DATE, unknown types
  if (num_blocks < 0 || op < QSX_EQ || op > QSX_GE ||
      (num_blocks > 0 && (block_rows == nullptr || block_lhs == nullptr || block_rhs == nullptr || block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (!run_blocks_ok(num_blocks, block_rows, block_lhs, reinterpret_cast<const void *const *>(block_out_bitmaps)) ||
      !run_blocks_ok(num_blocks, block_rows, block_rhs, nullptr)) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (!coding_ok(lhs_type, num_blocks, block_rows, lhs_coding) || !coding_ok(rhs_type, num_blocks, block_rows, rhs_coding)) return QSX_ERR_INVALID_ARGUMENT;
  if (num_blocks == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  const size_t nb = static_cast<size_t>(num_blocks);
  std::vector<int32_t> lhs_widths(nb, 0);
  if (lhs_coding != nullptr && lhs_coding->block_code_width != nullptr) lhs_widths.assign(lhs_coding->block_code_width, lhs_coding->block_code_width + nb);
  RunTable table;
  const long long tiles = table.build(kTileRows, num_blocks, block_rows, block_lhs, reinterpret_cast<const void *const *>(block_filters),
                                      reinterpret_cast<void *const *>(block_out_bitmaps), nullptr, lhs_widths.data(),
                                      lhs_coding != nullptr ? lhs_coding->block_dictionaries : nullptr);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  const long long extra = table.append(kExtraArrays * nb);
  for (size_t b = 0; b < nb; ++b) {
    long long *mine = table.words() + extra + b;
    mine[kRhsIn * nb] = RunTable::word_of(block_rhs[b]);
    if (rhs_coding != nullptr && rhs_coding->block_code_width != nullptr) {
      mine[kRhsCodeWidth * nb] = rhs_coding->block_code_width[b];
      if (rhs_coding->block_dictionaries != nullptr) mine[kRhsDictionary * nb] = RunTable::word_of(rhs_coding->block_dictionaries[b]);
      if (rhs_coding->block_num_codes != nullptr) mine[kRhsNumCodes * nb] = rhs_coding->block_num_codes[b];
    }
    if (lhs_coding != nullptr && lhs_coding->block_num_codes != nullptr) mine[kLhsNumCodes * nb] = lhs_coding->block_num_codes[b];
  }
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  // the usual arithmetic conversions of the pair (a DATE pair compares its ordered int64 keys)
  const bool any_double = lhs_type == QSX_DOUBLE || rhs_type == QSX_DOUBLE, any_float = lhs_type == QSX_FLOAT || rhs_type == QSX_FLOAT;
  const Compare cmp{any_double ? kClassDouble : any_float ? kClassFloat : kClassLong, op == QSX_LT || op == QSX_LE,
                    op == QSX_EQ || op == QSX_NE || op == QSX_LE || op == QSX_GE, op == QSX_GT || op == QSX_GE, op == QSX_NE};
  hipLaunchKernelGGL(cmp_columns_runs_kernel, dim3(tile_grid(tiles)), dim3(kBlock), 0, s, table.dev(), extra, lhs_type, rhs_type, cmp,
                     reinterpret_cast<unsigned long long *>(out_counts_dev));
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

}  // extern "C"
