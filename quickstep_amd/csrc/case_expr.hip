// case_expr.hip — searched CASE over WHEN bitmaps: qsx_eval_case / qsx_eval_case_blocks (include/qsx.h).
//
// The reference evaluates CASE WHEN p0 THEN e0 WHEN p1 THEN e1 .. ELSE e END per block as
// ScalarCaseExpression::getAllValues (expressions/scalar/ScalarCaseExpression.cpp:273-350): every WHEN predicate gives a
// TupleIdSequence over the rows no earlier WHEN took, every result expression is materialised over its own matches, and
// MultiplexNativeColumnVector (:420-470) scatters the pieces into one column.  Here the WHEN bitmaps come from the select
// kernels as they are (overlapping: the first set bit wins) and ONE pass multiplexes: the branch values share one
// expression program (qsx_expr_instr_t), evaluated for every row — no op traps, an unchosen branch's value is never
// stored — and the chosen operand is converted to the output type at the store (the resolver's Cast to the unified type,
// query_optimizer/resolver/Resolver.cpp:2819-2829).
//
// Shape: streaming, memory bound.  A lane owns kRowsPerLane = 4 consecutive rows, a wave 256 rows = four whole 64-row
// bitmap words: 16 bytes per lane of a 4-byte stripe, 2 x 16 bytes of an 8-byte one, the same for the output, non-temporal.
// No two waves touch one bitmap word, so the null bitmap is written with plain stores: the 4 bits of a lane are merged over
// its 16-lane group by a four-step butterfly and the group's first lane stores the word.  A tile that is not whole, or a
// stripe whose base is not 16-byte aligned, is read and written row by row under a bounds guard.
// NULLs: which columns a branch value depends on (through temps) is known on the host; the kernel gathers the row's
// "column is NULL" bits once and a row is NULL when its chosen branch is the NULL literal or depends on a NULL column.
#include "common.hpp"
#include "block_runs.hpp"

#include <cmath>
#include <type_traits>
#include <vector>

namespace qsx {
namespace case_expr {

constexpr int kBlock = 256;
constexpr int kRowsPerLane = 4;
constexpr int kWaveRows = kWave * kRowsPerLane;   // 256: four bitmap words
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kEagerWhens = 4;                    // WHEN bitmap words a lane asks for ahead of the program

// operand kinds on the device: the ABI's COLUMN / CONST / TEMP (a double temp) / NULL, and a temp of an integer instruction
constexpr int kOpdIntegerTemp = 4;

// Addresses of one stripe set (the single call, or one block of a run), as 64-bit words read with wave-uniform indices.
constexpr int kPtrOut = 0, kPtrOutNulls = 1, kPtrCols = 2, kPtrColNulls = kPtrCols + QSX_MAX_COLUMNS,
              kPtrWhens = kPtrColNulls + QSX_MAX_COLUMNS, kPtrWords = kPtrWhens + QSX_MAX_CASE_WHENS;

struct CaseOperand {
  int kind;
  int index;
};
struct CaseInstr {
  int op;       // QSX_EX_ADD .. QSX_EX_IDIV
  int dst;
  int narrow;   // integer instruction with two INT operands: the result wraps to 32 bits
  CaseOperand a, b;
};
struct CaseProgram {
  long long ptrs[kPtrWords];          // the single call's stripes (a run keeps one such set per block in its table)
  double consts[QSX_MAX_CONSTS];
  long long iconsts[QSX_MAX_CONSTS];  // the integral constants as int64 (0 for the others: never read)
  int types[QSX_MAX_COLUMNS];
  CaseInstr instrs[QSX_MAX_INSTRS];
  CaseOperand value[QSX_MAX_CASE_WHENS + 1];
  unsigned value_deps[QSX_MAX_CASE_WHENS + 1];   // bit c: the branch value depends on column c
  int num_columns, num_instrs, num_whens;
  int num_temps;   // (host side: which kernel to launch)
};
static_assert(sizeof(CaseProgram) % 4 == 0, "store_struct_kernel copies words");
static_assert(sizeof(CaseProgram) <= 4096, "travels as a kernel argument of store_struct_kernel");

// Run table: the header and first_tile[] of block_runs.hpp (run_locate, run_rows work on it), then one pointer set per block.
__device__ __forceinline__ const long long *run_ptrs(const long long *__restrict__ t, int b) {
  return t + kRunHeaderWords + (t[0] + 1) + t[0] + static_cast<long long>(b) * kPtrWords;
}

// The temps of a lane: NT of them (the kernel is compiled for programs whose temps all lie below kFewTemps and for the
// general case: eight temps of four rows are 64 VGPRs, and TPC-H's x * (1 - y) defines two).
constexpr int kFewTemps = 2;
template <int NT>
struct Temps {
  double t[NT][kRowsPerLane];   // 8-byte slots: a double, or the int64 bits of an integer temp
};
// (wave-uniform index -> scalar branches; the distinct asm comment per case keeps the cases from being merged into one
// dynamically indexed access, which would move the temps from VGPRs to scratch: agg_hash_update.hpp temps_get)
template <int NT>
__device__ __forceinline__ void temps_get(const Temps<NT> &s, int i, double (&out)[kRowsPerLane]) {
#define QSX_CASE_TG(k) \
  case k:              \
    if constexpr (k < NT) { _Pragma("unroll") for (int v = 0; v < kRowsPerLane; ++v) { out[v] = s.t[k][v]; asm("; case temp get " #k : "+v"(out[v])); } } \
    break;
  switch (i) {
    QSX_CASE_TG(0) QSX_CASE_TG(1) QSX_CASE_TG(2) QSX_CASE_TG(3) QSX_CASE_TG(4) QSX_CASE_TG(5) QSX_CASE_TG(6)
    default:
      if constexpr (NT > 7) {
#pragma unroll
        for (int v = 0; v < kRowsPerLane; ++v) { out[v] = s.t[7][v]; asm("; case temp get 7" : "+v"(out[v])); }
      }
      break;
  }
#undef QSX_CASE_TG
}
template <int NT>
__device__ __forceinline__ void temps_set(Temps<NT> &s, int i, const double (&in)[kRowsPerLane]) {
#define QSX_CASE_TS(k) \
  case k:              \
    if constexpr (k < NT) { _Pragma("unroll") for (int v = 0; v < kRowsPerLane; ++v) { s.t[k][v] = in[v]; asm("; case temp set " #k : "+v"(s.t[k][v])); } } \
    break;
  switch (i) {
    QSX_CASE_TS(0) QSX_CASE_TS(1) QSX_CASE_TS(2) QSX_CASE_TS(3) QSX_CASE_TS(4) QSX_CASE_TS(5) QSX_CASE_TS(6)
    default:
      if constexpr (NT > 7) {
#pragma unroll
        for (int v = 0; v < kRowsPerLane; ++v) { s.t[7][v] = in[v]; asm("; case temp set 7" : "+v"(s.t[7][v])); }
      }
      break;
  }
#undef QSX_CASE_TS
}

// What a wave works on: rows [row0, row0 + 256) of a stripe set of n rows; the lane's rows are row0 + 4 * lane + 0..3.
struct Tile {
  const long long *ptrs;   // wave-uniform
  int64_t n;
  int64_t row0;
  bool whole;              // all 256 rows exist
};

// The lane's four rows of a stripe of T.
template <typename T>
__device__ __forceinline__ void load_rows(const void *col, const Tile &tile, int lane, T (&v)[kRowsPerLane]) {
  const int64_t first = tile.row0 + static_cast<int64_t>(lane) * kRowsPerLane;
  const T *p = static_cast<const T *>(col) + first;
  if (tile.whole && (reinterpret_cast<uintptr_t>(col) & 15) == 0) {   // wave-uniform
    constexpr int kPer16 = 16 / sizeof(T);
#pragma unroll
    for (int q = 0; q < kRowsPerLane / kPer16; ++q) {
      const uint4 raw = stream_load16(p + q * kPer16);
      __builtin_memcpy(&v[q * kPer16], &raw, 16);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) v[j] = first + j < tile.n ? load_global_nt(p + j) : T(0);
}
template <typename T>
__device__ __forceinline__ void store_rows(void *out, const Tile &tile, int lane, const T (&v)[kRowsPerLane]) {
  const int64_t first = tile.row0 + static_cast<int64_t>(lane) * kRowsPerLane;
  T *p = static_cast<T *>(out) + first;
  if (tile.whole && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr int kPer16 = 16 / sizeof(T);
#pragma unroll
    for (int q = 0; q < kRowsPerLane / kPer16; ++q) {
      u32x4 raw;
      __builtin_memcpy(&raw, &v[q * kPer16], 16);
      __builtin_nontemporal_store(raw, (__attribute__((address_space(1))) u32x4 *)reinterpret_cast<uintptr_t>(p + q * kPer16));
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    if (first + j < tile.n) store_global_nt(v[j], p + j);
  }
}

// The lane's four bits of an MSB-first bitmap (bit 3 = its first row), 0 where the bitmap is absent or the word lies past n.
__device__ __forceinline__ unsigned load_nibble(const uint64_t *bitmap, const Tile &tile, int lane) {
  if (bitmap == nullptr) return 0u;
  const int64_t word_row = tile.row0 + (lane >> 4) * 64;
  if (word_row >= tile.n) return 0u;
  const uint64_t word = load_global(&bitmap[word_row >> 6]);
  return static_cast<unsigned>(word >> (60 - 4 * (lane & 15))) & 0xFu;
}
// The reverse: every 16-lane group's nibbles as the word of its 64 rows, stored by the group's first lane.
__device__ __forceinline__ void store_nibbles(uint64_t *bitmap, const Tile &tile, int lane, unsigned nibble) {
  unsigned long long m = nibble;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {   // after step d the first lane of every 2d-group holds 2d * 4 bits
    const unsigned long long other = __shfl_xor(m, d, kWave);
    m = (m << (4 * d)) | other;
  }
  const int64_t word_row = tile.row0 + (lane >> 4) * 64;
  if ((lane & 15) == 0 && word_row < tile.n) store_global(static_cast<uint64_t>(m), &bitmap[word_row >> 6]);
}

template <typename T>
__device__ __forceinline__ const T *ptr_word(const long long *ptrs, int i) {
  return as_global(reinterpret_cast<const T *>(ptrs[i]));
}

// An operand as doubles (AsInt = false: what a double instruction or a DOUBLE result reads) or as int64 (AsInt = true).
template <bool AsInt, int NT>
__device__ __forceinline__ void operand_rows(const CaseProgram &p, const CaseOperand &o, const Temps<NT> &temps, const Tile &tile, int lane,
                                             double (&out)[kRowsPerLane]) {
  typedef typename std::conditional<AsInt, long long, double>::type V;
  auto put = [&](int j, V value) {
    if constexpr (AsInt) out[j] = __longlong_as_double(value); else out[j] = value;
  };
  switch (o.kind) {
    case QSX_OPD_COLUMN: {
      const void *col = ptr_word<char>(tile.ptrs, kPtrCols + o.index);
      switch (p.types[o.index]) {
        case QSX_INT: {
          int32_t v[kRowsPerLane];
          load_rows<int32_t>(col, tile, lane, v);
#pragma unroll
          for (int j = 0; j < kRowsPerLane; ++j) put(j, static_cast<V>(v[j]));
          break;
        }
        case QSX_LONG: {
          long long v[kRowsPerLane];
          load_rows<long long>(col, tile, lane, v);
#pragma unroll
          for (int j = 0; j < kRowsPerLane; ++j) put(j, static_cast<V>(v[j]));
          break;
        }
        case QSX_FLOAT: {   // (never under AsInt: the host refuses it)
          float v[kRowsPerLane];
          load_rows<float>(col, tile, lane, v);
#pragma unroll
          for (int j = 0; j < kRowsPerLane; ++j) put(j, static_cast<V>(v[j]));
          break;
        }
        default: {
          double v[kRowsPerLane];
          load_rows<double>(col, tile, lane, v);
#pragma unroll
          for (int j = 0; j < kRowsPerLane; ++j) put(j, static_cast<V>(v[j]));
          break;
        }
      }
      break;
    }
    case QSX_OPD_CONST:
#pragma unroll
      for (int j = 0; j < kRowsPerLane; ++j) {
        if constexpr (AsInt) put(j, p.iconsts[o.index]); else put(j, p.consts[o.index]);
      }
      break;
    case kOpdIntegerTemp:
      temps_get(temps, o.index, out);
      if constexpr (!AsInt) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) out[j] = static_cast<double>(__double_as_longlong(out[j]));
      }
      break;
    case QSX_OPD_TEMP:   // a double temp (never under AsInt)
      temps_get(temps, o.index, out);
      break;
    default:             // QSX_OPD_NULL: the row is NULL and stores 0
#pragma unroll
      for (int j = 0; j < kRowsPerLane; ++j) out[j] = 0.0;   // (all-zero bits: 0 as an int64 too)
      break;
  }
}

// One integer node in 64 bits (agg_hash_update.hpp int_node: x / 0 = 0, x / -1 = 0 - x, everything wraps).
__device__ __forceinline__ long long integer_node(int op, long long a, long long b) {
  const unsigned long long ua = static_cast<unsigned long long>(a), ub = static_cast<unsigned long long>(b);
  switch (op) {
    case QSX_EX_IADD: return static_cast<long long>(ua + ub);
    case QSX_EX_ISUB: return static_cast<long long>(ua - ub);
    case QSX_EX_IMUL: return static_cast<long long>(ua * ub);
    default: return b == 0 ? 0 : (b == -1 ? static_cast<long long>(0ull - ua) : a / b);
  }
}

template <int OUT, int NT>
__device__ __forceinline__ void case_tile(const CaseProgram &p, const Tile &tile, int lane) {
  // The lane's word of the first kEagerWhens WHEN bitmaps, asked for before anything else and looked at only behind the
  // program: the loads are independent of each other and of the column loads, so they cost no round trip of their own; later
  // WHENs are read when their turn comes (eight words held across the program cost the INT kernels a wave per SIMD).  (A slot
  // past num_whens repeats WHEN 0 and a word past n reads word 0 — both exist — and neither is looked at.)
  const int64_t word_row = tile.row0 + (lane >> 4) * 64;
  const bool word_in_range = word_row < tile.n;
  const int64_t word_index = word_in_range ? word_row >> 6 : 0;
  uint64_t when_word[kEagerWhens];
#pragma unroll
  for (int k = 0; k < kEagerWhens; ++k) {
    when_word[k] = load_global(&ptr_word<uint64_t>(tile.ptrs, kPtrWhens + (k < p.num_whens ? k : 0))[word_index]);
  }
  // bit c of null_cols[j]: column c is NULL at row j
  unsigned null_cols[kRowsPerLane] = {};
  for (int c = 0; c < p.num_columns; ++c) {
    const uint64_t *nulls = ptr_word<uint64_t>(tile.ptrs, kPtrColNulls + c);
    if (nulls == nullptr) continue;   // wave-uniform
    const unsigned nib = load_nibble(nulls, tile, lane);
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) null_cols[j] |= ((nib >> (3 - j)) & 1u) << c;
  }
  // the shared program, every node rounded on its own (-ffp-contract=off)
  Temps<NT> temps;
  for (int k = 0; k < p.num_instrs; ++k) {
    const CaseInstr in = p.instrs[k];
    double a[kRowsPerLane], b[kRowsPerLane], r[kRowsPerLane];
    if (in.op >= QSX_EX_IADD) {
      operand_rows<true, NT>(p, in.a, temps, tile, lane, a);
      operand_rows<true, NT>(p, in.b, temps, tile, lane, b);
#pragma unroll
      for (int j = 0; j < kRowsPerLane; ++j) {
        long long v = integer_node(in.op, __double_as_longlong(a[j]), __double_as_longlong(b[j]));
        if (in.narrow) v = static_cast<long long>(static_cast<int32_t>(v));
        r[j] = __longlong_as_double(v);
      }
    } else {
      operand_rows<false, NT>(p, in.a, temps, tile, lane, a);
      operand_rows<false, NT>(p, in.b, temps, tile, lane, b);
#pragma unroll
      for (int j = 0; j < kRowsPerLane; ++j) {
        switch (in.op) {
          case QSX_EX_ADD: r[j] = a[j] + b[j]; break;
          case QSX_EX_SUB: r[j] = a[j] - b[j]; break;
          case QSX_EX_MUL: r[j] = a[j] * b[j]; break;
          default: r[j] = a[j] / b[j]; break;
        }
      }
    }
    temps_set(temps, in.dst, r);
  }
  int chosen[kRowsPerLane];
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) chosen[j] = p.num_whens;
  unsigned open = word_in_range ? 0xFu : 0u;
#pragma unroll
  for (int k = 0; k < kEagerWhens; ++k) {
    if (k >= p.num_whens) break;   // wave-uniform
    const unsigned take = static_cast<unsigned>(when_word[k] >> (60 - 4 * (lane & 15))) & open;
    open &= ~take;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      if ((take >> (3 - j)) & 1u) chosen[j] = k;
    }
  }
  for (int k = kEagerWhens; k < p.num_whens; ++k) {
    const unsigned take = load_nibble(ptr_word<uint64_t>(tile.ptrs, kPtrWhens + k), tile, lane) & open;
    open &= ~take;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      if ((take >> (3 - j)) & 1u) chosen[j] = k;
    }
  }
  // multiplex: the chosen branch's operand, converted to the output type
  double result[kRowsPerLane] = {};   // 8-byte slots again
  unsigned null_nibble = 0;
  for (int k = 0; k <= p.num_whens; ++k) {
    bool mine = false;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) mine |= chosen[j] == k;
    if (__ballot(mine) == 0ull) continue;   // no row of the wave took this branch: its stripes are not read
    const CaseOperand o = p.value[k];
    const unsigned deps = o.kind == QSX_OPD_NULL ? ~0u : p.value_deps[k];
    double v[kRowsPerLane];
    operand_rows<OUT != QSX_DOUBLE, NT>(p, o, temps, tile, lane, v);
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      if (chosen[j] != k) continue;
      const bool is_null = o.kind == QSX_OPD_NULL || (deps & null_cols[j]) != 0;
      result[j] = is_null ? 0.0 : v[j];
      if (is_null && tile.row0 + static_cast<int64_t>(lane) * kRowsPerLane + j < tile.n) null_nibble |= 1u << (3 - j);
    }
  }
  void *out = as_global(reinterpret_cast<char *>(tile.ptrs[kPtrOut]));
  if constexpr (OUT == QSX_INT) {
    int32_t narrow[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) narrow[j] = static_cast<int32_t>(__double_as_longlong(result[j]));
    store_rows<int32_t>(out, tile, lane, narrow);
  } else {
    store_rows<double>(out, tile, lane, result);   // (a LONG: its bits)
  }
  uint64_t *out_nulls = as_global(reinterpret_cast<uint64_t *>(tile.ptrs[kPtrOutNulls]));
  if (out_nulls != nullptr) store_nibbles(out_nulls, tile, lane, null_nibble);
}

template <int OUT, bool kRuns, int NT>
__global__ __launch_bounds__(kBlock) void case_kernel(const CaseProgram *__restrict__ program, const long long *__restrict__ runs, int64_t n) {
  const CaseProgram &p = *program;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int64_t num_tiles = kRuns ? runs[2] : (n + kWaveRows - 1) / kWaveRows;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; t < num_tiles; t += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
    Tile tile;
    if constexpr (kRuns) {
      const RunTile at = run_locate(runs, static_cast<int>(t));
      tile.ptrs = run_ptrs(runs, at.block);
      tile.n = run_rows(runs, at.block);
      tile.row0 = static_cast<int64_t>(at.tile_in_block) * kWaveRows;
    } else {
      tile.ptrs = p.ptrs;
      tile.n = n;
      tile.row0 = t * kWaveRows;
    }
    tile.whole = tile.row0 + kWaveRows <= tile.n;
    case_tile<OUT, NT>(p, tile, lane);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------

constexpr int kTypeNone = -1;

// The program and the branch values checked and typed (include/qsx.h "qsx_eval_case"); QSX_OK or the refusal.
static int translate(int num_columns, const int32_t *types, int num_instrs, const qsx_expr_instr_t *instrs, const double *consts,
                     const qsx_case_desc_t *desc, CaseProgram *prog, bool *has_null_branch) {
  if (num_columns < 0 || num_columns > QSX_MAX_COLUMNS || num_instrs < 0 || num_instrs > QSX_MAX_INSTRS || desc == nullptr ||
      (num_columns > 0 && types == nullptr) || (num_instrs > 0 && instrs == nullptr)) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (desc->num_whens < 1 || desc->num_whens > QSX_MAX_CASE_WHENS) return QSX_ERR_INVALID_ARGUMENT;
  if (desc->out_type != QSX_INT && desc->out_type != QSX_LONG && desc->out_type != QSX_DOUBLE) return QSX_ERR_INVALID_ARGUMENT;
  CaseProgram &p = *prog;
  p.num_columns = num_columns;
  p.num_instrs = num_instrs;
  p.num_whens = desc->num_whens;
  for (int c = 0; c < num_columns; ++c) {
    if (types[c] != QSX_INT && types[c] != QSX_LONG && types[c] != QSX_FLOAT && types[c] != QSX_DOUBLE) return QSX_ERR_UNSUPPORTED;
    p.types[c] = types[c];
  }
  int const_type[QSX_MAX_CONSTS];
  for (int k = 0; k < QSX_MAX_CONSTS; ++k) {
    const double c = consts != nullptr ? consts[k] : 0.0;
    p.consts[k] = c;
    const bool integral = std::isfinite(c) && c == std::trunc(c) && std::fabs(c) <= 9007199254740992.0;
    p.iconsts[k] = integral ? static_cast<long long>(c) : 0;
    const_type[k] = !integral ? QSX_DOUBLE : (c >= -2147483648.0 && c <= 2147483647.0 ? QSX_INT : QSX_LONG);
  }
  int temp_type[QSX_MAX_TEMPS];
  unsigned temp_deps[QSX_MAX_TEMPS] = {};
  for (int t = 0; t < QSX_MAX_TEMPS; ++t) temp_type[t] = kTypeNone;
  // type of an operand, kTypeNone when it is not a legal one
  auto operand_type = [&](const qsx_operand_t &o) {
    switch (o.kind) {
      case QSX_OPD_COLUMN: return o.index >= 0 && o.index < num_columns ? static_cast<int>(types[o.index]) : kTypeNone;
      case QSX_OPD_CONST: return o.index >= 0 && o.index < QSX_MAX_CONSTS && consts != nullptr ? const_type[o.index] : kTypeNone;
      case QSX_OPD_TEMP: return o.index >= 0 && o.index < QSX_MAX_TEMPS ? temp_type[o.index] : kTypeNone;
      default: return kTypeNone;   // QSX_OPD_NULL is a branch value only
    }
  };
  auto operand_deps = [&](const qsx_operand_t &o) {
    return o.kind == QSX_OPD_COLUMN ? 1u << o.index : (o.kind == QSX_OPD_TEMP ? temp_deps[o.index] : 0u);
  };
  auto device_operand = [&](const qsx_operand_t &o, int type) {
    return CaseOperand{o.kind == QSX_OPD_TEMP && type != QSX_DOUBLE ? kOpdIntegerTemp : o.kind, o.index};
  };
  auto is_integer = [](int type) { return type == QSX_INT || type == QSX_LONG; };
  for (int k = 0; k < num_instrs; ++k) {
    const qsx_expr_instr_t &in = instrs[k];
    if (in.op < QSX_EX_ADD || in.op > QSX_EX_IDIV || in.dst < 0 || in.dst >= QSX_MAX_TEMPS) return QSX_ERR_INVALID_ARGUMENT;
    const int ta = operand_type(in.a), tb = operand_type(in.b);
    if (ta == kTypeNone || tb == kTypeNone) return QSX_ERR_INVALID_ARGUMENT;
    CaseInstr &d = p.instrs[k];
    d.op = in.op;
    d.dst = in.dst;
    d.a = device_operand(in.a, ta);
    d.b = device_operand(in.b, tb);
    const unsigned deps = operand_deps(in.a) | operand_deps(in.b);
    if (in.op >= QSX_EX_IADD) {
      if (!is_integer(ta) || !is_integer(tb)) return QSX_ERR_INVALID_ARGUMENT;   // no implicit double -> integer conversion
      d.narrow = ta == QSX_INT && tb == QSX_INT ? 1 : 0;
      temp_type[in.dst] = d.narrow ? QSX_INT : QSX_LONG;
    } else {
      d.narrow = 0;
      temp_type[in.dst] = QSX_DOUBLE;
    }
    temp_deps[in.dst] = deps;
    if (in.dst + 1 > p.num_temps) p.num_temps = in.dst + 1;
  }
  *has_null_branch = false;
  for (int k = 0; k <= desc->num_whens; ++k) {
    const qsx_operand_t &o = desc->value[k];
    if (o.kind == QSX_OPD_NULL) {
      *has_null_branch = true;
      p.value[k] = CaseOperand{QSX_OPD_NULL, 0};
      p.value_deps[k] = 0;
      continue;
    }
    const int type = operand_type(o);
    if (type == kTypeNone) return QSX_ERR_INVALID_ARGUMENT;
    if (desc->out_type != QSX_DOUBLE && !is_integer(type)) return QSX_ERR_INVALID_ARGUMENT;    // the Cast never narrows a double
    if (desc->out_type == QSX_INT && type == QSX_LONG) return QSX_ERR_INVALID_ARGUMENT;        // nor a LONG
    p.value[k] = device_operand(o, type);
    p.value_deps[k] = operand_deps(o);
  }
  return QSX_OK;
}

template <bool kRuns, int NT>
static void launch_sized(int out_type, int grid, hipStream_t s, const CaseProgram *slot, const long long *runs, int64_t n) {
  switch (out_type) {
    case QSX_INT: hipLaunchKernelGGL((case_kernel<QSX_INT, kRuns, NT>), dim3(grid), dim3(kBlock), 0, s, slot, runs, n); break;
    case QSX_LONG: hipLaunchKernelGGL((case_kernel<QSX_LONG, kRuns, NT>), dim3(grid), dim3(kBlock), 0, s, slot, runs, n); break;
    default: hipLaunchKernelGGL((case_kernel<QSX_DOUBLE, kRuns, NT>), dim3(grid), dim3(kBlock), 0, s, slot, runs, n); break;
  }
}
// num_temps: one more than the highest temp the program writes (its reads were checked against its writes)
template <bool kRuns>
static void launch(int out_type, int num_temps, int grid, hipStream_t s, const CaseProgram *slot, const long long *runs, int64_t n) {
  if (num_temps <= kFewTemps) launch_sized<kRuns, kFewTemps>(out_type, grid, s, slot, runs, n);
  else launch_sized<kRuns, QSX_MAX_TEMPS>(out_type, grid, s, slot, runs, n);
}

static long long word_of(const void *p) { return static_cast<long long>(reinterpret_cast<uintptr_t>(p)); }

}  // namespace case_expr
}  // namespace qsx

using namespace qsx;
using namespace qsx::case_expr;

extern "C" {

size_t qsx_abi_sizeof_case_desc(void) { return sizeof(qsx_case_desc_t); }

int qsx_eval_case(int num_columns, const void *const *cols, const int32_t *types, const uint64_t *const *col_null_bitmaps, int num_instrs,
                  const qsx_expr_instr_t *instrs, const double *consts, const qsx_case_desc_t *desc, const uint64_t *const *when_bitmaps_dev,
                  int64_t n, void *out_dev, uint64_t *out_null_bitmap_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  CaseProgram prog{};
  bool has_null_branch = false;
  const int rc = translate(num_columns, types, num_instrs, instrs, consts, desc, &prog, &has_null_branch);
  if (rc != QSX_OK) return rc;
  if (n < 0 || (num_columns > 0 && cols == nullptr) || when_bitmaps_dev == nullptr || (n > 0 && out_dev == nullptr)) return QSX_ERR_INVALID_ARGUMENT;
  if (out_null_bitmap_dev == nullptr && (has_null_branch || col_null_bitmaps != nullptr)) return QSX_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < num_columns; ++c) {
    if (n > 0 && cols[c] == nullptr) return QSX_ERR_INVALID_ARGUMENT;
    prog.ptrs[kPtrCols + c] = word_of(cols[c]);
    prog.ptrs[kPtrColNulls + c] = col_null_bitmaps != nullptr ? word_of(col_null_bitmaps[c]) : 0;
  }
  for (int k = 0; k < desc->num_whens; ++k) {
    if (n > 0 && when_bitmaps_dev[k] == nullptr) return QSX_ERR_INVALID_ARGUMENT;
    prog.ptrs[kPtrWhens + k] = word_of(when_bitmaps_dev[k]);
  }
  prog.ptrs[kPtrOut] = word_of(out_dev);
  prog.ptrs[kPtrOutNulls] = word_of(out_null_bitmap_dev);
  if (n == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  // the program travels through a device slot, not the kernarg segment (DESIGN.md "Kernel arguments")
  CaseProgram *slot = device_slot<CaseProgram>(s);
  if (slot == nullptr) return QSX_ERR_OUT_OF_MEMORY;
  hipLaunchKernelGGL(store_struct_kernel<CaseProgram>, dim3(1), dim3(64), 0, s, prog, slot);
  QSX_CHECK_LAUNCH();
  launch<false>(desc->out_type, prog.num_temps, grid_for((n + kWaveRows - 1) / kWaveRows, kWavesPerBlock), s, slot, nullptr, n);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_eval_case_blocks(int num_columns, const int32_t *types, int num_instrs, const qsx_expr_instr_t *instrs, const double *consts,
                         const qsx_case_desc_t *desc, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols,
                         const uint64_t *const *block_col_null_bitmaps, const uint64_t *const *block_when_bitmaps, void *const *block_out,
                         uint64_t *const *block_out_null_bitmaps, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  CaseProgram prog{};
  bool has_null_branch = false;
  const int rc = translate(num_columns, types, num_instrs, instrs, consts, desc, &prog, &has_null_branch);
  if (rc != QSX_OK) return rc;
  if (num_blocks < 0 || (num_blocks > 0 && (block_rows == nullptr || block_when_bitmaps == nullptr || block_out == nullptr ||
                                            (num_columns > 0 && block_cols == nullptr)))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (block_out_null_bitmaps == nullptr && (has_null_branch || block_col_null_bitmaps != nullptr)) return QSX_ERR_INVALID_ARGUMENT;
  if (num_blocks == 0) return QSX_OK;
  if (!run_blocks_ok(num_blocks, block_rows, nullptr, block_out)) return QSX_ERR_INVALID_ARGUMENT;
  if (block_out_null_bitmaps != nullptr && !run_blocks_ok(num_blocks, block_rows, nullptr, reinterpret_cast<const void *const *>(block_out_null_bitmaps))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  // the run's table: the tile index of run_table.hpp (run_locate, run_rows work on it), then one pointer set per block
  const int whens = desc->num_whens;
  RunTable table;
  const long long tiles = table.index(kWaveRows, num_blocks, block_rows, kPtrWords);
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < num_blocks; ++b) {
    const int64_t r = block_rows[b];
    long long *set = table.at(kRunIn) + b * kPtrWords;
    set[kPtrOut] = word_of(block_out[b]);
    set[kPtrOutNulls] = block_out_null_bitmaps != nullptr ? word_of(block_out_null_bitmaps[b]) : 0;
    for (int c = 0; c < num_columns; ++c) {
      const void *col = block_cols[b * num_columns + c];
      if (r > 0 && col == nullptr) return QSX_ERR_INVALID_ARGUMENT;
      set[kPtrCols + c] = word_of(col);
      set[kPtrColNulls + c] = block_col_null_bitmaps != nullptr ? word_of(block_col_null_bitmaps[b * num_columns + c]) : 0;
    }
    for (int k = 0; k < whens; ++k) {
      const uint64_t *bitmap = block_when_bitmaps[b * whens + k];
      if (r > 0 && bitmap == nullptr) return QSX_ERR_INVALID_ARGUMENT;
      set[kPtrWhens + k] = word_of(bitmap);
    }
  }
  if (tiles == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  const int up = table.upload(s);
  if (up != QSX_OK) return up;
  const long long *runs_dev = table.dev();
  CaseProgram *slot = device_slot<CaseProgram>(s);
  if (slot == nullptr) return QSX_ERR_OUT_OF_MEMORY;
  hipLaunchKernelGGL(store_struct_kernel<CaseProgram>, dim3(1), dim3(64), 0, s, prog, slot);
  QSX_CHECK_LAUNCH();
  launch<true>(desc->out_type, prog.num_temps, grid_for(tiles, kWavesPerBlock), s, slot, runs_dev, 0);
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

}  // extern "C"
