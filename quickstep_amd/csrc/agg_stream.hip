// agg_stream.hip — Q1-shape aggregation for a handful of groups: rows stream from HBM through registers (agg_stream.hpp).
//
// A persistent grid walks tiles of 2 * BLOCK * U rows.  Within a step of a tile lane l of a wave owns the two consecutive rows
// base + 2 l and base + 2 l + 1: a DOUBLE column is one 16-byte load per lane (1 KiB per wave instruction), a CHAR(1) key
// column one 2-byte load.  The loads of the next tile are issued before the arithmetic of
// the current one, in straight-line code (two register sets, the loop body written twice), so the waits in front of the
// arithmetic are counted ones that leave the next tile's loads in flight.
//
// Every lane keeps the accumulators of kStreamGroups groups in registers; the key codes of those groups are wave-uniform (a
// wave adopts the first distinct codes it meets).  A row of any further group goes to a small workgroup-private LDS table and,
// when that is full, to the state's global table.  At the end the waves fold their registers into the same LDS table, and the
// workgroup sends one global atomic per group and accumulator.
#include "agg_stream.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace qsx {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ V stream_load_nt(const char *p) {
  return __builtin_nontemporal_load((const __attribute__((address_space(1))) V *)reinterpret_cast<uintptr_t>(p));
}

constexpr bool stream_value_column(const DevConfig &d, unsigned used, int col) {
  if (col >= d.num_columns || ((used >> col) & 1u) == 0) return false;
  for (int k = 0; k < d.num_keys; ++k) {
    if (d.key_column[k] == col) return false;
  }
  return true;
}

// The rows of one tile a lane owns, as the loads delivered them (nothing here is computed: a use would wait for the load).
template <int U>
struct StreamRows {
  f64x2 v[QSX_MAX_COLUMNS][U];   // DOUBLE columns: the two rows
  uint16_t k[QSX_MAX_KEYS][U];   // CHAR(1) keys: the two rows' bytes
};

template <int NS, typename Code>
struct StreamState {
  double acc[kStreamGroups][NS];
  unsigned int cnt[kStreamGroups];
  Code key[kStreamGroups];   // wave-uniform; slots below `held` are taken
  int held;
};

// kFull: every row of the tile exists (no comparison against n anywhere near a load).
template <int U, int BLOCK, bool kFull>
__device__ __forceinline__ void stream_load(const DevConfig &c, unsigned used, const StreamColumns &cols, int64_t n, int64_t tile,
                                            StreamRows<U> &r) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t row = (tile * U + u) * (2 * BLOCK) + 2 * static_cast<int64_t>(threadIdx.x);
#pragma unroll
    for (int k = 0; k < QSX_MAX_KEYS; ++k) {
      if (k < c.num_keys) {
        const char *p = static_cast<const char *>(cols.p[c.key_column[k]]) + row;
        uint16_t x = 0;
        if (kFull || row + 1 < n) {
          x = stream_load_nt<uint16_t>(p);
        } else if (row < n) {
          x = stream_load_nt<uint8_t>(p);
        }
        r.k[k][u] = x;
      }
    }
#pragma unroll
    for (int col = 0; col < QSX_MAX_COLUMNS; ++col) {
      if (stream_value_column(c, used, col)) {
        const char *p = static_cast<const char *>(cols.p[col]) + row * 8;
        f64x2 x = {0.0, 0.0};
        if (kFull || row + 1 < n) {
          x = stream_load_nt<f64x2>(p);
        } else if (row < n) {
          x.x = stream_load_nt<double>(p);
        }
        r.v[col][u] = x;
      }
    }
  }
}

__device__ __forceinline__ uint32_t stream_read_lane(uint32_t v, int lane) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lane));
}
__device__ __forceinline__ unsigned long long stream_bits(double v) { return static_cast<unsigned long long>(__double_as_longlong(v)); }

// `rows` rows of group `code` with these sums: into the workgroup's LDS table, or the global table when the group finds no slot.
template <int NS>
__device__ __forceinline__ void stream_table_add(unsigned long long *l_keys, unsigned long long *l_acc, const HashTableView &g,
                                                 unsigned long long code, unsigned long long rows, const double (&sum)[NS]) {
  const int s = lds_find_or_insert(l_keys, kStreamSlots, code);   // (a 32-bit code is never the table's empty marker)
  if (s >= 0) {
    lds_add(&l_acc[s], rows, kAccSumI64);
#pragma unroll
    for (int j = 0; j < NS; ++j) lds_add(&l_acc[(j + 1) * kStreamSlots + s], stream_bits(sum[j]), kAccSumF64);
    return;
  }
  const unsigned long long gs = global_find_or_insert(g, code);
  if (gs != ~0ull) {
    global_add(g, 0, gs, rows, kAccSumI64);
#pragma unroll
    for (int j = 0; j < NS; ++j) global_add(g, j + 1, gs, stream_bits(sum[j]), kAccSumF64);
  }
  // vmcnt(0): with atomics pending next to the row loads the compiler would wait for ALL of them at every later use of a
  // loaded row; behind this wait only loads are pending where this rare branch joins the stream again
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// Rows of held slot e under mask m: a select of the addend — x or +0.0, never a product, so that a NaN or Inf of one group
// cannot reach another.  (The same adds under the execution mask measured the same: DESIGN.md §4.)
template <int NS, typename Code>
__device__ __forceinline__ void stream_accumulate(StreamState<NS, Code> &st, int e, bool m, const double (&val)[NS]) {
#pragma unroll
  for (int j = 0; j < NS; ++j) st.acc[e][j] += m ? val[j] : 0.0;
  st.cnt[e] += m ? 1u : 0u;
}

template <int U, int BLOCK, bool kFull, int NS, typename Code>
__device__ __forceinline__ void stream_compute(const DevConfig &c, int64_t n, int64_t tile, const StreamRows<U> &r,
                                               StreamState<NS, Code> &st, unsigned long long *l_keys, unsigned long long *l_acc,
                                               const HashTableView &g) {
  // (no unroll pragma while U = 1: there is no loop left to unroll then, and the compiler warns about the request.  A larger U
  // needs it back, or the row registers indexed by u go to scratch.)
  static_assert(U == 1, "put #pragma unroll back on the step loop");
  for (int u = 0; u < U; ++u) {
    const int64_t row = (tile * U + u) * (2 * BLOCK) + 2 * static_cast<int64_t>(threadIdx.x);
    Code code[2];
    bool live[2], unmatched[2];
    double val[2][NS];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      live[i] = kFull || row + i < n;
      code[i] = 0;
#pragma unroll
      for (int k = 0; k < QSX_MAX_KEYS; ++k) {
        if (k < c.num_keys) {
          code[i] |= ((static_cast<uint32_t>(r.k[k][u]) >> (8 * i)) & 0xFFu) << c.key_shift[k];
        }
      }
      // the expression program, every node rounded on its own
      double temps[QSX_MAX_TEMPS] = {};
      auto operand = [&](const DevOperand &o) __attribute__((always_inline)) {
        return o.kind == QSX_OPD_CONST ? c.consts[o.index] : (o.kind == QSX_OPD_TEMP ? temps[o.index] : r.v[o.index][u][i]);
      };
#pragma unroll
      for (int t = 0; t < QSX_MAX_INSTRS; ++t) {
        if (t < c.num_instrs) {
          const double a = operand(c.instrs[t].a), b = operand(c.instrs[t].b);
          const int op = c.instrs[t].op;
          temps[c.instrs[t].dst] = op == QSX_EX_ADD ? a + b : (op == QSX_EX_SUB ? a - b : (op == QSX_EX_MUL ? a * b : a / b));
        }
      }
#pragma unroll
      for (int j = 0; j < NS; ++j) val[i][j] = operand(c.sums[j].arg);
      bool any = false;
#pragma unroll
      for (int e = 0; e < kStreamGroups; ++e) {
        const bool m = live[i] && e < st.held && code[i] == st.key[e];
        stream_accumulate(st, e, m, val[i]);
        any = any || m;
      }
      unmatched[i] = live[i] && !any;
    }
    // live rows of a group the wave does not hold: adopt the group while a slot is free, else the tables
    while (true) {
      const unsigned long long waiting = __ballot(unmatched[0] || unmatched[1]);
      if (waiting == 0) break;
      if (st.held == kStreamGroups) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (unmatched[i]) stream_table_add<NS>(l_keys, l_acc, g, code[i], 1ull, val[i]);
        }
        break;
      }
      const Code adopted = stream_read_lane(unmatched[0] ? code[0] : code[1], __builtin_ctzll(waiting));
#pragma unroll
      for (int e = 0; e < kStreamGroups; ++e) {
        if (e == st.held) {
          st.key[e] = adopted;
#pragma unroll
          for (int i = 0; i < 2; ++i) stream_accumulate(st, e, unmatched[i] && code[i] == adopted, val[i]);
        }
      }
      st.held += 1;
#pragma unroll
      for (int i = 0; i < 2; ++i) unmatched[i] = unmatched[i] && code[i] != adopted;
    }
  }
}

template <typename Shape, int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) void agg_stream_kernel(StreamColumns cols, int64_t n, HashTableView g) {
  static constexpr Translated T = Shape::translated(2 * BLOCK * U);
  static_assert(stream_serves(T), "the stream kernel does not take this plan shape");
  constexpr int NS = T.num_sums;
  constexpr unsigned kUsed = T.used_columns;
  constexpr int64_t TR = 2 * BLOCK * U;
  using Code = uint32_t;   // up to four CHAR(1) keys
  __shared__ unsigned long long l_keys[kStreamSlots];
  __shared__ unsigned long long l_acc[(NS + 1) * kStreamSlots];
  for (int i = threadIdx.x; i < kStreamSlots; i += BLOCK) l_keys[i] = kEmptyCode;
  for (int i = threadIdx.x; i < (NS + 1) * kStreamSlots; i += BLOCK) l_acc[i] = 0ull;
  __syncthreads();

  StreamState<NS, Code> st;
#pragma unroll
  for (int e = 0; e < kStreamGroups; ++e) {
    st.cnt[e] = 0u;
    st.key[e] = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) st.acc[e][j] = 0.0;
  }
  st.held = 0;

  // full tiles, strided by the grid, two per iteration (register sets a and b).  The loop has one exit, at its end: an exit
  // between the two halves would reach the loop's latch with b's loads pending as far as the compiler can tell, and every
  // iteration would then begin by waiting for all loads.  The second half of a workgroup's last pair may have no next tile:
  // it loads its own tile again (the result is never used) rather than put a branch between the loads and the arithmetic.
  const int64_t num_full = n / TR, stride = gridDim.x;
  int64_t t = blockIdx.x;
  if (t < num_full) {
    StreamRows<U> a, b;
    stream_load<U, BLOCK, true>(T.dev, kUsed, cols, n, t, a);
    while (t + stride < num_full) {
      stream_load<U, BLOCK, true>(T.dev, kUsed, cols, n, t + stride, b);
      __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise sinks these loads below the first waits for the current tile)
      stream_compute<U, BLOCK, true>(T.dev, n, t, a, st, l_keys, l_acc, g);
      t += stride;
      stream_load<U, BLOCK, true>(T.dev, kUsed, cols, n, t + stride < num_full ? t + stride : t, a);
      __builtin_amdgcn_sched_barrier(0);
      stream_compute<U, BLOCK, true>(T.dev, n, t, b, st, l_keys, l_acc, g);
      t += stride;
    }
    if (t < num_full) stream_compute<U, BLOCK, true>(T.dev, n, t, a, st, l_keys, l_acc, g);
  }
  // the ragged last tile, every row under its own predicate: one workgroup
  if (num_full * TR < n && static_cast<int64_t>(blockIdx.x) == num_full % stride) {
    StreamRows<U> a;
    stream_load<U, BLOCK, false>(T.dev, kUsed, cols, n, num_full, a);
    stream_compute<U, BLOCK, false>(T.dev, n, num_full, a, st, l_keys, l_acc, g);
  }

  // registers -> the workgroup's table: across the wave first, then one lane per wave and group
#pragma unroll
  for (int e = 0; e < kStreamGroups; ++e) {
    const unsigned long long rows = wave_reduce_add(static_cast<unsigned long long>(st.cnt[e]));
    double sum[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) sum[j] = wave_reduce_add(st.acc[e][j]);
    if (lane_id() == 0 && e < st.held && rows != 0) {
      stream_table_add<NS>(l_keys, l_acc, g, static_cast<unsigned long long>(st.key[e]), rows, sum);
    }
  }
  __syncthreads();
  // the table -> the state: one global atomic per group and accumulator
  for (int sl = threadIdx.x; sl < kStreamSlots; sl += BLOCK) {
    const unsigned long long code = l_keys[sl], rows = l_acc[sl];
    if (code == kEmptyCode || rows == 0) continue;
    const unsigned long long gs = global_find_or_insert(g, code);
    if (gs == ~0ull) continue;
    global_add(g, 0, gs, rows, kAccSumI64);
#pragma unroll
    for (int j = 0; j < NS; ++j) global_add(g, j + 1, gs, l_acc[(j + 1) * kStreamSlots + sl], kAccSumF64);
  }
}

// Launch geometry: one 256-thread workgroup per CU, one step per tile (two rows per lane in flight next to the two being
// added up).  More of either — two or four steps per tile, 512 threads, two or four workgroups per CU — measured slower:
// six read streams per workgroup run fastest with little in flight (tools/ubench/read_ceiling.hip).
constexpr int kStreamU = 1;
constexpr int kStreamBlock = 256;

}  // namespace

bool agg_stream_enabled() {
  const char *e = getenv("QSX_AGG_STREAM");
  return e == nullptr || atoi(e) != 0;
}

// Below this many rows a call keeps the staged-tile kernel: a stored block's 123 k rows took 19.5 us here against 15.5 us
// there, 500 k rows the same, 2 M rows and more less.  QSX_AGG_STREAM_MIN_ROWS, read per call, moves the
// threshold: the tests put row counts around every tile boundary through this kernel.
static int64_t stream_min_rows() {
  const char *e = getenv("QSX_AGG_STREAM_MIN_ROWS");
  return e != nullptr ? atoll(e) : 2000000;
}

template <typename Shape>
bool AggStream<Shape>::takes(const void *const *cols, int num_columns, int64_t n) {
  static constexpr Translated T = Shape::translated(kABlock);
  if (n <= 0 || n < stream_min_rows()) return false;
  for (int col = 0; col < T.dev.num_columns; ++col) {
    if (((T.used_columns >> col) & 1u) == 0) continue;
    if (col >= num_columns || cols[col] == nullptr) return false;
    const uintptr_t bytes = stream_value_column(T.dev, T.used_columns, col) ? 16 : 2;
    if (reinterpret_cast<uintptr_t>(cols[col]) % bytes != 0) return false;
  }
  return true;
}

template <typename Shape>
int AggStream<Shape>::launch(const void *const *cols, int num_columns, int64_t n, const HashTableView &g, hipStream_t stream) {
  if (n <= 0) return QSX_ERR_INVALID_ARGUMENT;   // (takes() says no)
  StreamColumns cp;
  for (int i = 0; i < QSX_MAX_COLUMNS; ++i) cp.p[i] = i < num_columns ? cols[i] : nullptr;
  constexpr int64_t tile_rows = 2ll * kStreamBlock * kStreamU;
  const int grid = static_cast<int>(std::min<int64_t>((n + tile_rows - 1) / tile_rows, kCUs));
  if (getenv("QSX_DEBUG_LAUNCH") != nullptr) {
    std::fprintf(stderr, "[qsx] stream launch grid=%d block=%d n=%lld\n", grid, kStreamBlock, static_cast<long long>(n));
  }
  hipLaunchKernelGGL((agg_stream_kernel<Shape, kStreamU, kStreamBlock>), dim3(grid), dim3(kStreamBlock), 0, stream, cp, n, g);
  return QSX_OK;
}

template struct AggStream<ShapeTpchQ1>;

}  // namespace qsx
