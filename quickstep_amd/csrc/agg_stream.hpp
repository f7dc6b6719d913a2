// agg_stream.hpp — the stream kernel of the ahead-of-time plan shapes (agg_shapes.hpp) for a handful of groups.
//
// The hash update kernel (agg_hash_update.hpp) stages every tile in LDS and touches LDS three times per row: the staging
// write, the argument reads and one atomic per accumulator.  With a handful of groups none of that is needed: the rows go from
// HBM straight into registers, and every lane keeps the accumulators of kStreamGroups groups in registers.  LDS holds only a
// small workgroup table for the rows of further groups and for the workgroup's own reduction (agg_stream.hip).
//
// launch_shape_v (aggregate.hip) takes this kernel for the default small-group geometry over plain, suitably aligned columns;
// everything else keeps the kernels it had.
#ifndef QSX_CSRC_AGG_STREAM_HPP_
#define QSX_CSRC_AGG_STREAM_HPP_

#include "agg_shapes.hpp"

namespace qsx {

constexpr int kStreamGroups = 4;   // groups a lane holds in registers
constexpr int kStreamSlots = 16;   // slots of the workgroup's LDS table

// Plans the kernel template takes: CHAR(1) keys packed into one code (at most four: the code is 32 bits), DOUBLE arguments,
// a double expression program, SUM / AVG / COUNT(*) only (every accumulator an f64 sum), no predicate, no nullable or coded
// column.  Of the registered shapes that is TPC-H Q1; the two-INT-keys shape keeps the staged-tile kernel.
constexpr bool stream_serves(const Translated &t) {
  const DevConfig &d = t.dev;
  if (t.status != QSX_OK || t.dense || d.wide_words != 0 || d.num_pred != 0 || d.num_null_cols != 0) return false;
  if (d.num_keys < 1 || t.num_sums < 1 || t.num_sums > 6) return false;
  bool is_key[QSX_MAX_COLUMNS] = {};
  for (int k = 0; k < d.num_keys; ++k) {
    const int col = d.key_column[k], type = d.column_type[col];
    if (type != QSX_CHAR || d.key_width[k] != 1) return false;
    is_key[col] = true;
  }
  for (int col = 0; col < d.num_columns; ++col) {
    if (d.code_width[col] != 0) return false;
    if (((t.used_columns >> col) & 1u) && !is_key[col] && d.column_type[col] != QSX_DOUBLE) return false;
  }
  auto double_operand = [&](const DevOperand &o) {
    return o.kind == QSX_OPD_CONST || o.kind == QSX_OPD_TEMP || (o.kind == QSX_OPD_COLUMN && d.column_type[o.index] == QSX_DOUBLE);
  };
  for (int i = 0; i < d.num_instrs; ++i) {
    if (d.instrs[i].op < QSX_EX_ADD || d.instrs[i].op >= QSX_EX_IADD) return false;
    if (!double_operand(d.instrs[i].a) || !double_operand(d.instrs[i].b)) return false;
  }
  for (int j = 0; j < t.num_sums; ++j) {
    const DevSum &s = d.sums[j];
    if (s.kind != kAccSumF64 || s.is_int != 0 || s.count_valid != 0 || s.null_mask != 0) return false;
    if (s.arg.kind == QSX_OPD_CONST || !double_operand(s.arg)) return false;
  }
  return true;
}

struct StreamColumns {
  const void *p[QSX_MAX_COLUMNS];
};

template <typename Shape>
struct AggStream {
  // The kernel takes this call: there are enough rows (QSX_AGG_STREAM_MIN_ROWS, 2 M by default), every DOUBLE column the plan reads is 16-byte aligned and every key column
  // 2-byte aligned (a lane reads its two rows with one load per column).
  static bool takes(const void *const *cols, int num_columns, int64_t n);
  // One update launch over n rows of plain columns into the state's table g.
  static int launch(const void *const *cols, int num_columns, int64_t n, const HashTableView &g, hipStream_t stream);
};

// QSX_AGG_STREAM=0 (read per call) keeps the hash update kernel for every launch.
bool agg_stream_enabled();

}  // namespace qsx

#endif  // QSX_CSRC_AGG_STREAM_HPP_
