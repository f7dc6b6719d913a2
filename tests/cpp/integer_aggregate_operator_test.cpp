// AggregationStateSpec::integer_argument_arithmetic through the operators: aggregates whose argument is an integer-typed
// scalar expression, evaluated as the reference's ArithmeticBinaryOperators evaluate them (INT op INT wraps to 32 bits, anything
// with a LONG to 64; types/operations/binary_operations/ArithmeticBinaryOperators.hpp:203-340) and typed as its catalog types
// them (SUM: LONG, MIN / MAX: the expression's type, AVG: DOUBLE).  A relation shaped like Distinct.test's foo (x INT, y DOUBLE,
// z INT group key) plus a LONG attribute w near 2^41; Foreman + Workers and the synchronous driver, work orders per block and per
// run of blocks.  With the flag: values equal to integer arithmetic done here.  Without it: DOUBLE results, as ever.
#include <cstring>
#include <vector>

#include "test_util.hpp"

using namespace quickstep;

namespace {
constexpr int kRows = 30000, kBlock = 1000, kGroups = 3;

template <typename T>
T at(const std::vector<unsigned char> &col, std::size_t i) {
  T v;
  std::memcpy(&v, col.data() + i * sizeof(T), sizeof(T));
  return v;
}
std::vector<std::vector<unsigned char>> readAll(QueryContext &ctx, QueryContext::insert_destination_id dest, StorageManager &storage,
                                                const CatalogRelation &rel, std::size_t *rows) {
  std::vector<std::vector<unsigned char>> cols(rel.size());
  *rows = 0;
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = storage.getBlock(b);
    for (std::size_t a = 0; a < rel.size(); ++a) {
      const std::size_t w = rel.getAttributeType(static_cast<attribute_id>(a)).width;
      const std::size_t at_byte = cols[a].size();
      cols[a].resize(at_byte + w * blk->numTuples());
      blk->copyAttributeToHost(static_cast<attribute_id>(a), cols[a].data() + at_byte);
    }
    *rows += static_cast<std::size_t>(blk->numTuples());
  }
  return cols;
}

std::int32_t wrap32(std::int64_t v) { return static_cast<std::int32_t>(static_cast<std::uint32_t>(static_cast<std::uint64_t>(v))); }

struct Want {   // per group, in the reference's integer arithmetic
  std::uint64_t sum_2x = 0;        // SUM(x + x): INT terms (wrapped to 32 bits), summed in int64
  std::uint64_t sum_x_wide = 0;    // SUM(x * 5000000000): LONG terms
  std::int32_t min_x_7 = INT32_MAX;   // MIN(x - 7): INT
  std::int64_t sum_xx = 0;         // AVG(x * x): INT terms
  std::uint64_t sum_w_x = 0;       // SUM(w + x): LONG terms, the sum beyond 2^53
  std::int64_t count = 0;
  // the same in double arithmetic: what the state returns without the flag
  double d_sum_2x = 0, d_min_x_7 = 1e300, d_sum_w_x = 0;
};
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "integer_aggregate_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  StorageManager storage;
  CatalogRelation foo(130, "foo");
  foo.addAttribute("x", Type::Int());
  foo.addAttribute("y", Type::Double());
  foo.addAttribute("z", Type::Int());
  foo.addAttribute("w", Type::Long());
  Want want[kGroups];
  int wrapped_sums = 0;
  for (int b = 0; b < kRows; b += kBlock) {
    std::vector<std::int32_t> x(kBlock), z(kBlock);
    std::vector<double> y(kBlock);
    std::vector<std::int64_t> w(kBlock);
    for (int t = 0; t < kBlock; ++t) {
      const int i = b + t;
      // every tenth row beyond +-2^30: x + x and x * x leave the INT range there
      x[t] = i % 10 == 0 ? (i % 20 == 0 ? 1 : -1) * ((1 << 30) + i) : i * 71 - 1000000;
      y[t] = 0.5 * i;
      z[t] = i % kGroups;
      w[t] = (static_cast<std::int64_t>(1) << 41) + 2 * static_cast<std::int64_t>(i) + 1;
      Want &g = want[z[t]];
      const std::int64_t xv = x[t];
      const std::int32_t two_x = wrap32(xv + xv);
      wrapped_sums += two_x != xv + xv ? 1 : 0;
      g.sum_2x += static_cast<std::uint64_t>(static_cast<std::int64_t>(two_x));
      g.sum_x_wide += static_cast<std::uint64_t>(xv) * static_cast<std::uint64_t>(5000000000ll);
      g.min_x_7 = std::min(g.min_x_7, wrap32(xv - 7));
      g.sum_xx += wrap32(static_cast<std::int64_t>(static_cast<std::uint64_t>(xv) * static_cast<std::uint64_t>(xv)));
      g.sum_w_x += static_cast<std::uint64_t>(w[t]) + static_cast<std::uint64_t>(xv);
      ++g.count;
      g.d_sum_2x += static_cast<double>(xv) + static_cast<double>(xv);
      g.d_min_x_7 = std::min(g.d_min_x_7, static_cast<double>(xv) - 7.0);
      g.d_sum_w_x += static_cast<double>(w[t]) + static_cast<double>(xv);
    }
    storage.loadBlock(&foo, {x.data(), y.data(), z.data(), w.data()}, kBlock);
  }
  EXPECT_TRUE(wrapped_sums > kRows / 20);
  for (const Want &g : want) {
    // (beyond 2^53: a double accumulator cannot be trusted with it)
    EXPECT_TRUE(static_cast<std::int64_t>(g.sum_w_x) > (static_cast<std::int64_t>(1) << 53));
  }
  const ScalarPtr x = Scalar::Attribute(0), w = Scalar::Attribute(3);
  const std::vector<AggregateSpec> aggregates = {
      AggregateSpec(AggregationID::kSum, Scalar::Binary(BinaryOperationID::kAdd, x, x)),
      AggregateSpec(AggregationID::kSum, Scalar::Binary(BinaryOperationID::kMultiply, x, Scalar::IntLiteral(5000000000ll))),
      AggregateSpec(AggregationID::kMin, Scalar::Binary(BinaryOperationID::kSubtract, x, Scalar::IntLiteral(7))),
      AggregateSpec(AggregationID::kAvg, Scalar::Binary(BinaryOperationID::kMultiply, x, x)),
      AggregateSpec(AggregationID::kSum, Scalar::Binary(BinaryOperationID::kAdd, w, x)),
      AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  for (const bool integer : {true, false}) {
    for (const bool foreman_driver : {false, true}) {
      for (const int blocks_per_work_order : {1, 8}) {
        for (const qsx_agg_strategy_t strategy : {QSX_AGG_COMPACT_KEY, QSX_AGG_GENERIC, QSX_AGG_COLLISION_FREE}) {
          CatalogRelation result(131, "result");
          result.addAttribute("z", Type::Int());
          result.addAttribute("sum_2x", integer ? Type::Long() : Type::Double());
          result.addAttribute("sum_x_wide", integer ? Type::Long() : Type::Double());
          result.addAttribute("min_x_7", integer ? Type::Int() : Type::Double());
          result.addAttribute("avg_xx", Type::Double());
          result.addAttribute("sum_w_x", integer ? Type::Long() : Type::Double());
          result.addAttribute("count", Type::Long());
          QueryContext ctx;
          AggregationStateSpec spec;
          spec.input_relation = &foo;
          spec.group_by = {2};
          spec.aggregates = aggregates;
          spec.strategy = strategy;
          spec.estimated_num_groups = kGroups;
          spec.collision_free_num_entries = kGroups;
          spec.integer_argument_arithmetic = integer;
          const auto state = ctx.addAggregationState(spec);
          const auto dest = ctx.addInsertDestination(&result, &storage);
          if (foreman_driver) {
            auto *aggregate = new AggregationOperator(0, foo, true, state);
            aggregate->setBlocksPerWorkOrder(blocks_per_work_order);
            QueryPlan plan;
            const auto a = plan.addRelationalOperator(aggregate);
            const auto fz = plan.addRelationalOperator(new FinalizeAggregationOperator(0, state, 1, false, 1, result, dest));
            plan.addDirectDependency(fz, a, true);
            ForemanSingleNode foreman(&plan, &ctx, &storage, 4);
            foreman.run();
          } else {
            AggregationOperator op(0, foo, true, state);
            op.setBlocksPerWorkOrder(blocks_per_work_order);
            FinalizeAggregationOperator fin(0, state, 1, false, 1, result, dest);
            fetchAndExecuteWorkOrders(&op, &ctx, &storage);
            fetchAndExecuteWorkOrders(&fin, &ctx, &storage);
          }
          std::size_t rows = 0;
          auto cols = readAll(ctx, dest, storage, result, &rows);
          EXPECT_EQ(rows, static_cast<std::size_t>(kGroups));
          for (std::size_t i = 0; i < rows && i < static_cast<std::size_t>(kGroups); ++i) {
            const int zv = at<std::int32_t>(cols[0], i);
            EXPECT_TRUE(zv >= 0 && zv < kGroups);
            if (zv < 0 || zv >= kGroups) continue;
            const Want &g = want[zv];
            EXPECT_EQ(at<std::int64_t>(cols[6], i), g.count);
            if (integer) {
              EXPECT_EQ(at<std::int64_t>(cols[1], i), static_cast<std::int64_t>(g.sum_2x));
              EXPECT_EQ(at<std::int64_t>(cols[2], i), static_cast<std::int64_t>(g.sum_x_wide));
              EXPECT_EQ(at<std::int32_t>(cols[3], i), g.min_x_7);
              EXPECT_TRUE(at<double>(cols[4], i) == static_cast<double>(g.sum_xx) / static_cast<double>(g.count));
              EXPECT_EQ(at<std::int64_t>(cols[5], i), static_cast<std::int64_t>(g.sum_w_x));
            } else {
              // evaluated in double, typed DOUBLE: sums of integers below 2^53 are exact in any order, the others close
              EXPECT_TRUE(at<double>(cols[1], i) == g.d_sum_2x);
              EXPECT_TRUE(at<double>(cols[3], i) == g.d_min_x_7);
              EXPECT_NEAR(at<double>(cols[5], i), g.d_sum_w_x, 1e-9 * g.d_sum_w_x);
            }
          }
        }
      }
    }
  }
  return finish("integer_aggregate_operator_test");
}
