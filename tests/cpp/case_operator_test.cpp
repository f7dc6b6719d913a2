// Scalar::kCaseExpression through the operators: a Select projecting a DOUBLE CASE and a nullable INT CASE; Q14's shape
// SUM(CASE WHEN p_type LIKE 'PROMO%' THEN x * (1 - y) ELSE 0 END), SUM(x * (1 - y)) per block and over a run (the run leg must
// stay on the run path); Q12's shape — two WHENs with CHAR(15) equality and result 1, summed as LONG under
// integer_argument_arithmetic, grouped by a CHAR(10) key; the reference's own SUM(CASE WHEN i < 4 THEN i ELSE i * i END) = 47
// (query_optimizer/tests/execution_generator/Select.test:742-752); COUNT / AVG / SUM over a CASE with NULLs, a group whose every
// row is NULL finalizing as NULL; and the refusals.  Expected results are computed here on the host columns.
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kId = 0, kX, kY, kType, kPrio, kMode, kI, kJ };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};

struct Lines {
  std::vector<std::int32_t> id, i, j;
  std::vector<double> x, y;
  std::vector<char> type, prio, mode;   // CHAR(25), CHAR(15), CHAR(10)
  std::vector<bool> i_null;
  std::size_t n = 0;
  Lines() {
    const char *types[] = {"PROMO BRUSHED TIN", "STANDARD PLATED BRASS", "PROMO ANODIZED STEEL", "SMALL POLISHED COPPER", "ECONOMY PROMO NICKEL", "MEDIUM BURNISHED TIN"};
    const char *prios[] = {"1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"};
    const char *modes[] = {"MAIL", "SHIP", "AIR", "REG AIR", "TRUCK"};
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (std::int64_t b : kBlockSizes) n += static_cast<std::size_t>(b);
    type.assign(n * 25, 0);
    prio.assign(n * 15, 0);
    mode.assign(n * 10, 0);
    for (std::size_t r = 0; r < n; ++r) {
      id.push_back(static_cast<std::int32_t>(r));
      x.push_back(static_cast<double>(4 * (rnd() % 25000 + 1)));          // multiples of 4: x * (1 - y) is an integer,
      y.push_back(static_cast<double>(rnd() % 3) * 0.25);                 // every sum exact in any order
      std::strncpy(&type[r * 25], types[rnd() % 6], 25);
      std::strncpy(&prio[r * 15], prios[rnd() % 5], 15);                  // "4-NOT SPECIFIED" fills all 15 bytes
      std::strncpy(&mode[r * 10], modes[rnd() % 5], 10);
      i.push_back(static_cast<std::int32_t>(rnd() % 2001) - 1000);
      j.push_back(static_cast<std::int32_t>(rnd() % 9));
      i_null.push_back(rnd() % 4 == 0);
    }
  }
  bool promo(std::size_t r) const { return std::strncmp(&type[r * 25], "PROMO", 5) == 0; }
  std::string prioOf(std::size_t r) const { return std::string(&prio[r * 15], ::strnlen(&prio[r * 15], 15)); }
  std::string modeOf(std::size_t r) const { return std::string(&mode[r * 10], ::strnlen(&mode[r * 10], 10)); }
};

void load(const Lines &t, CatalogRelation *rel, StorageManager *storage) {
  rel->addAttribute("id", Type::Int());
  rel->addAttribute("x", Type::Double());
  rel->addAttribute("y", Type::Double());
  rel->addAttribute("p_type", Type::Char(25));
  rel->addAttribute("o_orderpriority", Type::Char(15));
  rel->addAttribute("l_shipmode", Type::Char(10));
  rel->addAttribute("i", Type::Int().getNullableVersion());
  rel->addAttribute("j", Type::Int());
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    std::vector<std::uint64_t> nulls(static_cast<std::size_t>(n) / 64 + 2, 0);
    for (std::size_t r = 0; r < static_cast<std::size_t>(n); ++r) if (t.i_null[at + r]) nulls[r / 64] |= 1ull << (63 - r % 64);
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n > 0 ? nulls.data() : nullptr, nullptr};
    storage->loadBlock(rel, {t.id.data() + at, t.x.data() + at, t.y.data() + at, t.type.data() + at * 25, t.prio.data() + at * 15,
                             t.mode.data() + at * 10, t.i.data() + at, t.j.data() + at}, n, 0, nullptr, &bitmaps);
    at += static_cast<std::size_t>(n);
  }
}

Predicate Where(std::initializer_list<ComparisonPredicate> terms) { Predicate p; p.conjuncts = terms; return p; }
ScalarPtr Revenue() {
  return Scalar::Binary(BinaryOperationID::kMultiply, Scalar::Attribute(kX),
                        Scalar::Binary(BinaryOperationID::kSubtract, Scalar::Literal(1.0), Scalar::Attribute(kY)));
}
ScalarPtr PromoRevenue() {
  return Scalar::Case({{Where({{kType, ComparisonID::kLike, TypedLiteral::Char("PROMO%")}}), Revenue()}}, Scalar::Literal(0.0));
}
// CASE WHEN j < 3 THEN i WHEN j < 6 THEN i + j END — i is nullable, no ELSE
ScalarPtr NullableIntCase() {
  return Scalar::Case({{Where({{kJ, ComparisonID::kLess, TypedLiteral::Int(3)}}), Scalar::Attribute(kI)},
                       {Where({{kJ, ComparisonID::kLess, TypedLiteral::Int(6)}}),
                        Scalar::Binary(BinaryOperationID::kAdd, Scalar::Attribute(kI), Scalar::Attribute(kJ))}}, nullptr);
}

template <typename T>
std::vector<T> column(StorageManager *storage, const std::vector<block_id> &blocks, attribute_id a, std::vector<bool> *is_null = nullptr) {
  std::vector<T> v;
  for (block_id b : blocks) {
    BlockReference blk = storage->getBlock(b);
    const std::size_t at = v.size(), k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    v.resize(at + k);
    blk->copyAttributeToHost(a, v.data() + at);
    if (is_null != nullptr) {
      std::vector<std::uint64_t> nulls((k + 63) / 64 + 1, 0);
      blk->copyNullBitmapToHost(a, nulls.data());
      for (std::size_t r = 0; r < k; ++r) is_null->push_back((nulls[r >> 6] >> (63 - (r & 63))) & 1u);
    }
  }
  return v;
}

// select id, <double case>, <nullable int case> from t where j >= 1
void runSelect(const Lines &t, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), out(2, "out");
  StorageManager storage;
  load(t, &rel, &storage);
  out.addAttribute("id", Type::Int());
  out.addAttribute("promo_revenue", Type::Double());
  out.addAttribute("picked", Type::Int().getNullableVersion());
  QueryContext ctx;
  const auto pred = ctx.addPredicate(Where({{kJ, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(1)}}));
  const auto dest = ctx.addInsertDestination(&out, &storage);
  SelectOperator select(0, rel, false, out, dest, pred, std::vector<ScalarPtr>{Scalar::Attribute(kId), PromoRevenue(), NullableIntCase()}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &storage);
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  std::vector<bool> picked_null;
  const std::vector<std::int32_t> ids = column<std::int32_t>(&storage, blocks, 0);
  const std::vector<double> revenue = column<double>(&storage, blocks, 1);
  const std::vector<std::int32_t> picked = column<std::int32_t>(&storage, blocks, 2, &picked_null);
  std::size_t want_rows = 0, nulls_seen = 0, values_seen = 0;
  for (std::size_t r = 0; r < t.n; ++r) want_rows += t.j[r] >= 1;
  EXPECT_EQ(ids.size(), want_rows);
  std::vector<bool> seen(t.n, false);
  for (std::size_t k = 0; k < ids.size(); ++k) {
    const std::size_t r = static_cast<std::size_t>(ids[k]);
    EXPECT_TRUE(r < t.n && !seen[r] && t.j[r] >= 1);
    seen[r] = true;
    EXPECT_TRUE(revenue[k] == (t.promo(r) ? t.x[r] * (1.0 - t.y[r]) : 0.0));
    const bool want_null = t.j[r] >= 6 || t.i_null[r];          // no WHEN holds, or the chosen branch reads a NULL i
    EXPECT_EQ(static_cast<bool>(picked_null[k]), want_null);
    if (want_null) { ++nulls_seen; continue; }
    ++values_seen;
    EXPECT_EQ(picked[k], t.j[r] < 3 ? t.i[r] : t.i[r] + t.j[r]);
  }
  EXPECT_TRUE(nulls_seen > 100 && values_seen > 100);
}

// select sum(case when p_type like 'PROMO%' then x * (1 - y) else 0 end), sum(x * (1 - y)) from t
void runQ14(const Lines &t, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  result.addAttribute("promo", Type::Double());
  result.addAttribute("all", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.aggregates = {AggregateSpec(AggregationID::kSum, PromoRevenue()), AggregateSpec(AggregationID::kSum, Revenue())};
  spec.strategy = QSX_AGG_SINGLE_STATE;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  double want_promo = 0.0, want_all = 0.0;
  for (std::size_t r = 0; r < t.n; ++r) {
    const double v = t.x[r] * (1.0 - t.y[r]);
    want_all += v;
    if (t.promo(r)) want_promo += v;
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  const std::vector<double> promo = column<double>(&storage, blocks, 0), all = column<double>(&storage, blocks, 1);
  EXPECT_EQ(promo.size(), std::size_t(1));
  EXPECT_TRUE(want_promo > 0.0 && want_promo < want_all);
  if (promo.size() == 1) {
    EXPECT_TRUE(promo[0] == want_promo);      // integers below 2^53: exact in any order, so per block and over a run agree
    EXPECT_TRUE(all[0] == want_all);
  }
  // the run leg stays on the run path: its four non-empty blocks went through qsx_eval_case_blocks and one update
  const std::int64_t in_runs = ctx.getAggregationState(state)->numBlocksWithCaseEvaluatedInRuns();
  if (blocks_per_order > 1) EXPECT_EQ(in_runs, std::int64_t(4));
}

// select l_shipmode, sum(case when prio = '1-URGENT' then 1 when prio = '2-HIGH' then 1 else 0 end),
//        sum(case when prio <> '1-URGENT' and prio <> '2-HIGH' then 1 else 0 end) from t group by l_shipmode
void runQ12(const Lines &t, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  result.addAttribute("l_shipmode", Type::Char(10));
  result.addAttribute("high_line_count", Type::Long());
  result.addAttribute("low_line_count", Type::Long());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  const auto prio = [](ComparisonID c, const char *text) { return ComparisonPredicate(kPrio, c, TypedLiteral::Char(text)); };
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by = {kMode};
  spec.aggregates = {
      AggregateSpec(AggregationID::kSum, Scalar::Case({{Where({prio(ComparisonID::kEqual, "1-URGENT")}), Scalar::IntLiteral(1)},
                                                       {Where({prio(ComparisonID::kEqual, "2-HIGH")}), Scalar::IntLiteral(1)}}, Scalar::IntLiteral(0))),
      AggregateSpec(AggregationID::kSum, Scalar::Case({{Where({prio(ComparisonID::kNotEqual, "1-URGENT"), prio(ComparisonID::kNotEqual, "2-HIGH")}),
                                                        Scalar::IntLiteral(1)}}, Scalar::IntLiteral(0)))};
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 8;
  spec.integer_argument_arithmetic = true;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::map<std::string, std::pair<std::int64_t, std::int64_t>> want, got;
  for (std::size_t r = 0; r < t.n; ++r) {
    const std::string p = t.prioOf(r);
    auto &w = want[t.modeOf(r)];
    (p == "1-URGENT" || p == "2-HIGH" ? w.first : w.second) += 1;
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  const std::vector<std::int64_t> high = column<std::int64_t>(&storage, blocks, 1), low = column<std::int64_t>(&storage, blocks, 2);
  std::size_t at = 0;
  for (block_id b : blocks) {
    BlockReference blk = storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    std::vector<char> modes(k * 10);
    blk->copyAttributeToHost(0, modes.data());
    for (std::size_t r = 0; r < k; ++r, ++at) got[std::string(&modes[r * 10], ::strnlen(&modes[r * 10], 10))] = {high[at], low[at]};
  }
  EXPECT_EQ(want.size(), std::size_t(5));
  EXPECT_TRUE(got == want);
  if (blocks_per_order > 1) EXPECT_EQ(ctx.getAggregationState(state)->numBlocksWithCaseEvaluatedInRuns(), std::int64_t(4));
}

// SELECT SUM(CASE WHEN i < 4 THEN i ELSE i * i END) FROM generate_series(1, 5) AS gs(i) — 47, in integer arithmetic
void runReferenceQuery() {
  CatalogRelation rel(1, "gs"), result(2, "result");
  StorageManager storage;
  rel.addAttribute("i", Type::Int());
  const std::vector<std::int32_t> series = {1, 2, 3, 4, 5};
  storage.loadBlock(&rel, {series.data()}, 5);
  result.addAttribute("result", Type::Long());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  const ScalarPtr i = Scalar::Attribute(0);
  spec.aggregates = {AggregateSpec(AggregationID::kSum, Scalar::Case({{Where({{0, ComparisonID::kLess, TypedLiteral::Int(4)}}), i}},
                                                                     Scalar::Binary(BinaryOperationID::kMultiply, i, i)))};
  spec.strategy = QSX_AGG_SINGLE_STATE;
  spec.integer_argument_arithmetic = true;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  const std::vector<std::int64_t> sum = column<std::int64_t>(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks(), 0);
  EXPECT_EQ(sum.size(), std::size_t(1));
  if (sum.size() == 1) EXPECT_EQ(sum[0], std::int64_t(47));
}

// select g, count(case when j < 3 then 1 end), avg(case when j < 3 then i end), sum(case when j < 3 then i end), count(*)
// from t group by g, g = id % 3 with every j of group 2 moved to >= 3: that group's CASEs are NULL in every row
void runNulls(const Lines &base, std::size_t blocks_per_order) {
  Lines t = base;
  for (std::size_t r = 0; r < t.n; ++r) {
    t.id[r] = static_cast<std::int32_t>(r % 3);
    if (r % 3 == 2 && t.j[r] < 3) t.j[r] += 3;
  }
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  result.addAttribute("g", Type::Int());
  result.addAttribute("count_case", Type::Long());
  result.addAttribute("avg_case", Type::Double().getNullableVersion());
  result.addAttribute("sum_case", Type::Double().getNullableVersion());
  result.addAttribute("count_star", Type::Long());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  const Predicate small = Where({{kJ, ComparisonID::kLess, TypedLiteral::Int(3)}});
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by = {kId};
  spec.aggregates = {AggregateSpec(AggregationID::kCount, Scalar::Case({{small, Scalar::IntLiteral(1)}}, nullptr)),
                     AggregateSpec(AggregationID::kAvg, Scalar::Case({{small, Scalar::Attribute(kI)}}, nullptr)),
                     AggregateSpec(AggregationID::kSum, Scalar::Case({{small, Scalar::Attribute(kI)}}, nullptr)),
                     AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 8;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::int64_t want_count[3] = {}, want_values[3] = {}, want_sum[3] = {}, want_star[3] = {};
  for (std::size_t r = 0; r < t.n; ++r) {
    const int g = t.id[r];
    ++want_star[g];
    if (t.j[r] >= 3) continue;
    ++want_count[g];                                  // THEN 1: not NULL whatever i is
    if (t.i_null[r]) continue;
    ++want_values[g];
    want_sum[g] += t.i[r];
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  std::vector<bool> avg_null, sum_null;
  const std::vector<std::int32_t> g = column<std::int32_t>(&storage, blocks, 0);
  const std::vector<std::int64_t> count = column<std::int64_t>(&storage, blocks, 1), star = column<std::int64_t>(&storage, blocks, 4);
  const std::vector<double> avg = column<double>(&storage, blocks, 2, &avg_null), sum = column<double>(&storage, blocks, 3, &sum_null);
  EXPECT_EQ(g.size(), std::size_t(3));
  EXPECT_TRUE(want_count[2] == 0 && want_values[0] > 100 && want_values[0] < want_count[0]);
  for (std::size_t k = 0; k < g.size(); ++k) {
    const int grp = g[k];
    EXPECT_EQ(count[k], want_count[grp]);
    EXPECT_EQ(star[k], want_star[grp]);
    EXPECT_EQ(static_cast<bool>(avg_null[k]), want_values[grp] == 0);      // the group whose every row is NULL finalizes as NULL
    EXPECT_EQ(static_cast<bool>(sum_null[k]), want_values[grp] == 0);
    if (want_values[grp] == 0) continue;
    EXPECT_TRUE(sum[k] == static_cast<double>(want_sum[grp]));
    EXPECT_TRUE(avg[k] == static_cast<double>(want_sum[grp]) / static_cast<double>(want_values[grp]));
  }
}

int statusOf(const std::function<void()> &body) {
  try {
    body();
  } catch (const ExecutionError &e) {
    return e.status();
  }
  return QSX_OK;
}

void runRefusals(const Lines &t) {
  const Predicate small = Where({{kJ, ComparisonID::kLess, TypedLiteral::Int(3)}});
  const auto select = [&](ScalarPtr scalar, Type out_type) {
    return statusOf([&]() {
      CatalogRelation rel(1, "t"), out(2, "out");
      StorageManager storage;
      load(t, &rel, &storage);
      out.addAttribute("v", out_type);
      QueryContext ctx;
      const auto dest = ctx.addInsertDestination(&out, &storage);
      SelectOperator op(0, rel, false, out, dest, QueryContext::kInvalidPredicateId, std::vector<ScalarPtr>{scalar}, true);
      fetchAndExecuteWorkOrders(&op, &ctx, &storage);
    });
  };
  const ScalarPtr inner = Scalar::Case({{small, Scalar::Attribute(kJ)}}, Scalar::IntLiteral(0));
  EXPECT_EQ(select(inner, Type::Int()), static_cast<int>(QSX_OK));
  // a CASE nested in a branch, a CASE under an arithmetic node, a CHAR-typed result
  EXPECT_EQ(select(Scalar::Case({{small, inner}}, Scalar::IntLiteral(0)), Type::Int()), static_cast<int>(QSX_ERR_UNSUPPORTED));
  EXPECT_EQ(select(Scalar::Case({{small, Scalar::IntLiteral(0)}}, inner), Type::Int()), static_cast<int>(QSX_ERR_UNSUPPORTED));
  EXPECT_EQ(select(Scalar::Binary(BinaryOperationID::kAdd, inner, Scalar::IntLiteral(1)), Type::Int()), static_cast<int>(QSX_ERR_UNSUPPORTED));
  EXPECT_EQ(select(Scalar::Case({{small, Scalar::Attribute(kMode)}}, nullptr), Type::Char(10).getNullableVersion()),
            static_cast<int>(QSX_ERR_UNSUPPORTED));
  // a CASE that can be NULL into a non-nullable attribute
  EXPECT_EQ(select(Scalar::Case({{small, Scalar::Attribute(kJ)}}, nullptr), Type::Int()), static_cast<int>(QSX_ERR_INVALID_ARGUMENT));
  // DISTINCT over a CASE
  EXPECT_EQ(statusOf([&]() {
    CatalogRelation rel(1, "t");
    StorageManager storage;
    load(t, &rel, &storage);
    QueryContext ctx;
    AggregationStateSpec spec;
    spec.input_relation = &rel;
    AggregateSpec distinct(AggregationID::kSum, inner);
    distinct.is_distinct = true;
    spec.aggregates = {distinct};
    spec.strategy = QSX_AGG_SINGLE_STATE;
    ctx.addAggregationState(spec);
  }), static_cast<int>(QSX_ERR_UNSUPPORTED));
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "case_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Lines t;
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    runSelect(t, per_order);
    runQ14(t, per_order);
    runQ12(t, per_order);
    runNulls(t, per_order);
  }
  runReferenceQuery();
  runRefusals(t);
  return finish("case_operator_test");
}
