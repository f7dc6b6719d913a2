// GROUP BY CHAR(n) through the operators: group-by attributes of CHAR(10), CHAR(15), CHAR(25) and a nullable CHAR(12) are
// interned into ids on the device (qsx_char_dict_*), grouped as INT columns and turned back into bytes at finalize.  Per block
// and over runs, synchronously and under Foreman + 4 Workers, over plain blocks and over blocks whose `mode` attribute is
// dictionary-coded (the block's dictionary is interned, the values are never decoded), with a predicate that holds a numeric
// and a LIKE term, under the GENERIC and the COMPACT_KEY strategy, with a dictionary that starts far too small, with a
// partitioned finalize, and with the sort operators behind the aggregation (TPC-H Q12's shape).  Then what stays refused.
// The checker is a std::map on the host columns; results are compared as sets, with integer-valued doubles so that every sum
// is exact.
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kMode = 0, kPrio, kName, kTag, kK, kX };
const int kWidth[] = {10, 15, 25, 12};
constexpr std::int64_t kRows = 6000, kBlockRows = 700;   // 9 blocks, the last one of 400 rows
constexpr int kNames = 500;

struct Orders {
  std::vector<char> text[4];        // mode, prio, name, tag
  std::vector<bool> tag_null;
  std::vector<std::int32_t> k;
  std::vector<double> x;
  Orders() {
    const char *modes[] = {"MAIL", "SHIP", "AIR", "REG AIR", "TRUCK", "RAIL", "FOB"};
    const char *prios[] = {"1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"};   // "4-NOT SPECIFIED" fills the field: no NUL
    const char *tags[] = {"", "a", "ab", "abb", "twelve bytes", "TWELVE BYTES"};
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int a = 0; a < 4; ++a) text[a].assign(static_cast<std::size_t>(kRows) * kWidth[a], 0);
    for (std::int64_t i = 0; i < kRows; ++i) {
      char name[32];
      std::snprintf(name, sizeof(name), "Customer#%09d", static_cast<int>(rnd() % kNames) * 7919);
      const std::string value[4] = {modes[rnd() % 7], prios[rnd() % 5], name, tags[rnd() % 6]};
      for (int a = 0; a < 4; ++a) {
        char *f = &text[a][static_cast<std::size_t>(i) * kWidth[a]];
        for (int j = 0; j < kWidth[a]; ++j) f[j] = static_cast<char>('!' + rnd() % 90);   // what lies behind a NUL is never looked at
        std::memcpy(f, value[a].data(), value[a].size());
        if (static_cast<int>(value[a].size()) < kWidth[a]) f[value[a].size()] = '\0';
      }
      tag_null.push_back(rnd() % 4 == 0);
      k.push_back(static_cast<std::int32_t>(rnd() % 4));
      x.push_back(static_cast<double>(static_cast<std::int64_t>(rnd() % 20001) - 10000));
    }
  }
  std::string field(int a, std::size_t i) const {
    const char *f = &text[a][i * kWidth[a]];
    return std::string(f, ::strnlen(f, static_cast<std::size_t>(kWidth[a])));
  }
};

std::vector<std::uint64_t> packBits(const std::vector<bool> &bits, std::size_t from, std::size_t n) {
  std::vector<std::uint64_t> words(n / 64 + 2, 0);
  for (std::size_t i = 0; i < n; ++i) {
    if (bits[from + i]) words[i / 64] |= 1ull << (63 - i % 64);
  }
  return words;
}

void load(const Orders &o, CatalogRelation *rel, StorageManager *storage, bool compressed) {
  rel->addAttribute("mode", Type::Char(10));
  rel->addAttribute("prio", Type::Char(15));
  rel->addAttribute("name", Type::Char(25));
  rel->addAttribute("tag", Type::Char(12).getNullableVersion());
  rel->addAttribute("k", Type::Int());
  rel->addAttribute("x", Type::Double());
  const std::vector<bool> compress = {true, false, false, false, false, false};
  for (std::size_t at = 0; at < static_cast<std::size_t>(kRows); at += kBlockRows) {
    const std::size_t n = std::min<std::size_t>(kBlockRows, static_cast<std::size_t>(kRows) - at);
    const std::vector<std::uint64_t> nulls = packBits(o.tag_null, at, n);
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, nullptr, nulls.data(), nullptr, nullptr};
    storage->loadBlock(rel, {o.text[0].data() + at * 10, o.text[1].data() + at * 15, o.text[2].data() + at * 25, o.text[3].data() + at * 12,
                             o.k.data() + at, o.x.data() + at},
                       static_cast<std::int64_t>(n), 0, compressed ? &compress : nullptr, &bitmaps);
  }
  EXPECT_TRUE(rel->getBlocksSnapshot().size() >= 8);
  if (compressed) {
    const CompressedAttribute *c = storage->getBlock(rel->getBlocksSnapshot().front())->compressedAttribute(kMode);
    EXPECT_TRUE(c != nullptr && c->kind == CompressedAttribute::kDictionary && c->code_width == 1 && c->value_width == 10);
  }
}

struct Group {
  double sum = 0.0, min = 0.0;
  std::int64_t count = 0;
  bool operator==(const Group &o) const { return sum == o.sum && min == o.min && count == o.count; }
};
typedef std::map<std::string, Group> Groups;

struct Case {
  std::vector<attribute_id> group_by;
  qsx_agg_strategy_t strategy = QSX_AGG_COMPACT_KEY;
  bool compressed = false;
  std::size_t blocks_per_order = 1;
  bool foreman = false;
  std::int64_t estimated_groups = 16;
  std::size_t finalize_partitions = 1;
  bool with_predicate = false;     // k >= 1 AND mode LIKE '%AIR%'
};

bool RowPasses(const Orders &o, std::size_t i, const Case &c) {
  return !c.with_predicate || (o.k[i] >= 1 && o.field(kMode, i).find("AIR") != std::string::npos);
}

Groups Expected(const Orders &o, const Case &c) {
  Groups want;
  for (std::size_t i = 0; i < static_cast<std::size_t>(kRows); ++i) {
    if (!RowPasses(o, i, c)) continue;
    std::string key;
    bool null_key = false;
    for (attribute_id a : c.group_by) {
      if (a == kTag && o.tag_null[i]) null_key = true;   // a tuple with a NULL group-by key is skipped
      key += (a == kK ? std::to_string(o.k[i]) : o.field(a, i)) + "|";
    }
    if (null_key) continue;
    Group &g = want[key];
    g.min = g.count == 0 ? o.x[i] : std::min(g.min, o.x[i]);
    g.sum += o.x[i];
    g.count += 1;
  }
  return want;
}

void addResultAttributes(const Case &c, CatalogRelation *result) {
  for (attribute_id a : c.group_by) {
    if (a == kK) result->addAttribute("k", Type::Int());
    else result->addAttribute("key", Type::Char(kWidth[a]));
  }
  result->addAttribute("sum", Type::Double());
  result->addAttribute("avg", Type::Double());
  result->addAttribute("min", Type::Double());
  result->addAttribute("count", Type::Long());
}

// The rows of the result blocks as (key, group); *order: the keys in the order they were read.
Groups ReadGroups(const Case &c, const std::vector<block_id> &blocks, StorageManager *storage, std::vector<std::string> *order = nullptr) {
  Groups got;
  const std::size_t nk = c.group_by.size();
  for (block_id b : blocks) {
    BlockReference blk = storage->getBlock(b);
    const std::size_t n = static_cast<std::size_t>(blk->numTuples());
    if (n == 0) continue;
    std::vector<std::string> keys(n);
    for (std::size_t k = 0; k < nk; ++k) {
      if (c.group_by[k] == kK) {
        std::vector<std::int32_t> v(n);
        blk->copyAttributeToHost(static_cast<attribute_id>(k), v.data());
        for (std::size_t i = 0; i < n; ++i) keys[i] += std::to_string(v[i]) + "|";
        continue;
      }
      const std::size_t w = static_cast<std::size_t>(kWidth[c.group_by[k]]);
      std::vector<char> v(n * w);
      blk->copyAttributeToHost(static_cast<attribute_id>(k), v.data());
      for (std::size_t i = 0; i < n; ++i) {
        const std::size_t len = ::strnlen(&v[i * w], w);
        for (std::size_t j = len; j < w; ++j) EXPECT_TRUE(v[i * w + j] == '\0');   // the canonical value: zero-filled
        keys[i] += std::string(&v[i * w], len) + "|";
      }
    }
    std::vector<double> sum(n), avg(n), min(n);
    std::vector<std::int64_t> count(n);
    blk->copyAttributeToHost(static_cast<attribute_id>(nk), sum.data());
    blk->copyAttributeToHost(static_cast<attribute_id>(nk + 1), avg.data());
    blk->copyAttributeToHost(static_cast<attribute_id>(nk + 2), min.data());
    blk->copyAttributeToHost(static_cast<attribute_id>(nk + 3), count.data());
    for (std::size_t i = 0; i < n; ++i) {
      EXPECT_TRUE(got.count(keys[i]) == 0);                                   // every group leaves exactly once
      EXPECT_TRUE(avg[i] == sum[i] / static_cast<double>(count[i]));          // exact sums: AVG rounds once
      Group g;
      g.sum = sum[i];
      g.min = min[i];
      g.count = count[i];
      got[keys[i]] = g;
      if (order != nullptr) order->push_back(keys[i]);
    }
  }
  return got;
}

AggregationStateSpec MakeSpec(const Case &c, const CatalogRelation &rel, const Predicate *pred) {
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by = c.group_by;
  spec.aggregates = {AggregateSpec(AggregationID::kSum, kX), AggregateSpec(AggregationID::kAvg, kX), AggregateSpec(AggregationID::kMin, kX),
                     AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  spec.predicate = pred;
  spec.strategy = c.strategy;
  spec.estimated_num_groups = c.estimated_groups;
  return spec;
}

void run(const Orders &o, const Case &c, const char *what) {
  CatalogRelation rel(1, "orders"), result(2, "result");
  StorageManager storage;
  load(o, &rel, &storage, c.compressed);
  addResultAttributes(c, &result);
  QueryContext ctx;
  Predicate pred;
  pred.conjuncts.push_back(ComparisonPredicate(kK, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(1)));
  pred.conjuncts.push_back(ComparisonPredicate(kMode, ComparisonID::kLike, TypedLiteral::Char("%AIR%")));
  const Predicate *stored = c.with_predicate ? ctx.getPredicate(ctx.addPredicate(pred)) : nullptr;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  const auto state = ctx.addAggregationState(MakeSpec(c, rel, stored));
  auto *aggregate = new AggregationOperator(0, rel, true, state);
  auto *finalize = new FinalizeAggregationOperator(0, state, 1, false, c.finalize_partitions, result, dest);
  aggregate->setBlocksPerWorkOrder(c.blocks_per_order);
  if (c.foreman) {
    QueryPlan plan;
    const auto a = plan.addRelationalOperator(aggregate);
    const auto f = plan.addRelationalOperator(finalize);
    plan.addDirectDependency(f, a, true);
    ForemanSingleNode foreman(&plan, &ctx, &storage, 4);
    foreman.run();
  } else {
    std::unique_ptr<RelationalOperator> a(aggregate), f(finalize);
    fetchAndExecuteWorkOrders(a.get(), &ctx, &storage);
    fetchAndExecuteWorkOrders(f.get(), &ctx, &storage);
  }
  const Groups want = Expected(o, c);
  const Groups got = ReadGroups(c, ctx.getInsertDestination(dest)->getTouchedBlocks(), &storage);
  EXPECT_TRUE(want.size() > 1);
  if (got != want) std::fprintf(stderr, "%s: %zu groups, %zu expected\n", what, got.size(), want.size());
  EXPECT_TRUE(got == want);
  if (c.compressed) {   // the dictionaries were interned, the rows only mapped through their codes
    for (block_id b : rel.getBlocksSnapshot()) {
      BlockReference blk = storage.getBlock(b);
      EXPECT_TRUE(blk->compressedAttribute(kMode) != nullptr);
      EXPECT_TRUE(!blk->valuesMaterialized(kMode));
    }
  }
}

// select mode, sum(x), ... from orders group by mode order by mode — the aggregate's output block goes into the sort operators
void runSorted(const Orders &o) {
  Case c;
  c.group_by = {kMode};
  CatalogRelation rel(1, "orders"), result(2, "result"), runs(3, "runs"), sorted(4, "sorted");
  StorageManager storage;
  load(o, &rel, &storage, false);
  for (CatalogRelation *r : {&result, &runs, &sorted}) addResultAttributes(c, r);
  QueryContext ctx;
  const auto d_result = ctx.addInsertDestination(&result, &storage), d_runs = ctx.addInsertDestination(&runs, &storage),
             d_sorted = ctx.addInsertDestination(&sorted, &storage);
  const auto state = ctx.addAggregationState(MakeSpec(c, rel, nullptr));
  const auto sort_config = ctx.addSortConfig({{0}, {true}});
  QueryPlan plan;
  auto *aggregate = new AggregationOperator(0, rel, true, state);
  aggregate->setBlocksPerWorkOrder(4);
  const auto a = plan.addRelationalOperator(aggregate);
  const auto f = plan.addRelationalOperator(new FinalizeAggregationOperator(0, state, 1, false, 1, result, d_result));
  const auto g = plan.addRelationalOperator(new SortRunGenerationOperator(0, result, runs, d_runs, sort_config, false));
  const auto m = plan.addRelationalOperator(new SortMergeRunOperator(0, runs, sorted, d_sorted, runs, d_runs, sort_config, 4, 0, false));
  plan.addDirectDependency(f, a, true);
  plan.addDirectDependency(g, f, false);
  plan.addDirectDependency(m, g, false);
  ForemanSingleNode foreman(&plan, &ctx, &storage, 4);
  foreman.run();
  std::vector<std::string> order;
  const Groups got = ReadGroups(c, ctx.getInsertDestination(d_sorted)->getTouchedBlocks(), &storage, &order);
  EXPECT_TRUE(got == Expected(o, c));
  EXPECT_EQ(order.size(), static_cast<std::size_t>(7));
  EXPECT_TRUE(std::is_sorted(order.begin(), order.end()));
}

int statusOf(const std::function<void()> &f) {
  try {
    f();
  } catch (const ExecutionError &e) {
    return e.status();
  }
  return QSX_OK;
}

void runRefused(const Orders &o) {
  CatalogRelation rel(1, "orders");
  StorageManager storage;
  load(o, &rel, &storage, false);
  Case c;
  c.group_by = {kMode};
  {   // a DISTINCT aggregate beside an interned key
    QueryContext ctx;
    AggregationStateSpec spec = MakeSpec(c, rel, nullptr);
    AggregateSpec distinct(AggregationID::kCount, kK);
    distinct.is_distinct = true;
    spec.aggregates.push_back(distinct);
    EXPECT_EQ(statusOf([&]() { ctx.addAggregationState(spec); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
  }
  {   // the ids are local to a rank: the state is not exchanged (the refusal comes in front of the first collective)
    QueryContext ctx;
    const auto state = ctx.addAggregationState(MakeSpec(c, rel, nullptr));
    EXPECT_EQ(statusOf([&]() { ctx.getAggregationState(state)->mergeAcrossRanks(nullptr); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
  }
  {   // ... while a CHAR key the state packs itself is exchanged as before: CHAR(1) under COMPACT_KEY is not interned
    CatalogRelation flags(5, "flags");
    flags.addAttribute("flag", Type::Char(1));
    flags.addAttribute("x", Type::Double());
    const std::vector<char> flag = {'A', 'N', 'R', 'A'};
    const std::vector<double> x = {1, 2, 3, 4};
    storage.loadBlock(&flags, {flag.data(), x.data()}, 4);
    CatalogRelation result(6, "by_flag");
    result.addAttribute("flag", Type::Char(1));
    result.addAttribute("sum", Type::Double());
    QueryContext ctx;
    AggregationStateSpec spec;
    spec.input_relation = &flags;
    spec.group_by = {0};
    spec.aggregates = {AggregateSpec(AggregationID::kSum, 1)};
    spec.strategy = QSX_AGG_COMPACT_KEY;
    spec.estimated_num_groups = 4;
    const auto state = ctx.addAggregationState(spec);
    const auto dest = ctx.addInsertDestination(&result, &storage);
    AggregationOperator aggregate(0, flags, true, state);
    FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
    fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
    fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
    std::map<char, double> got;
    for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
      BlockReference blk = storage.getBlock(b);
      const std::size_t n = static_cast<std::size_t>(blk->numTuples());
      std::vector<char> key(n);
      std::vector<double> sum(n);
      blk->copyAttributeToHost(0, key.data());
      blk->copyAttributeToHost(1, sum.data());
      for (std::size_t i = 0; i < n; ++i) got[key[i]] = sum[i];
    }
    EXPECT_TRUE((got == std::map<char, double>{{'A', 5.0}, {'N', 2.0}, {'R', 3.0}}));
  }
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "char_group_by_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Orders o;
  const auto with = [](std::vector<attribute_id> group_by, void (*more)(Case *)) {
    Case c;
    c.group_by = std::move(group_by);
    if (more != nullptr) more(&c);
    return c;
  };
  const std::vector<std::vector<attribute_id>> keys = {{kMode}, {kName, kK}, {kPrio, kMode}, {kTag}};
  for (const auto &group_by : keys) {
    for (const std::size_t per_order : {std::size_t(1), std::size_t(64)}) {
      for (const bool foreman : {false, true}) {
        Case c = with(group_by, nullptr);
        c.blocks_per_order = per_order;
        c.foreman = foreman;
        run(o, c, "plain");
        c.with_predicate = true;
        run(o, c, "a numeric and a LIKE term");
        c.with_predicate = false;
        c.strategy = QSX_AGG_GENERIC;
        run(o, c, "GENERIC");
      }
    }
  }
  for (const std::size_t per_order : {std::size_t(1), std::size_t(64)}) {
    for (const bool foreman : {false, true}) {
      for (const bool with_predicate : {false, true}) {
        Case c = with({kMode}, nullptr);   // `mode` dictionary-coded: never decoded
        c.compressed = true;
        c.blocks_per_order = per_order;
        c.foreman = foreman;
        c.with_predicate = with_predicate;
        run(o, c, "dictionary-coded mode");
        c.group_by = {kPrio, kMode};
        run(o, c, "dictionary-coded mode behind a plain key");
      }
      Case small = with({kName}, nullptr);   // 500 values into a dictionary made for one: drop, reserve, repeat
      small.estimated_groups = 1;
      small.blocks_per_order = per_order;
      small.foreman = foreman;
      run(o, small, "estimated_num_groups = 1");
      small.strategy = QSX_AGG_GENERIC;
      run(o, small, "estimated_num_groups = 1, GENERIC");
      Case parts = with({kName, kK}, nullptr);
      parts.finalize_partitions = 3;
      parts.blocks_per_order = per_order;
      parts.foreman = foreman;
      run(o, parts, "finalize in 3 partitions");
    }
  }
  runSorted(o);
  runRefused(o);
  return finish("char_group_by_operator_test");
}
