// Comparisons of two attributes of one relation (ComparisonPredicate::Attributes as a conjunct) through the operators: Q12's
// l_commitdate < l_receiptdate AND l_shipdate < l_commitdate AND l_receiptdate >= d1 AND l_receiptdate < d2 AND l_shipmode IN (..)
// through a SelectOperator, row for row against a host loop, with one block per work order and with five (which must stay ONE run);
// INT against LONG and LONG against DOUBLE (C++'s usual arithmetic conversions); a nullable attribute on either side (NULL rows are
// never selected, the work falls to the per-block path); COUNT(*) / SUM under such a predicate through the AggregationOperator; the
// same comparison as the WHEN of a CASE; the refusals.  The relation is loaded plain and compressed: compressed, the dates are
// 2-byte codes into a dictionary per block and the INT attribute is truncated in some blocks only, so the two sides of a term differ
// in coding inside a block and from block to block.  Expected rows are computed here on the host columns.
#include <cstring>
#include <functional>
#include <set>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kId = 0, kShip, kCommit, kReceipt, kQty, kBig, kPrice, kMaybe, kMode };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};
const char *kModes[] = {"MAIL", "SHIP", "AIR", "REG AIR", "TRUCK", "RAIL", "FOB"};

struct Rows {
  std::vector<std::int32_t> id, qty, maybe;
  std::vector<DateLit> ship, commit, receipt;
  std::vector<std::int64_t> big;
  std::vector<double> price;
  std::vector<char> mode;   // CHAR(10)
  std::vector<bool> maybe_null;
  std::size_t n = 0;
  Rows() {
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    const auto date = [&]() {
      return DateLit::Create(1994 + static_cast<std::int32_t>(rnd() % 2), static_cast<std::uint8_t>(1 + rnd() % 6), static_cast<std::uint8_t>(1 + rnd() % 28));
    };
    for (std::int64_t b : kBlockSizes) n += static_cast<std::size_t>(b);
    mode.assign(n * 10, 0);
    for (std::size_t r = 0; r < n; ++r) {
      id.push_back(static_cast<std::int32_t>(r));
      ship.push_back(date());
      commit.push_back(rnd() % 10 == 0 ? ship.back() : date());   // (some rows committed for the very day they shipped)
      receipt.push_back(date());
      // the INT attribute: small and non-negative in the first and the last block (truncated when compressed), of both signs and
      // many values in the others (not truncated)
      const bool small = r < 2500 || r >= 2500 + 1001 + 777;
      qty.push_back(small ? static_cast<std::int32_t>(rnd() % 50) : static_cast<std::int32_t>(rnd() % 200001) - 100000);
      // the LONG attribute around the INT one, with values no int32 and no double holds
      const std::uint64_t kind = rnd() % 8;
      big.push_back(kind == 0 ? (std::int64_t(1) << 53) + 1 : kind == 1 ? 4294967295ll : kind == 2 ? -(std::int64_t(1) << 40)
                                                                                       : static_cast<std::int64_t>(qty.back()) + static_cast<std::int64_t>(rnd() % 3) - 1);
      // the DOUBLE attribute around the LONG one: equal, half above, 2^53 (which 2^53 + 1 equals in double)
      const std::uint64_t pk = rnd() % 4;
      price.push_back(pk == 0 ? static_cast<double>(big.back()) : pk == 1 ? static_cast<double>(big.back()) + 0.5 : pk == 2 ? 9007199254740992.0 : -3.25);
      maybe.push_back(static_cast<std::int32_t>(rnd() % 50));
      maybe_null.push_back(rnd() % 4 == 0);
      std::strncpy(&mode[r * 10], kModes[rnd() % 7], 10);
    }
  }
  std::string modeOf(std::size_t r) const { return std::string(&mode[r * 10], ::strnlen(&mode[r * 10], 10)); }
};

void load(const Rows &t, CatalogRelation *rel, StorageManager *storage, bool compressed) {
  rel->addAttribute("id", Type::Int());
  rel->addAttribute("l_shipdate", Type::Date());
  rel->addAttribute("l_commitdate", Type::Date());
  rel->addAttribute("l_receiptdate", Type::Date());
  rel->addAttribute("qty", Type::Int());
  rel->addAttribute("big", Type::Long());
  rel->addAttribute("price", Type::Double());
  rel->addAttribute("maybe", Type::Int().getNullableVersion());
  rel->addAttribute("l_shipmode", Type::Char(10));
  const std::vector<bool> compress = {false, true, true, true, true, false, false, false, true};
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    std::vector<std::uint64_t> nulls(static_cast<std::size_t>(n) / 64 + 2, 0);
    for (std::size_t r = 0; r < static_cast<std::size_t>(n); ++r) if (t.maybe_null[at + r]) nulls[r / 64] |= 1ull << (63 - r % 64);
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n > 0 ? nulls.data() : nullptr, nullptr};
    storage->loadBlock(rel, {t.id.data() + at, t.ship.data() + at, t.commit.data() + at, t.receipt.data() + at, t.qty.data() + at, t.big.data() + at,
                             t.price.data() + at, t.maybe.data() + at, t.mode.data() + at * 10}, n, 0, compressed ? &compress : nullptr, &bitmaps);
    at += static_cast<std::size_t>(n);
  }
  if (compressed) {
    const std::vector<block_id> ids = rel->getBlocksSnapshot();
    const BlockReference first = storage->getBlock(ids[0]), second = storage->getBlock(ids[1]);
    for (const attribute_id a : {kShip, kCommit, kReceipt}) {
      EXPECT_TRUE(first->compressedAttribute(a) != nullptr && first->compressedAttribute(a)->kind == CompressedAttribute::kDictionary);
      EXPECT_TRUE(first->compressedAttribute(a) != nullptr && first->compressedAttribute(a)->code_width == 2);
    }
    EXPECT_TRUE(first->compressedAttribute(kQty) != nullptr && first->compressedAttribute(kQty)->kind == CompressedAttribute::kTruncated);
    EXPECT_TRUE(second->compressedAttribute(kQty) == nullptr || second->compressedAttribute(kQty)->kind != CompressedAttribute::kTruncated);
  }
}

typedef std::function<bool(const Rows &, std::size_t)> RowTest;
struct Query {
  const char *name;
  Predicate predicate;
  RowTest want;
  bool nullable;   // a term over the nullable attribute: the run falls to the per-block path
};

ComparisonPredicate A(attribute_id lhs, ComparisonID c, attribute_id rhs) { return ComparisonPredicate::Attributes(lhs, false, c, rhs, false); }

std::vector<Query> queries() {
  std::vector<Query> q;
  // Q12: two comparisons of two dates, a range on one of them, and the IN list as the tree
  Predicate q12 = Predicate::Tree(Predicate::In(kMode, {TypedLiteral::Char("MAIL"), TypedLiteral::Char("SHIP")}));
  q12.conjuncts = {A(kCommit, ComparisonID::kLess, kReceipt), A(kShip, ComparisonID::kLess, kCommit),
                   {kReceipt, ComparisonID::kGreaterOrEqual, TypedLiteral::Date(1994, 3, 1)}, {kReceipt, ComparisonID::kLess, TypedLiteral::Date(1995, 3, 1)}};
  q.push_back({"q12", q12, [](const Rows &t, std::size_t r) {
                 const DateLit d1 = DateLit::Create(1994, 3, 1), d2 = DateLit::Create(1995, 3, 1);
                 return t.commit[r] < t.receipt[r] && t.ship[r] < t.commit[r] && !(t.receipt[r] < d1) && t.receipt[r] < d2 &&
                        (t.modeOf(r) == "MAIL" || t.modeOf(r) == "SHIP");
               }, false});
  // Q4 / Q21 alone, the other way round, and equality of dates
  Predicate q21;
  q21.conjuncts = {A(kReceipt, ComparisonID::kGreater, kCommit), A(kShip, ComparisonID::kNotEqual, kReceipt)};
  q.push_back({"q21", q21, [](const Rows &t, std::size_t r) { return t.commit[r] < t.receipt[r] && !(t.ship[r] == t.receipt[r]); }, false});
  Predicate same_day;
  same_day.conjuncts = {A(kShip, ComparisonID::kEqual, kCommit)};
  q.push_back({"same_day", same_day, [](const Rows &t, std::size_t r) { return t.ship[r] == t.commit[r]; }, false});
  // INT against LONG: compared in int64 (4294967295 is no -1); behind a literal term (on an attribute every block holds the same
  // way: a literal term on the INT attribute, truncated in some blocks only, would send the run to the per-block path by itself)
  Predicate int_long;
  int_long.conjuncts = {{kId, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(100)}, A(kQty, ComparisonID::kLess, kBig)};
  q.push_back({"int_long", int_long, [](const Rows &t, std::size_t r) { return t.id[r] >= 100 && static_cast<std::int64_t>(t.qty[r]) < t.big[r]; }, false});
  Predicate long_int;
  long_int.conjuncts = {A(kBig, ComparisonID::kEqual, kQty)};
  q.push_back({"long_int", long_int, [](const Rows &t, std::size_t r) { return t.big[r] == static_cast<std::int64_t>(t.qty[r]); }, false});
  // LONG against DOUBLE: compared in double (2^53 + 1 equals 2^53)
  Predicate long_double;
  long_double.conjuncts = {A(kBig, ComparisonID::kGreaterOrEqual, kPrice)};
  q.push_back({"long_double", long_double, [](const Rows &t, std::size_t r) { return static_cast<double>(t.big[r]) >= t.price[r]; }, false});
  Predicate double_int;
  double_int.conjuncts = {A(kPrice, ComparisonID::kLessOrEqual, kQty), A(kCommit, ComparisonID::kLessOrEqual, kReceipt)};
  q.push_back({"double_int", double_int, [](const Rows &t, std::size_t r) {
                 return t.price[r] <= static_cast<double>(t.qty[r]) && !(t.receipt[r] < t.commit[r]);
               }, false});
  // the nullable attribute on either side: a NULL row is never selected, not even by <>
  Predicate null_left;
  null_left.conjuncts = {A(kMaybe, ComparisonID::kNotEqual, kQty)};
  q.push_back({"null_left", null_left, [](const Rows &t, std::size_t r) { return !t.maybe_null[r] && t.maybe[r] != t.qty[r]; }, true});
  Predicate null_right;
  null_right.conjuncts = {A(kCommit, ComparisonID::kLess, kReceipt), A(kQty, ComparisonID::kLessOrEqual, kMaybe)};
  q.push_back({"null_right", null_right, [](const Rows &t, std::size_t r) {
                 return t.commit[r] < t.receipt[r] && !t.maybe_null[r] && t.qty[r] <= t.maybe[r];
               }, true});
  return q;
}

std::set<std::int32_t> selectedIds(StorageManager *storage, const std::vector<block_id> &blocks, std::size_t *rows) {
  std::set<std::int32_t> ids;
  *rows = 0;
  for (block_id b : blocks) {
    BlockReference blk = storage->getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    std::vector<std::int32_t> v(k);
    blk->copyAttributeToHost(0, v.data());
    ids.insert(v.begin(), v.end());
    *rows += k;
  }
  return ids;
}

void runSelects(const Rows &t, bool compressed, std::size_t blocks_per_order) {
  for (const Query &query : queries()) {
    CatalogRelation rel(1, "t"), out(2, "out");
    StorageManager storage;
    load(t, &rel, &storage, compressed);
    out.addAttribute("id", Type::Int());
    QueryContext ctx;
    const auto pred = ctx.addPredicate(query.predicate);
    const auto dest = ctx.addInsertDestination(&out, &storage);
    SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
    select.setBlocksPerWorkOrder(blocks_per_order);
    std::int64_t terms = 0;
    for (const ComparisonPredicate &term : query.predicate.conjuncts) terms += term.rhs_attribute != kInvalidAttributeID;
    const std::int64_t block_before = NumAttributeComparisonBlockEvaluations(), run_before = NumAttributeComparisonRunEvaluations();
    const std::int64_t tree_run_before = NumPredicateTreeRunEvaluations();
    fetchAndExecuteWorkOrders(&select, &ctx, &storage);
    const std::int64_t by_block = NumAttributeComparisonBlockEvaluations() - block_before, by_run = NumAttributeComparisonRunEvaluations() - run_before;
    if (blocks_per_order > 1 && !query.nullable) {   // the five blocks stayed ONE run: one launch per term, nothing block by block
      EXPECT_EQ(by_run, terms);
      EXPECT_EQ(by_block, std::int64_t(0));
      if (query.predicate.tree != nullptr) EXPECT_EQ(NumPredicateTreeRunEvaluations() - tree_run_before, std::int64_t(1));
    } else {                                         // one block per order, or a nullable operand: the per-block path
      EXPECT_EQ(by_run, std::int64_t(0));
      EXPECT_EQ(by_block, terms * static_cast<std::int64_t>(kBlockSizes.size()));
    }
    std::size_t rows = 0, want_rows = 0;
    const std::set<std::int32_t> ids = selectedIds(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks(), &rows);
    bool same = true, null_selected = false;
    for (std::size_t r = 0; r < t.n; ++r) {
      const bool want = query.want(t, r);
      want_rows += want;
      const bool got = ids.count(static_cast<std::int32_t>(r)) != 0;
      if (want != got) same = false;
      if (got && query.nullable && t.maybe_null[r]) null_selected = true;
    }
    if (!same || rows != want_rows) {
      std::fprintf(stderr, "query %s, %s, %zu blocks per order: %zu rows, want %zu\n", query.name, compressed ? "compressed" : "plain", blocks_per_order, rows, want_rows);
    }
    EXPECT_TRUE(same);
    EXPECT_EQ(rows, want_rows);
    EXPECT_TRUE(want_rows > 20 && want_rows < t.n);
    EXPECT_TRUE(!null_selected);
  }
}

// select count(*), sum(qty), sum(case when l_commitdate < l_receiptdate then 1 else 0 end) from t where l_shipdate < l_commitdate and qty < big
void runAggregation(const Rows &t, bool compressed, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage, compressed);
  result.addAttribute("rows", Type::Long());
  result.addAttribute("sum_qty", Type::Long());
  result.addAttribute("late", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  Predicate where, late;
  where.conjuncts = {A(kShip, ComparisonID::kLess, kCommit), A(kQty, ComparisonID::kLess, kBig)};
  late.conjuncts = {A(kCommit, ComparisonID::kLess, kReceipt)};
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.predicate = &where;
  spec.aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID), AggregateSpec(AggregationID::kSum, kQty),
                     AggregateSpec(AggregationID::kSum, Scalar::Case({{late, Scalar::Literal(1.0)}}, Scalar::Literal(0.0)))};
  spec.strategy = QSX_AGG_SINGLE_STATE;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::int64_t want_rows = 0, want_sum = 0, want_late = 0;
  for (std::size_t r = 0; r < t.n; ++r) {
    if (!(t.ship[r] < t.commit[r] && static_cast<std::int64_t>(t.qty[r]) < t.big[r])) continue;
    ++want_rows;
    want_sum += t.qty[r];
    want_late += t.commit[r] < t.receipt[r];
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  EXPECT_EQ(blocks.size(), std::size_t(1));
  if (blocks.size() != 1) return;
  BlockReference b = storage.getBlock(blocks[0]);
  EXPECT_EQ(b->numTuples(), std::int64_t(1));
  std::int64_t rows = 0, sum = 0;
  double late_rows = 0;
  b->copyAttributeToHost(0, &rows);
  b->copyAttributeToHost(1, &sum);
  b->copyAttributeToHost(2, &late_rows);
  EXPECT_TRUE(want_rows > 100 && want_late > 10 && want_late < want_rows);
  EXPECT_EQ(rows, want_rows);
  EXPECT_EQ(sum, want_sum);
  EXPECT_TRUE(late_rows == static_cast<double>(want_late));   // integers far below 2^53: exact in any order
}

int statusOf(const std::function<void()> &body, std::string *message) {
  message->clear();
  try {
    body();
  } catch (const ExecutionError &e) {
    *message = e.what();
    return e.status();
  }
  return QSX_OK;
}

void runRefusals(const Rows &t) {
  CatalogRelation rel(1, "t");
  StorageManager storage;
  load(t, &rel, &storage, false);
  const BlockReference block = storage.getBlock(rel.getBlocksSnapshot().front());
  std::string message;
  // every refusal on the per-block path and over a run of five blocks
  const auto refused = [&](const Predicate &p, int status, const char *word) {
    EXPECT_EQ(statusOf([&]() {
                std::int64_t n = 0;
                qsx_device_free(p.getMatchesForBlock(*block, &n));
              }, &message), status);
    EXPECT_TRUE(message.find(word) != std::string::npos);
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      CatalogRelation out(2, "out");
      out.addAttribute("id", Type::Int());
      QueryContext ctx;
      const auto pred = ctx.addPredicate(p);
      const auto dest = ctx.addInsertDestination(&out, &storage);
      SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
      select.setBlocksPerWorkOrder(per_order);
      EXPECT_EQ(statusOf([&]() { fetchAndExecuteWorkOrders(&select, &ctx, &storage); }, &message), status);
      EXPECT_TRUE(message.find(word) != std::string::npos);
    }
  };
  const auto conjunct = [](const ComparisonPredicate &term) {
    Predicate p;
    p.conjuncts = {term};
    return p;
  };
  refused(conjunct(A(kMode, ComparisonID::kEqual, kMode)), QSX_ERR_UNSUPPORTED, "CHAR(n)");
  refused(conjunct(A(kQty, ComparisonID::kLess, kMode)), QSX_ERR_UNSUPPORTED, "CHAR(n)");
  refused(conjunct(A(kMode, ComparisonID::kLike, kMode)), QSX_ERR_UNSUPPORTED, "LIKE");
  refused(conjunct(A(kCommit, ComparisonID::kLess, kQty)), QSX_ERR_UNSUPPORTED, "DATE");
  refused(conjunct(A(kBig, ComparisonID::kLess, kReceipt)), QSX_ERR_UNSUPPORTED, "DATE");
  refused(conjunct(ComparisonPredicate::Attributes(kCommit, true, ComparisonID::kLess, kReceipt, false)), QSX_ERR_INVALID_ARGUMENT, "join residual");
  refused(conjunct(ComparisonPredicate::Attributes(kCommit, false, ComparisonID::kLess, kReceipt, true)), QSX_ERR_INVALID_ARGUMENT, "join residual");
  // as a LEAF of a tree the comparison of two attributes stays refused, with the message it always had
  refused(Predicate::Tree(Predicate::Or({Predicate::Compare(A(kCommit, ComparisonID::kLess, kReceipt)),
                                         Predicate::Compare(kQty, ComparisonID::kLess, TypedLiteral::Int(3))})),
          QSX_ERR_UNSUPPORTED, "predicate tree: a comparison of two attributes as a leaf");
  // the WHEN of a CASE is checked when the state is made
  EXPECT_EQ(statusOf([&]() {
              QueryContext ctx;
              AggregationStateSpec spec;
              spec.input_relation = &rel;
              spec.aggregates = {AggregateSpec(AggregationID::kSum, Scalar::Case({{conjunct(A(kCommit, ComparisonID::kLess, kQty)), Scalar::Literal(1.0)}}, Scalar::Literal(0.0)))};
              spec.strategy = QSX_AGG_SINGLE_STATE;
              ctx.addAggregationState(spec);
            }, &message), static_cast<int>(QSX_ERR_UNSUPPORTED));
  EXPECT_TRUE(message.find("DATE") != std::string::npos);
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "attribute_comparison_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Rows t;
  for (const bool compressed : {false, true}) {
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      runSelects(t, compressed, per_order);
      runAggregation(t, compressed, per_order);
    }
  }
  runRefusals(t);
  return finish("attribute_comparison_operator_test");
}
