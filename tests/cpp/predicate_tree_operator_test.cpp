// Predicate trees (PredicateNode: OR / NOT / IN over comparison leaves) through the operators: a Select over a few thousand rows
// in several small blocks with a Q19-shaped OR of three conjunctions, Q12's l_shipmode IN (..) behind a range on the sort
// column, Q16's NOT IN together with NOT LIKE and <>, and NOT over a nullable attribute (the reference selects the NULL rows:
// expressions/predicate/NegationPredicate.cpp:70-90) — on plain blocks, on compressed blocks with a dictionary per block, on a
// sorted column, per block and over a run (which must stay on the run path).  Then an aggregation with a tree predicate against
// exact integer sums, SUM(CASE WHEN a = x OR a = y THEN 1 ELSE 0 END) with ONE WHEN, the refusals, and a conjuncts-only predicate
// against the same terms as a tree's conjunction.  Expected rows are computed here on the host columns.
#include <algorithm>
#include <cstring>
#include <functional>
#include <set>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kId = 0, kSize, kQty, kBrand, kContainer, kMode, kType, kPrio, kKey };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};
const char *kBrands[] = {"Brand#12", "Brand#23", "Brand#34", "Brand#45", "Brand#51"};
const char *kContainers[] = {"SM CASE", "SM BOX", "SM PACK", "SM PKG", "MED BAG", "MED BOX", "MED PKG", "MED PACK", "LG CASE", "LG BOX", "LG PACK", "LG PKG", "JUMBO JAR", "WRAP DRUM"};
const char *kModes[] = {"MAIL", "SHIP", "AIR", "REG AIR", "TRUCK", "RAIL", "FOB"};
const char *kTypes[] = {"MEDIUM POLISHED TIN", "MEDIUM POLISHED BRASS", "STANDARD PLATED BRASS", "PROMO ANODIZED STEEL", "SMALL POLISHED COPPER", "MEDIUM BURNISHED TIN"};
const char *kPrios[] = {"1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"};

struct Rows {
  std::vector<std::int32_t> id, size, qty, key;
  std::vector<char> brand, container, mode, type, prio;   // CHAR(10) x 3, CHAR(25), CHAR(15)
  std::vector<bool> qty_null;
  std::size_t n = 0;
  Rows() {
    std::uint64_t s = 0x2545F4914F6CDD1Dull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (std::int64_t b : kBlockSizes) n += static_cast<std::size_t>(b);
    brand.assign(n * 10, 0);
    container.assign(n * 10, 0);
    mode.assign(n * 10, 0);
    type.assign(n * 25, 0);
    prio.assign(n * 15, 0);
    for (std::size_t r = 0; r < n; ++r) {
      id.push_back(static_cast<std::int32_t>(r));
      size.push_back(static_cast<std::int32_t>(rnd() % 50) + 1);
      qty.push_back(static_cast<std::int32_t>(rnd() % 40) + 1);
      qty_null.push_back(rnd() % 5 == 0);
      std::strncpy(&brand[r * 10], kBrands[rnd() % 5], 10);
      std::strncpy(&container[r * 10], kContainers[rnd() % 14], 10);
      std::strncpy(&mode[r * 10], kModes[rnd() % 7], 10);
      std::strncpy(&type[r * 25], kTypes[rnd() % 6], 25);
      std::strncpy(&prio[r * 15], kPrios[rnd() % 5], 15);
    }
    // the sort column: ascending inside every block, few distinct far-apart values (a dictionary when compressed)
    std::size_t at = 0;
    for (std::int64_t b : kBlockSizes) {
      std::vector<std::int32_t> k;
      for (std::int64_t i = 0; i < b; ++i) k.push_back(static_cast<std::int32_t>(rnd() % 60) * 1000003 + 17);
      std::sort(k.begin(), k.end());
      key.insert(key.end(), k.begin(), k.end());
      at += static_cast<std::size_t>(b);
    }
  }
  std::string text(const std::vector<char> &col, int width, std::size_t r) const {
    return std::string(&col[r * width], ::strnlen(&col[r * width], width));
  }
  std::string brandOf(std::size_t r) const { return text(brand, 10, r); }
  std::string containerOf(std::size_t r) const { return text(container, 10, r); }
  std::string modeOf(std::size_t r) const { return text(mode, 10, r); }
  std::string typeOf(std::size_t r) const { return text(type, 25, r); }
  std::string prioOf(std::size_t r) const { return text(prio, 15, r); }
};

enum Layout { kPlain = 0, kCompressed, kSorted, kSortedCompressed };

void load(const Rows &t, CatalogRelation *rel, StorageManager *storage, Layout layout) {
  rel->addAttribute("id", Type::Int());
  rel->addAttribute("p_size", Type::Int());
  rel->addAttribute("l_quantity", Type::Int().getNullableVersion());
  rel->addAttribute("p_brand", Type::Char(10));
  rel->addAttribute("p_container", Type::Char(10));
  rel->addAttribute("l_shipmode", Type::Char(10));
  rel->addAttribute("p_type", Type::Char(25));
  rel->addAttribute("o_orderpriority", Type::Char(15));
  rel->addAttribute("key", Type::Int());
  const bool compressed = layout == kCompressed || layout == kSortedCompressed;
  const std::vector<bool> compress = {false, true, false, true, true, true, true, false, true};
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    std::vector<std::uint64_t> nulls(static_cast<std::size_t>(n) / 64 + 2, 0);
    for (std::size_t r = 0; r < static_cast<std::size_t>(n); ++r) if (t.qty_null[at + r]) nulls[r / 64] |= 1ull << (63 - r % 64);
    // (the 777-row block gets no null bitmap contents at all: every quantity there counts as present)
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, n > 0 && n != 777 ? nulls.data() : nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, nullptr};
    const block_id id = storage->loadBlock(rel, {t.id.data() + at, t.size.data() + at, t.qty.data() + at, t.brand.data() + at * 10,
                                                 t.container.data() + at * 10, t.mode.data() + at * 10, t.type.data() + at * 25,
                                                 t.prio.data() + at * 15, t.key.data() + at}, n, 0, compressed ? &compress : nullptr, &bitmaps);
    if (layout == kSorted || layout == kSortedCompressed) storage->getBlock(id)->setSortColumn(kKey);
    at += static_cast<std::size_t>(n);
  }
  if (compressed) {
    const BlockReference b = storage->getBlock(rel->getBlocksSnapshot().front());
    EXPECT_TRUE(b->compressedAttribute(kSize) != nullptr && b->compressedAttribute(kSize)->kind == CompressedAttribute::kTruncated);
    EXPECT_TRUE(b->compressedAttribute(kMode) != nullptr && b->compressedAttribute(kMode)->kind == CompressedAttribute::kDictionary);
    EXPECT_TRUE(b->compressedAttribute(kContainer) != nullptr && b->compressedAttribute(kType) != nullptr);
    EXPECT_TRUE(b->compressedAttribute(kKey) != nullptr && b->compressedAttribute(kKey)->kind == CompressedAttribute::kDictionary);
  }
}

// Whether quantity r counts as NULL in the loaded relation (the 777-row block was loaded without null bits).
bool qtyNull(const Rows &t, std::size_t r) {
  const std::size_t first_777 = 2500 + 1001, end_777 = first_777 + 777;
  return t.qty_null[r] && !(r >= first_777 && r < end_777);
}

typedef std::function<bool(const Rows &, std::size_t)> RowTest;
struct Query {
  const char *name;
  Predicate predicate;
  RowTest want;
};

TypedLiteral C(const char *text) { return TypedLiteral::Char(text); }
std::vector<TypedLiteral> Chars(std::initializer_list<const char *> texts) {
  std::vector<TypedLiteral> out;
  for (const char *t : texts) out.push_back(C(t));
  return out;
}
std::vector<TypedLiteral> Ints(std::initializer_list<int> values) {
  std::vector<TypedLiteral> out;
  for (int v : values) out.push_back(TypedLiteral::Int(v));
  return out;
}
bool in(const std::string &v, std::initializer_list<const char *> texts) {
  for (const char *t : texts) if (v == t) return true;
  return false;
}
bool in(int v, std::initializer_list<int> values) { return std::find(values.begin(), values.end(), v) != values.end(); }
bool between(int v, int lo, int hi) { return v >= lo && v <= hi; }

std::vector<Query> queries() {
  typedef Predicate P;
  std::vector<Query> q;
  const auto leg = [](const char *brand, std::vector<TypedLiteral> containers, int qty_lo, int size_hi) {
    return P::And({P::Compare(kBrand, ComparisonID::kEqual, C(brand)), P::In(kContainer, std::move(containers)),
                   P::Compare(kQty, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(qty_lo)),
                   P::Compare(kQty, ComparisonID::kLessOrEqual, TypedLiteral::Int(qty_lo + 10)),
                   P::Compare(kSize, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(1)),
                   P::Compare(kSize, ComparisonID::kLessOrEqual, TypedLiteral::Int(size_hi)), P::In(kMode, Chars({"AIR", "REG AIR"}))});
  };
  // Q19: three OR-ed conjunctions; l_quantity is nullable, and a NULL quantity passes none of them
  q.push_back({"q19", P::Tree(P::Or({leg("Brand#12", Chars({"SM CASE", "SM BOX", "SM PACK", "SM PKG"}), 1, 15),
                                     leg("Brand#23", Chars({"MED BAG", "MED BOX", "MED PKG", "MED PACK"}), 10, 30),
                                     leg("Brand#34", Chars({"LG CASE", "LG BOX", "LG PACK", "LG PKG"}), 20, 45)})),
               [](const Rows &t, std::size_t r) {
                 const bool mode = in(t.modeOf(r), {"AIR", "REG AIR"});
                 const bool qty_ok = !qtyNull(t, r);
                 return (t.brandOf(r) == "Brand#12" && in(t.containerOf(r), {"SM CASE", "SM BOX", "SM PACK", "SM PKG"}) && qty_ok &&
                         between(t.qty[r], 1, 11) && between(t.size[r], 1, 15) && mode) ||
                        (t.brandOf(r) == "Brand#23" && in(t.containerOf(r), {"MED BAG", "MED BOX", "MED PKG", "MED PACK"}) && qty_ok &&
                         between(t.qty[r], 10, 20) && between(t.size[r], 1, 30) && mode) ||
                        (t.brandOf(r) == "Brand#34" && in(t.containerOf(r), {"LG CASE", "LG BOX", "LG PACK", "LG PKG"}) && qty_ok &&
                         between(t.qty[r], 20, 30) && between(t.size[r], 1, 45) && mode);
               }});
  // Q12: l_shipmode IN ('MAIL', 'SHIP') behind a range on the (sort) column, which stays a top-level conjunct
  Predicate q12 = P::Tree(P::In(kMode, Chars({"MAIL", "SHIP"})));
  q12.conjuncts = {{kKey, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(10 * 1000003 + 17)}, {kKey, ComparisonID::kLess, TypedLiteral::Int(40 * 1000003 + 17)}};
  q.push_back({"q12", q12, [](const Rows &t, std::size_t r) {
                 return t.key[r] >= 10 * 1000003 + 17 && t.key[r] < 40 * 1000003 + 17 && in(t.modeOf(r), {"MAIL", "SHIP"});
               }});
  // Q16: p_brand <> 'Brand#45' AND p_type NOT LIKE 'MEDIUM POLISHED%' AND p_size NOT IN (8 values)
  q.push_back({"q16", P::Tree(P::And({P::Compare(kBrand, ComparisonID::kNotEqual, C("Brand#45")), P::Compare(kType, ComparisonID::kNotLike, C("MEDIUM POLISHED%")),
                                      P::NotIn(kSize, Ints({49, 14, 23, 45, 19, 3, 36, 9}))})),
               [](const Rows &t, std::size_t r) {
                 return t.brandOf(r) != "Brand#45" && t.typeOf(r).compare(0, 15, "MEDIUM POLISHED") != 0 && !in(t.size[r], {49, 14, 23, 45, 19, 3, 36, 9});
               }});
  // NOT over a nullable attribute: the reference selects the rows whose l_quantity is NULL (two-valued logic)
  q.push_back({"not_over_null", P::Tree(P::And({P::Not(P::Compare(kQty, ComparisonID::kLess, TypedLiteral::Int(30))), P::NotIn(kQty, Ints({31, 33, 35, 37, 39})),
                                                P::In(kKey, Ints({17, 3 * 1000003 + 17, 20 * 1000003 + 17, 21 * 1000003 + 17, 59 * 1000003 + 17, 5}))})),
               [](const Rows &t, std::size_t r) {
                 const bool null = qtyNull(t, r);
                 const bool lt30 = !null && t.qty[r] < 30, in_odd = !null && in(t.qty[r], {31, 33, 35, 37, 39});
                 return !lt30 && !in_odd && in(t.key[r] / 1000003, {0, 3, 20, 21, 59});
               }});
  // an IN list of more than QSX_MAX_IN_LIST literals: several IN leaves under an OR (on the sort column of the sorted layouts,
  // against the dictionaries of the compressed ones)
  std::vector<TypedLiteral> many;
  for (int k = 0; k < 40; ++k) many.push_back(TypedLiteral::Int((k == 39 ? 59 : k) * 1000003 + 17));   // keys 0..38 and 59
  q.push_back({"long_list", P::Tree(P::Or({P::Not(P::In(kKey, many)), P::Compare(kSize, ComparisonID::kLess, TypedLiteral::Int(3))})),
               [](const Rows &t, std::size_t r) {
                 const int k = t.key[r] / 1000003;
                 return !(k <= 38 || k == 59) || t.size[r] < 3;
               }});
  // Q12 behind a lower bound every key passes (the smallest is 17): on the compressed layouts the rewrite of `key >= 5` is
  // "every code" in every block — block by block a scan of the code stripe, on the sort column too; over a run of sorted blocks
  // one more search
  Predicate q12_open = q12;
  q12_open.conjuncts[0] = {kKey, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(5)};
  q.push_back({"q12_open", q12_open, [](const Rows &t, std::size_t r) {
                 return t.key[r] >= 5 && t.key[r] < 40 * 1000003 + 17 && in(t.modeOf(r), {"MAIL", "SHIP"});
               }});
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

void runSelects(const Rows &t, Layout layout, std::size_t blocks_per_order) {
  for (const Query &query : queries()) {
    CatalogRelation rel(1, "t"), out(2, "out");
    StorageManager storage;
    load(t, &rel, &storage, layout);
    out.addAttribute("id", Type::Int());
    QueryContext ctx;
    const auto pred = ctx.addPredicate(query.predicate);
    const auto dest = ctx.addInsertDestination(&out, &storage);
    SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
    select.setBlocksPerWorkOrder(blocks_per_order);
    const std::int64_t block_before = NumPredicateTreeBlockEvaluations(), run_before = NumPredicateTreeRunEvaluations();
    fetchAndExecuteWorkOrders(&select, &ctx, &storage);
    const std::int64_t by_block = NumPredicateTreeBlockEvaluations() - block_before, by_run = NumPredicateTreeRunEvaluations() - run_before;
    if (blocks_per_order > 1) {   // the run stays on the run path: one qsx_bitmap_eval_blocks, nothing block by block
      EXPECT_EQ(by_run, std::int64_t(1));
      EXPECT_EQ(by_block, std::int64_t(0));
    } else {
      EXPECT_EQ(by_run, std::int64_t(0));
      EXPECT_EQ(by_block, static_cast<std::int64_t>(kBlockSizes.size()));
    }
    std::size_t rows = 0, want_rows = 0, nulls_selected = 0;
    const std::set<std::int32_t> ids = selectedIds(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks(), &rows);
    bool same = true;
    for (std::size_t r = 0; r < t.n; ++r) {
      const bool want = query.want(t, r);
      want_rows += want;
      if (want != (ids.count(static_cast<std::int32_t>(r)) != 0)) same = false;
      if (want && qtyNull(t, r)) ++nulls_selected;
    }
    if (!same || rows != want_rows) std::fprintf(stderr, "query %s, layout %d, %zu blocks per order: %zu rows, want %zu\n", query.name, layout, blocks_per_order, rows, want_rows);
    EXPECT_TRUE(same);
    EXPECT_EQ(rows, want_rows);
    EXPECT_TRUE(want_rows > 20 && want_rows < t.n);
    if (std::string(query.name) == "not_over_null") EXPECT_TRUE(nulls_selected > 20);   // the NOT-over-NULL rows are present
    if (std::string(query.name) == "q19") EXPECT_EQ(nulls_selected, std::size_t(0));
  }
}

// select sum(p_size), count(*) from t where <q16>  — and the one-WHEN CASE: sum(case when prio = '1-URGENT' or prio = '2-HIGH' then 1 else 0 end)
void runAggregation(const Rows &t, Layout layout, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage, layout);
  result.addAttribute("sum_size", Type::Long());
  result.addAttribute("rows", Type::Long());
  result.addAttribute("high", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  const Query q16 = queries()[2];
  const Predicate urgent_or_high = Predicate::Tree(Predicate::Or({Predicate::Compare(kPrio, ComparisonID::kEqual, C("1-URGENT")),
                                                                  Predicate::Compare(kPrio, ComparisonID::kEqual, C("2-HIGH"))}));
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.predicate = &q16.predicate;
  spec.aggregates = {AggregateSpec(AggregationID::kSum, kSize), AggregateSpec(AggregationID::kCount, kInvalidAttributeID),
                     AggregateSpec(AggregationID::kSum, Scalar::Case({{urgent_or_high, Scalar::Literal(1.0)}}, Scalar::Literal(0.0)))};
  spec.strategy = QSX_AGG_SINGLE_STATE;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::int64_t want_sum = 0, want_rows = 0, want_high = 0;
  for (std::size_t r = 0; r < t.n; ++r) {
    if (!q16.want(t, r)) continue;
    want_sum += t.size[r];
    ++want_rows;
    want_high += t.prioOf(r) == "1-URGENT" || t.prioOf(r) == "2-HIGH";
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  EXPECT_EQ(blocks.size(), std::size_t(1));
  if (blocks.size() != 1) return;
  BlockReference b = storage.getBlock(blocks[0]);
  EXPECT_EQ(b->numTuples(), std::int64_t(1));
  double high = 0;
  std::int64_t sum = 0, rows = 0;
  b->copyAttributeToHost(0, &sum);
  b->copyAttributeToHost(1, &rows);
  b->copyAttributeToHost(2, &high);
  EXPECT_TRUE(want_rows > 100 && want_high > 10 && want_high < want_rows);
  EXPECT_EQ(sum, want_sum);
  EXPECT_EQ(rows, want_rows);
  EXPECT_TRUE(high == static_cast<double>(want_high));   // integers far below 2^53: exact in any order
}

int statusOf(const std::function<void()> &body, std::string *message = nullptr) {
  try {
    body();
  } catch (const ExecutionError &e) {
    if (message != nullptr) *message = e.what();
    return e.status();
  }
  return QSX_OK;
}

void runRefusals(const Rows &t) {
  const Predicate tree = Predicate::Tree(Predicate::Or({Predicate::Compare(kSize, ComparisonID::kLess, TypedLiteral::Int(3)),
                                                        Predicate::Compare(kSize, ComparisonID::kGreater, TypedLiteral::Int(47))}));
  std::string message;
  {  // a join's residual predicate cannot carry a tree
    CatalogRelation rel(1, "t"), result(2, "result");
    StorageManager storage;
    load(t, &rel, &storage, kPlain);
    result.addAttribute("id", Type::Int());
    QueryContext ctx;
    const auto table = ctx.addJoinHashTable(kInt, 16, 1);
    const auto dest = ctx.addInsertDestination(&result, &storage);
    const auto selection = ctx.addScalarGroup({kId});
    const auto residual = ctx.addPredicate(tree);
    const std::vector<bool> on_build = {false};
    BuildHashOperator builder(0, rel, true, {kId}, false, 1, table);
    fetchAndExecuteWorkOrders(&builder, &ctx, &storage);
    HashJoinOperator prober(0, rel, rel, true, {kId}, false, 1, false, result, dest, table, residual, selection, &on_build,
                            HashJoinOperator::JoinType::kInnerJoin);
    EXPECT_EQ(statusOf([&]() { fetchAndExecuteWorkOrders(&prober, &ctx, &storage); }, &message), static_cast<int>(QSX_ERR_UNSUPPORTED));
    EXPECT_TRUE(message.find("residual") != std::string::npos && message.find("tree") != std::string::npos);
    DestroyHashOperator cleaner(0, 1, table);
    fetchAndExecuteWorkOrders(&cleaner, &ctx, &storage);
  }
  {  // the terms of a qsx_agg_config_t cannot hold a tree: with nowhere else to put it, it is refused; with an external predicate it goes there
    CatalogRelation rel(1, "t");
    StorageManager storage;
    load(t, &rel, &storage, kPlain);
    qsx_agg_config_t config;
    std::memset(&config, 0, sizeof(config));
    Predicate both = tree;
    both.conjuncts = {{kSize, ComparisonID::kGreater, TypedLiteral::Int(1)}};
    const auto column_of = [](attribute_id a) { return static_cast<int>(a); };
    message.clear();
    EXPECT_EQ(statusOf([&]() { LowerPredicateToAggConfig(both, rel, column_of, &config, nullptr); }, &message), static_cast<int>(QSX_ERR_UNSUPPORTED));
    EXPECT_TRUE(message.find("qsx_agg_config_t") != std::string::npos && message.find("tree") != std::string::npos);
    Predicate external;
    EXPECT_EQ(statusOf([&]() { LowerPredicateToAggConfig(both, rel, column_of, &config, &external); }), static_cast<int>(QSX_OK));
    EXPECT_EQ(config.num_pred_terms, 1);
    EXPECT_TRUE(external.conjuncts.empty() && external.tree == tree.tree);
  }
  {  // what a tree cannot express here
    CatalogRelation rel(1, "t");
    StorageManager storage;
    load(t, &rel, &storage, kPlain);
    const BlockReference block = storage.getBlock(rel.getBlocksSnapshot().front());
    const auto matches = [&](const Predicate &p) {
      std::int64_t n = 0;
      qsx_device_free(p.getMatchesForBlock(*block, &n));
    };
    const Predicate wrong_type = Predicate::Tree(Predicate::In(kSize, {TypedLiteral::Int(1), TypedLiteral::Long(2)}));
    EXPECT_EQ(statusOf([&]() { matches(wrong_type); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
    const Predicate two_attributes = Predicate::Tree(Predicate::Not(Predicate::Compare(ComparisonPredicate::Attributes(kSize, false, ComparisonID::kEqual, kQty, false))));
    EXPECT_EQ(statusOf([&]() { matches(two_attributes); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
    EXPECT_EQ(statusOf([&]() { matches(Predicate::Tree(Predicate::In(kSize, {}))); }), static_cast<int>(QSX_ERR_INVALID_ARGUMENT));
    EXPECT_EQ(statusOf([&]() { matches(Predicate::Tree(Predicate::Or({}))); }), static_cast<int>(QSX_ERR_INVALID_ARGUMENT));
    // LIKE on an attribute that is not CHAR(n), as a leaf: refused per block, over a run and inside a WHEN alike
    const Predicate like_on_int = Predicate::Tree(Predicate::Or({Predicate::Compare(kSize, ComparisonID::kLike, C("4%")),
                                                                 Predicate::Compare(kSize, ComparisonID::kLess, TypedLiteral::Int(3))}));
    EXPECT_EQ(statusOf([&]() { matches(like_on_int); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      CatalogRelation out(2, "out");
      out.addAttribute("id", Type::Int());
      QueryContext ctx;
      const auto pred = ctx.addPredicate(like_on_int);
      const auto dest = ctx.addInsertDestination(&out, &storage);
      SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
      select.setBlocksPerWorkOrder(per_order);
      EXPECT_EQ(statusOf([&]() { fetchAndExecuteWorkOrders(&select, &ctx, &storage); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
    }
    EXPECT_EQ(statusOf([&]() {
                QueryContext ctx;
                AggregationStateSpec spec;
                spec.input_relation = &rel;
                spec.aggregates = {AggregateSpec(AggregationID::kSum, Scalar::Case({{like_on_int, Scalar::Literal(1.0)}}, Scalar::Literal(0.0)))};
                spec.strategy = QSX_AGG_SINGLE_STATE;
                ctx.addAggregationState(spec);
              }), static_cast<int>(QSX_ERR_UNSUPPORTED));
    std::vector<PredicateNodePtr> deep;   // nine levels of nesting: deeper than one program holds
    PredicateNodePtr node = Predicate::Compare(kSize, ComparisonID::kLess, TypedLiteral::Int(3));
    for (int level = 0; level < 9; ++level) node = Predicate::And({Predicate::Compare(kSize, ComparisonID::kGreater, TypedLiteral::Int(level)), node});
    EXPECT_EQ(statusOf([&]() { matches(Predicate::Tree(node)); }), static_cast<int>(QSX_ERR_UNSUPPORTED));
  }
}

// A conjuncts-only predicate and the same terms as a tree's conjunction: identical bitmaps, block by block, on every layout.
void runChainAgainstTree(const Rows &t, Layout layout) {
  CatalogRelation rel(1, "t");
  StorageManager storage;
  load(t, &rel, &storage, layout);
  const std::vector<ComparisonPredicate> terms = {{kKey, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(5 * 1000003 + 17)},
                                                  {kSize, ComparisonID::kLessOrEqual, TypedLiteral::Int(30)},
                                                  {kQty, ComparisonID::kGreater, TypedLiteral::Int(7)},
                                                  {kMode, ComparisonID::kNotEqual, C("RAIL")},
                                                  {kType, ComparisonID::kLike, C("%BRASS")}};
  Predicate chain;
  chain.conjuncts = terms;
  std::vector<PredicateNodePtr> leaves;
  for (const ComparisonPredicate &term : terms) leaves.push_back(Predicate::Compare(term));
  const Predicate tree = Predicate::Tree(Predicate::And(leaves));
  std::int64_t total = 0;
  for (block_id id : rel.getBlocksSnapshot()) {
    const BlockReference block = storage.getBlock(id);
    const std::size_t words = static_cast<std::size_t>((block->numTuples() + 63) / 64);
    std::int64_t chain_count = -1, tree_count = -2;
    void *a = chain.getMatchesForBlock(*block, &chain_count), *b = tree.getMatchesForBlock(*block, &tree_count);
    std::vector<std::uint64_t> wa(words + 1, 1), wb(words + 1, 2);
    if (words > 0) {
      EXPECT_EQ(qsx_copy_to_host(wa.data(), a, words * 8, nullptr), static_cast<int>(QSX_OK));
      EXPECT_EQ(qsx_copy_to_host(wb.data(), b, words * 8, nullptr), static_cast<int>(QSX_OK));
      EXPECT_EQ(qsx_stream_synchronize(nullptr), static_cast<int>(QSX_OK));
      EXPECT_TRUE(std::equal(wa.begin(), wa.begin() + static_cast<std::ptrdiff_t>(words), wb.begin()));
    }
    EXPECT_EQ(chain_count, tree_count);
    total += chain_count;
    qsx_device_free(a);
    qsx_device_free(b);
  }
  std::int64_t want = 0;
  for (std::size_t r = 0; r < t.n; ++r) {
    const std::string type = t.typeOf(r);
    want += t.key[r] >= 5 * 1000003 + 17 && t.size[r] <= 30 && !qtyNull(t, r) && t.qty[r] > 7 && t.modeOf(r) != "RAIL" && type.size() >= 5 &&
            type.compare(type.size() - 5, 5, "BRASS") == 0;
  }
  EXPECT_EQ(total, want);
  EXPECT_TRUE(want > 50);
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "predicate_tree_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Rows t;
  for (const Layout layout : {kPlain, kCompressed, kSorted, kSortedCompressed}) {
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      runSelects(t, layout, per_order);
      runAggregation(t, layout, per_order);
    }
    runChainAgainstTree(t, layout);
  }
  runRefusals(t);
  return finish("predicate_tree_operator_test");
}
