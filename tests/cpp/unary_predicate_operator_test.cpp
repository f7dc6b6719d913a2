// Predicates over a unary operation (ComparisonPredicate::operand) through the operators: Q22's SUBSTRING(c_phone FROM 1 FOR 2)
// IN (7 codes) AND c_acctbal > x with the balance as a conjunct and as a leaf, NOT IN over a nullable phone (the reference
// selects the NULL rows: NegationPredicate.cpp:70-90), a unary leaf next to a leaf over the attribute itself (two leaves, not
// one), EXTRACT(YEAR) = y, a range of two conjuncts, EXTRACT(MONTH) IN (..) — a few thousand rows in several small blocks, plain
// and dictionary-compressed, per block and over a run (which must stay on the run path).  Then an aggregation whose predicate
// holds such terms against exact integer sums, SUM(CASE WHEN EXTRACT(YEAR ..) = y THEN v ELSE 0 END), and every refusal with
// its status and message.  And a DATE dictionary the term cannot be evaluated over — inside an adopted block image, at an address
// that is no multiple of 8 —, where a block reads the decoded stripe.  Expected rows are computed here on the host columns.
#include <algorithm>
#include <cstring>
#include <functional>
#include <set>
#include <string>

#include "block_image_util.hpp"
#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kId = 0, kDate, kNullableDate, kPhone, kFax, kBal, kValue };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};
const char *const kCodes[] = {"13", "31", "23", "29", "30", "18", "17"};

struct Customers {
  std::vector<std::int32_t> id, bal, value;
  std::vector<DateLit> date;
  std::vector<char> phone;   // CHAR(15)
  std::vector<bool> date_null, fax_null;
  std::size_t n = 0;
  Customers() {
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (std::int64_t b : kBlockSizes) n += static_cast<std::size_t>(b);
    phone.assign(n * 15, 0);
    for (std::size_t r = 0; r < n; ++r) {
      id.push_back(static_cast<std::int32_t>(r));
      date.push_back(DateLit::Create(1992 + static_cast<std::int32_t>(rnd() % 7), static_cast<std::uint8_t>(1 + rnd() % 12),
                                     static_cast<std::uint8_t>(1 + 7 * (rnd() % 4))));   // 336 dates: every block's dictionary pays
      bal.push_back(static_cast<std::int32_t>(rnd() % 20000) - 10000);
      value.push_back(static_cast<std::int32_t>(rnd() % 100000) + 1);
      // "CC-ddd-ddd-dddd" out of 300 numbers (a dictionary pays), 25 country codes 10..34; every 16th phone ends behind its
      // country code, with the rest of the field left as it was (bytes behind the NUL never take part)
      const int k = static_cast<int>(rnd() % 300);
      char text[32] = {};
      std::snprintf(text, sizeof(text), "%02d-%03d-%03d-%04d", 10 + k % 25, k, (7 * k) % 1000, (13 * k) % 10000);
      if (r % 16 == 5) text[2] = 0;
      std::memcpy(&phone[r * 15], text, 15);
      date_null.push_back(rnd() % 5 == 0);
      fax_null.push_back(rnd() % 7 == 0);
    }
  }
  std::string phoneOf(std::size_t r) const { return std::string(&phone[r * 15], ::strnlen(&phone[r * 15], 15)); }
  std::string code(std::size_t r) const { return phoneOf(r).substr(0, 2); }
  bool codeListed(std::size_t r) const {
    for (const char *c : kCodes) if (code(r) == c) return true;
    return false;
  }
};

void load(const Customers &t, CatalogRelation *rel, StorageManager *storage, bool compressed) {
  rel->addAttribute("id", Type::Int());
  rel->addAttribute("o_orderdate", Type::Date());
  rel->addAttribute("o_commitdate", Type::Date().getNullableVersion());
  rel->addAttribute("c_phone", Type::Char(15));
  rel->addAttribute("c_fax", Type::Char(15).getNullableVersion());
  rel->addAttribute("c_acctbal", Type::Int());
  rel->addAttribute("value", Type::Int());
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    std::vector<std::uint64_t> date_nulls(static_cast<std::size_t>(n) / 64 + 2, 0), fax_nulls(static_cast<std::size_t>(n) / 64 + 2, 0);
    for (std::size_t r = 0; r < static_cast<std::size_t>(n); ++r) {
      if (t.date_null[at + r]) date_nulls[r / 64] |= 1ull << (63 - r % 64);
      if (t.fax_null[at + r]) fax_nulls[r / 64] |= 1ull << (63 - r % 64);
    }
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, n > 0 ? date_nulls.data() : nullptr, nullptr,
                                                        n > 0 ? fax_nulls.data() : nullptr, nullptr, nullptr};
    const bool c = compressed && n > 0;
    const std::vector<bool> compress = {false, c, c, c, c, false, false};
    storage->loadBlock(rel, {t.id.data() + at, t.date.data() + at, t.date.data() + at, t.phone.data() + at * 15, t.phone.data() + at * 15,
                             t.bal.data() + at, t.value.data() + at}, n, 0, &compress, &bitmaps);
    at += static_cast<std::size_t>(n);
  }
  if (compressed) {
    const BlockReference b = storage->getBlock(rel->getBlocksSnapshot().front());
    for (attribute_id a : {kDate, kNullableDate, kPhone, kFax}) {
      EXPECT_TRUE(b->compressedAttribute(a) != nullptr && b->compressedAttribute(a)->kind == CompressedAttribute::kDictionary);
    }
  }
}

typedef Predicate P;
TypedLiteral C(const char *text) { return TypedLiteral::Char(text); }
TypedLiteral I(int v) { return TypedLiteral::Int(v); }
std::vector<TypedLiteral> Codes() {
  std::vector<TypedLiteral> out;
  for (const char *c : kCodes) out.push_back(C(c));
  return out;
}
ScalarPtr Year(attribute_id a) { return Scalar::DateExtract(QSX_DATE_YEAR, Scalar::Attribute(a)); }
ScalarPtr Month(attribute_id a) { return Scalar::DateExtract(QSX_DATE_MONTH, Scalar::Attribute(a)); }
ScalarPtr CountryCode(attribute_id a) { return Scalar::Substring(0, 2, Scalar::Attribute(a)); }
Predicate Where(std::vector<ComparisonPredicate> terms, PredicateNodePtr tree = nullptr) {
  Predicate p;
  p.conjuncts = std::move(terms);
  p.tree = std::move(tree);
  return p;
}

struct Query {
  const char *name;
  Predicate predicate;
  std::function<bool(const Customers &, std::size_t)> want;
  bool on_run_path;       // a conjunct over a nullable attribute sends a run to the per-block path, like every conjunct does
  bool selects_nulls;
};

std::vector<Query> queries() {
  std::vector<Query> q;
  // Q22: substring(c_phone from 1 for 2) in (..) and c_acctbal > x — the balance as a conjunct in front of the tree
  q.push_back({"q22_conjunct", Where({{kBal, ComparisonID::kGreater, I(1000)}}, P::In(CountryCode(kPhone), Codes())),
               [](const Customers &t, std::size_t r) { return t.bal[r] > 1000 && t.codeListed(r); }, true, false});
  // the same with both as leaves of one AND
  q.push_back({"q22_leaves", P::Tree(P::And({P::In(CountryCode(kPhone), Codes()), P::Compare(kBal, ComparisonID::kGreater, I(1000))})),
               [](const Customers &t, std::size_t r) { return t.bal[r] > 1000 && t.codeListed(r); }, true, false});
  // a comparison over the substring as a top-level conjunct, behind another conjunct's filter
  q.push_back({"code_conjunct", Where({{kBal, ComparisonID::kLess, I(5000)}, ComparisonPredicate::OnScalar(CountryCode(kPhone), ComparisonID::kGreaterOrEqual, C("30"))}),
               [](const Customers &t, std::size_t r) { return t.bal[r] < 5000 && t.code(r) >= "30"; }, true, false});
  // NOT IN over a nullable phone: the NULL rows are selected
  q.push_back({"not_in_nullable", P::Tree(P::NotIn(CountryCode(kFax), Codes())),
               [](const Customers &t, std::size_t r) { return t.fax_null[r] || !t.codeListed(r); }, true, true});
  // NOT (SUBSTRING(x ..) = '13'): the same rule
  q.push_back({"not_eq_nullable", P::Tree(P::And({P::Not(P::Compare(CountryCode(kFax), ComparisonID::kEqual, C("13"))), P::Compare(kBal, ComparisonID::kLess, I(0))})),
               [](const Customers &t, std::size_t r) { return (t.fax_null[r] || t.code(r) != "13") && t.bal[r] < 0; }, true, true});
  // a leaf over the unary and a leaf over the attribute itself, same comparison and literal: two leaves.  (Taken for one leaf,
  // x AND NOT x selects nothing and NOT x OR x everything.)
  q.push_back({"leaf_identity", P::Tree(P::And({P::Compare(CountryCode(kPhone), ComparisonID::kEqual, C("13")), P::Not(P::Compare(kPhone, ComparisonID::kEqual, C("13")))})),
               [](const Customers &t, std::size_t r) { return t.code(r) == "13" && t.phoneOf(r) != "13"; }, true, false});
  q.push_back({"leaf_identity_reversed", P::Tree(P::Or({P::Not(P::Compare(kPhone, ComparisonID::kEqual, C("13"))), P::Compare(CountryCode(kPhone), ComparisonID::kEqual, C("13"))})),
               [](const Customers &, std::size_t) { return true; }, true, false});
  q.push_back({"in_leaf_identity", P::Tree(P::And({P::In(CountryCode(kPhone), {C("13"), C("31")}), P::Not(P::In(kPhone, {C("13"), C("31")}))})),
               [](const Customers &t, std::size_t r) { return (t.code(r) == "13" || t.code(r) == "31") && t.phoneOf(r).size() > 2; }, true, false});
  // EXTRACT
  q.push_back({"year_eq", Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, I(1995))}),
               [](const Customers &t, std::size_t r) { return t.date[r].year == 1995; }, true, false});
  q.push_back({"year_range", Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kGreaterOrEqual, I(1993)),
                                    ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kLessOrEqual, I(1995))}),
               [](const Customers &t, std::size_t r) { return t.date[r].year >= 1993 && t.date[r].year <= 1995; }, true, false});
  q.push_back({"month_in", P::Tree(P::In(Month(kDate), {I(1), I(6), I(12)})),
               [](const Customers &t, std::size_t r) { return t.date[r].month == 1 || t.date[r].month == 6 || t.date[r].month == 12; }, true, false});
  // over a nullable date: as a conjunct the NULL rows are taken back, under a NOT they are selected
  q.push_back({"nullable_year_conjunct", Where({ComparisonPredicate::OnScalar(Year(kNullableDate), ComparisonID::kNotEqual, I(1994))}),
               [](const Customers &t, std::size_t r) { return !t.date_null[r] && t.date[r].year != 1994; }, false, false});
  q.push_back({"nullable_month_not", P::Tree(P::Not(P::Compare(Month(kNullableDate), ComparisonID::kLess, I(11)))),
               [](const Customers &t, std::size_t r) { return t.date_null[r] || t.date[r].month >= 11; }, true, true});
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

void runSelects(const Customers &t, bool compressed, std::size_t blocks_per_order) {
  for (const Query &query : queries()) {
    CatalogRelation rel(1, "customer"), out(2, "out");
    StorageManager storage;
    load(t, &rel, &storage, compressed);
    out.addAttribute("id", Type::Int());
    QueryContext ctx;
    const auto pred = ctx.addPredicate(query.predicate);
    const auto dest = ctx.addInsertDestination(&out, &storage);
    SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
    select.setBlocksPerWorkOrder(blocks_per_order);
    const std::int64_t block_before = NumUnaryPredicateBlockEvaluations(), run_before = NumUnaryPredicateRunEvaluations();
    fetchAndExecuteWorkOrders(&select, &ctx, &storage);
    const std::int64_t by_block = NumUnaryPredicateBlockEvaluations() - block_before, by_run = NumUnaryPredicateRunEvaluations() - run_before;
    if (blocks_per_order > 1 && query.on_run_path) {   // the run stays on the run path: the run counter moves, the block counter does not
      EXPECT_TRUE(by_run >= 1);
      EXPECT_EQ(by_block, std::int64_t(0));
    } else {
      EXPECT_EQ(by_run, std::int64_t(0));
      EXPECT_TRUE(by_block >= static_cast<std::int64_t>(kBlockSizes.size()) - 1);
    }
    std::size_t rows = 0, want_rows = 0, nulls_selected = 0;
    const std::set<std::int32_t> ids = selectedIds(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks(), &rows);
    bool same = true;
    for (std::size_t r = 0; r < t.n; ++r) {
      const bool want = query.want(t, r);
      want_rows += want;
      if (want != (ids.count(static_cast<std::int32_t>(r)) != 0)) same = false;
      if (want && (t.fax_null[r] || t.date_null[r])) ++nulls_selected;
    }
    if (!same || rows != want_rows) {
      std::fprintf(stderr, "query %s, compressed %d, %zu blocks per order: %zu rows, want %zu\n", query.name, compressed, blocks_per_order, rows, want_rows);
    }
    EXPECT_TRUE(same);
    EXPECT_EQ(rows, want_rows);
    EXPECT_TRUE(want_rows > 20 && (want_rows < t.n || std::string(query.name) == "leaf_identity_reversed"));
    if (query.selects_nulls) EXPECT_TRUE(nulls_selected > 20);
  }
}

// select sum(value), count(*), sum(case when extract(year from o_orderdate) = 1995 then value else 0 end) from customer
// where extract(year from o_orderdate) >= 1994 and c_acctbal > 0 and substring(c_phone from 1 for 2) in (..)
void runAggregation(const Customers &t, bool compressed, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "customer"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage, compressed);
  result.addAttribute("sum_value", Type::Long());
  result.addAttribute("rows", Type::Long());
  result.addAttribute("in_1995", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  const Predicate where = Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kGreaterOrEqual, I(1994)), {kBal, ComparisonID::kGreater, I(0)}},
                                P::In(CountryCode(kPhone), Codes()));
  const Predicate in_1995 = Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, I(1995))});
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.predicate = &where;
  spec.aggregates = {AggregateSpec(AggregationID::kSum, kValue), AggregateSpec(AggregationID::kCount, kInvalidAttributeID),
                     AggregateSpec(AggregationID::kSum, Scalar::Case({{in_1995, Scalar::Attribute(kValue)}}, Scalar::Literal(0.0)))};
  spec.strategy = QSX_AGG_SINGLE_STATE;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::int64_t want_sum = 0, want_rows = 0, want_1995 = 0;
  for (std::size_t r = 0; r < t.n; ++r) {
    if (!(t.date[r].year >= 1994 && t.bal[r] > 0 && t.codeListed(r))) continue;
    want_sum += t.value[r];
    ++want_rows;
    if (t.date[r].year == 1995) want_1995 += t.value[r];
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  EXPECT_EQ(blocks.size(), std::size_t(1));
  if (blocks.size() != 1) return;
  BlockReference b = storage.getBlock(blocks[0]);
  EXPECT_EQ(b->numTuples(), std::int64_t(1));
  double got_1995 = 0;
  std::int64_t sum = 0, rows = 0;
  b->copyAttributeToHost(0, &sum);
  b->copyAttributeToHost(1, &rows);
  b->copyAttributeToHost(2, &got_1995);
  EXPECT_TRUE(want_rows > 100 && want_1995 > 0 && want_1995 < want_sum);
  EXPECT_EQ(sum, want_sum);
  EXPECT_EQ(rows, want_rows);
  EXPECT_TRUE(got_1995 == static_cast<double>(want_1995));   // integers far below 2^53: exact in any order
}

// (id, o_orderdate) of the first four blocks as CompressedColumnStore images adopted in place, the dates behind 2-byte codes into
// a dictionary that follows the image's protobuf header: it lies at an address that is no multiple of 8, and the date kernels
// read 8-byte words.  UnaryOnDictionary says no, so a single block evaluates the term over the decoded stripe (stripe()), and
// RunPredicateCovers sends a run block by block — the run counter must not move.  The empty block holds a dictionary without entries.
void runAdoptedImages(const Customers &t, std::size_t blocks_per_order) {
  struct Images {
    std::vector<void *> dev;
    ~Images() { for (void *p : dev) qsx_device_free(p); }
  };
  for (const bool as_tree : {false, true}) {
    Images images;   // (outlives the storage manager whose blocks point into it)
    CatalogRelation rel(1, "orders"), out(2, "out");
    StorageManager storage;
    rel.addAttribute("id", Type::Int());
    rel.addAttribute("o_orderdate", Type::Date());
    out.addAttribute("id", Type::Int());
    block_image::Coding values, dictionary;
    dictionary.kind = block_image::Coding::kDictionary;
    dictionary.code_width = 2;
    std::size_t loaded = 0;
    for (const std::int64_t n : {2500, 1001, 0, 777}) {
      const std::vector<unsigned char> image = block_image::BuildCompressed(rel, {t.id.data() + loaded, t.date.data() + loaded}, {{}, {}}, n,
                                                                            std::size_t(1) << 21, 0, {values, dictionary});
      void *dev = nullptr;
      CheckStatus(qsx_device_alloc(image.size(), &dev), "qsx_device_alloc");
      images.dev.push_back(dev);
      CheckStatus(qsx_copy_to_device(dev, image.data(), image.size(), nullptr), "qsx_copy_to_device");
      CheckStatus(qsx_stream_synchronize(nullptr), "qsx_stream_synchronize");
      const BlockReference b = storage.getBlock(storage.adoptBlockImage(&rel, dev, image.size()));
      const CompressedAttribute *c = b->compressedAttribute(1);
      EXPECT_EQ(b->numTuples(), n);
      EXPECT_TRUE(c != nullptr && c->kind == CompressedAttribute::kDictionary && (n == 0) == (c->num_codes == 0));
      EXPECT_TRUE(c != nullptr && (reinterpret_cast<std::uintptr_t>(c->dictionary) & 7) != 0);
      loaded += static_cast<std::size_t>(n);
    }
    const std::function<bool(std::size_t)> want = as_tree ? std::function<bool(std::size_t)>([&](std::size_t r) { return t.date[r].month == 1 || t.date[r].month == 6 || t.date[r].month == 12; })
                                                          : std::function<bool(std::size_t)>([&](std::size_t r) { return t.date[r].year == 1995; });
    QueryContext ctx;
    const auto pred = ctx.addPredicate(as_tree ? P::Tree(P::In(Month(1), {I(1), I(6), I(12)}))
                                               : Where({ComparisonPredicate::OnScalar(Year(1), ComparisonID::kEqual, I(1995))}));
    const auto dest = ctx.addInsertDestination(&out, &storage);
    SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{0}, true);
    select.setBlocksPerWorkOrder(blocks_per_order);
    const std::int64_t block_before = NumUnaryPredicateBlockEvaluations(), run_before = NumUnaryPredicateRunEvaluations();
    fetchAndExecuteWorkOrders(&select, &ctx, &storage);
    EXPECT_EQ(NumUnaryPredicateRunEvaluations() - run_before, std::int64_t(0));
    EXPECT_EQ(NumUnaryPredicateBlockEvaluations() - block_before, std::int64_t(4));
    std::size_t rows = 0, want_rows = 0;
    const std::set<std::int32_t> ids = selectedIds(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks(), &rows);
    bool same = true;
    for (std::size_t r = 0; r < loaded; ++r) {
      want_rows += want(r);
      if (want(r) != (ids.count(static_cast<std::int32_t>(r)) != 0)) same = false;
    }
    EXPECT_TRUE(same);
    EXPECT_EQ(rows, want_rows);
    EXPECT_TRUE(want_rows > 20 && want_rows < loaded);
  }
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
bool says(const std::string &message, std::initializer_list<const char *> words) {
  for (const char *w : words) if (message.find(w) == std::string::npos) return false;
  return true;
}

void runRefusals(const Customers &t) {
  const int unsupported = QSX_ERR_UNSUPPORTED, invalid = QSX_ERR_INVALID_ARGUMENT;
  CatalogRelation rel(1, "customer");
  StorageManager storage;
  load(t, &rel, &storage, false);
  const BlockReference block = storage.getBlock(rel.getBlocksSnapshot().front());
  std::string message;
  const auto matches = [&](const Predicate &p) {
    std::int64_t n = 0;
    qsx_device_free(p.getMatchesForBlock(*block, &n));
  };
  const auto refused = [&](const Predicate &p, int status, std::initializer_list<const char *> words) {
    // per block, over a run, and as the WHEN of a CASE alike
    EXPECT_EQ(statusOf([&]() { matches(p); }, &message), status);
    EXPECT_TRUE(says(message, words));
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      CatalogRelation out(2, "out");
      out.addAttribute("id", Type::Int());
      QueryContext ctx;
      const auto pred = ctx.addPredicate(p);
      const auto dest = ctx.addInsertDestination(&out, &storage);
      SelectOperator select(0, rel, false, out, dest, pred, std::vector<attribute_id>{kId}, true);
      select.setBlocksPerWorkOrder(per_order);
      EXPECT_EQ(statusOf([&]() { fetchAndExecuteWorkOrders(&select, &ctx, &storage); }, &message), status);
      EXPECT_TRUE(says(message, words));
    }
  };
  // an operand that is not a unary of an attribute
  refused(Where({ComparisonPredicate::OnScalar(Scalar::Attribute(kPhone), ComparisonID::kEqual, C("13"))}), unsupported, {"not EXTRACT / SUBSTRING of an attribute"});
  refused(P::Tree(P::Compare(Scalar::Substring(0, 1, CountryCode(kPhone)), ComparisonID::kEqual, C("1"))), unsupported, {"not EXTRACT / SUBSTRING of an attribute"});
  refused(P::Tree(P::In(Scalar::Binary(BinaryOperationID::kAdd, Year(kDate), Scalar::IntLiteral(1)), {I(1996)})), unsupported,
          {"not EXTRACT / SUBSTRING of an attribute"});
  // the operation's own rules (UnaryResultType)
  refused(Where({ComparisonPredicate::OnScalar(Year(kPhone), ComparisonID::kEqual, I(1995))}), unsupported, {"EXTRACT", "DATE"});
  refused(Where({ComparisonPredicate::OnScalar(Scalar::Substring(15, 2, Scalar::Attribute(kPhone)), ComparisonID::kEqual, C("13"))}), invalid, {"SUBSTRING"});
  // LIKE / NOT LIKE over a unary
  refused(Where({ComparisonPredicate::OnScalar(CountryCode(kPhone), ComparisonID::kLike, C("1%"))}), unsupported, {"LIKE", "unary"});
  refused(P::Tree(P::Compare(CountryCode(kPhone), ComparisonID::kNotLike, C("1%"))), unsupported, {"LIKE", "unary"});
  // a literal of the wrong type
  refused(Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, C("1995"))}), unsupported, {"EXTRACT wants an INT literal"});
  refused(Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, TypedLiteral::Long(1995))}), unsupported, {"EXTRACT wants an INT literal"});
  refused(P::Tree(P::Compare(CountryCode(kPhone), ComparisonID::kEqual, I(13))), unsupported, {"SUBSTRING a CHAR literal"});
  refused(P::Tree(P::In(CountryCode(kPhone), {C("13"), I(31)})), unsupported, {"SUBSTRING a CHAR literal"});
  refused(P::Tree(P::In(Month(kDate), {I(1), TypedLiteral::Double(2.0)})), unsupported, {"EXTRACT wants an INT literal"});
  // a scalar operand combined with rhs_attribute
  ComparisonPredicate both = ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, I(1995));
  both.rhs_attribute = kBal;
  refused(Where({both}), invalid, {"rhs_attribute"});
  refused(P::Tree(P::Not(P::Compare(both))), invalid, {"rhs_attribute"});
  {  // a VARCHAR operand
    CatalogRelation texts(3, "texts");
    texts.addAttribute("id", Type::Int());
    texts.addAttribute("comment", Type::VarChar(20));
    qsx_agg_config_t config;
    std::memset(&config, 0, sizeof(config));
    Predicate external;
    const Predicate p = Where({ComparisonPredicate::OnScalar(Scalar::Substring(0, 2, Scalar::Attribute(1)), ComparisonID::kEqual, C("ab"))});
    EXPECT_EQ(statusOf([&]() { LowerPredicateToAggConfig(p, texts, [](attribute_id a) { return static_cast<int>(a); }, &config, &external); }, &message),
              unsupported);
    EXPECT_TRUE(says(message, {"VARCHAR"}));
  }
  {  // qsx_agg_config_t.pred cannot hold the term: with nowhere else to put it, it is refused; with an external predicate it goes there
    qsx_agg_config_t config;
    std::memset(&config, 0, sizeof(config));
    const Predicate p = Where({{kBal, ComparisonID::kGreater, I(0)}, ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, I(1995))});
    const auto column_of = [](attribute_id a) { return static_cast<int>(a); };
    EXPECT_EQ(statusOf([&]() { LowerPredicateToAggConfig(p, rel, column_of, &config, nullptr); }, &message), unsupported);
    EXPECT_TRUE(says(message, {"qsx_agg_config_t", "unary operation"}));
    Predicate external;
    EXPECT_EQ(statusOf([&]() { LowerPredicateToAggConfig(p, rel, column_of, &config, &external); }, &message), static_cast<int>(QSX_OK));
    EXPECT_EQ(config.num_pred_terms, 1);
    EXPECT_TRUE(external.conjuncts.size() == 1 && external.conjuncts[0].operand != nullptr && external.tree == nullptr);
  }
  {  // the WHEN of a CASE: refused where the state is made
    const Predicate like = Where({ComparisonPredicate::OnScalar(CountryCode(kPhone), ComparisonID::kLike, C("1%"))});
    EXPECT_EQ(statusOf([&]() {
                QueryContext ctx;
                AggregationStateSpec spec;
                spec.input_relation = &rel;
                spec.aggregates = {AggregateSpec(AggregationID::kSum, Scalar::Case({{like, Scalar::Literal(1.0)}}, Scalar::Literal(0.0)))};
                spec.strategy = QSX_AGG_SINGLE_STATE;
                ctx.addAggregationState(spec);
              }, &message), unsupported);
    EXPECT_TRUE(says(message, {"LIKE", "unary"}));
  }
  {  // a join's residual predicate
    CatalogRelation result(2, "result");
    result.addAttribute("id", Type::Int());
    QueryContext ctx;
    const auto table = ctx.addJoinHashTable(kInt, 16, 1);
    const auto dest = ctx.addInsertDestination(&result, &storage);
    const auto selection = ctx.addScalarGroup({kId});
    const auto residual = ctx.addPredicate(Where({ComparisonPredicate::OnScalar(Year(kDate), ComparisonID::kEqual, I(1995))}));
    const std::vector<bool> on_build = {false};
    BuildHashOperator builder(0, rel, true, {kId}, false, 1, table);
    fetchAndExecuteWorkOrders(&builder, &ctx, &storage);
    HashJoinOperator prober(0, rel, rel, true, {kId}, false, 1, false, result, dest, table, residual, selection, &on_build,
                            HashJoinOperator::JoinType::kInnerJoin);
    EXPECT_EQ(statusOf([&]() { fetchAndExecuteWorkOrders(&prober, &ctx, &storage); }, &message), unsupported);
    EXPECT_TRUE(says(message, {"residual", "scalar operand"}));
    DestroyHashOperator cleaner(0, 1, table);
    fetchAndExecuteWorkOrders(&cleaner, &ctx, &storage);
  }
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "unary_predicate_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Customers t;
  for (const bool compressed : {false, true}) {
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      runSelects(t, compressed, per_order);
      runAggregation(t, compressed, per_order);
    }
  }
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) runAdoptedImages(t, per_order);
  runRefusals(t);
  return finish("unary_predicate_operator_test");
}
