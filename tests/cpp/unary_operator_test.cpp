// Scalar::kUnaryExpression through the operators: a Select projecting EXTRACT(YEAR), EXTRACT(MONTH), SUBSTRING(phone, 0, 2) and
// EXTRACT(YEAR) * 100 + EXTRACT(MONTH) under a predicate, over a nullable date whose NULLs must arrive in the output bitmaps;
// Q8's shape — SUM(CASE ..), SUM(volume) GROUP BY EXTRACT(YEAR FROM o_orderdate) through group_by_scalars — per block, over a
// run (which must stay on the run path) and as Select -> Aggregation on the projected attribute, also with the date
// dictionary-compressed (extracted from the dictionary, the dates never decoded) and under COLLISION_FREE; Q22's shape —
// COUNT(*), SUM(c_acctbal) GROUP BY SUBSTRING(c_phone, 0, 2) over CHAR(15), packed for m = 2 and interned for m = 3; NULL
// operands as NULL keys; and the refusals.  Expected results are computed here on the host columns.
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kId = 0, kDate, kNullableDate, kVolume, kNation, kPhone, kNullablePhone, kBal };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};
const char *const kNations[] = {"BRAZIL", "ARGENTINA", "CANADA", "PERU", "UNITED STATES"};

struct Orders {
  std::vector<std::int32_t> id;
  std::vector<DateLit> date;
  std::vector<double> volume, bal;
  std::vector<char> nation, phone;   // CHAR(25), CHAR(15)
  std::vector<bool> date_null, phone_null;
  std::size_t n = 0;
  Orders() {
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (std::int64_t b : kBlockSizes) n += static_cast<std::size_t>(b);
    nation.assign(n * 25, 0);
    phone.assign(n * 15, 0);
    for (std::size_t r = 0; r < n; ++r) {
      id.push_back(static_cast<std::int32_t>(r));
      date.push_back(DateLit::Create(1992 + static_cast<std::int32_t>(rnd() % 7), static_cast<std::uint8_t>(1 + rnd() % 12),
                                     static_cast<std::uint8_t>(1 + 7 * (rnd() % 4))));   // 336 dates: every block's dictionary pays, 2-byte codes
      volume.push_back(static_cast<double>(rnd() % 100000 + 1));   // integers: every sum exact in any order
      bal.push_back(static_cast<double>(static_cast<std::int64_t>(rnd() % 20000) - 10000));
      std::strncpy(&nation[r * 25], kNations[rnd() % 5], 25);
      // "CC-ddd-ddd-dddd": 25 country codes 10..34, the text fills all 15 bytes; every 16th phone ends behind its country code,
      // with the rest of the field left as it was (bytes behind the NUL never take part)
      char text[32] = {};
      std::snprintf(text, sizeof(text), "%02d-%03d-%03d-%04d", static_cast<int>(10 + rnd() % 25), static_cast<int>(rnd() % 1000),
                    static_cast<int>(rnd() % 1000), static_cast<int>(rnd() % 10000));
      if (r % 16 == 5) text[2] = 0;
      std::memcpy(&phone[r * 15], text, 15);
      date_null.push_back(rnd() % 5 == 0);
      phone_null.push_back(rnd() % 7 == 0);
    }
  }
  bool brazil(std::size_t r) const { return std::strncmp(&nation[r * 25], "BRAZIL", 25) == 0; }
  std::string phonePrefix(std::size_t r, std::size_t m) const {
    const std::size_t len = ::strnlen(&phone[r * 15], 15);
    return std::string(&phone[r * 15], std::min(len, m));
  }
};

void load(const Orders &t, CatalogRelation *rel, StorageManager *storage, bool compress_date = false) {
  rel->addAttribute("id", Type::Int());
  rel->addAttribute("o_orderdate", Type::Date());
  rel->addAttribute("o_commitdate", Type::Date().getNullableVersion());
  rel->addAttribute("volume", Type::Double());
  rel->addAttribute("nation", Type::Char(25));
  rel->addAttribute("c_phone", Type::Char(15));
  rel->addAttribute("c_fax", Type::Char(15).getNullableVersion());
  rel->addAttribute("c_acctbal", Type::Double());
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    std::vector<std::uint64_t> date_nulls(static_cast<std::size_t>(n) / 64 + 2, 0), phone_nulls(static_cast<std::size_t>(n) / 64 + 2, 0);
    for (std::size_t r = 0; r < static_cast<std::size_t>(n); ++r) {
      if (t.date_null[at + r]) date_nulls[r / 64] |= 1ull << (63 - r % 64);
      if (t.phone_null[at + r]) phone_nulls[r / 64] |= 1ull << (63 - r % 64);
    }
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, n > 0 ? date_nulls.data() : nullptr, nullptr, nullptr, nullptr,
                                                        n > 0 ? phone_nulls.data() : nullptr, nullptr};
    const std::vector<bool> compress = {false, compress_date && n > 0, false, false, false, false, false, false};
    storage->loadBlock(rel, {t.id.data() + at, t.date.data() + at, t.date.data() + at, t.volume.data() + at, t.nation.data() + at * 25,
                             t.phone.data() + at * 15, t.phone.data() + at * 15, t.bal.data() + at}, n, 0, &compress, &bitmaps);
    at += static_cast<std::size_t>(n);
  }
}

Predicate Where(std::initializer_list<ComparisonPredicate> terms) { Predicate p; p.conjuncts = terms; return p; }
ScalarPtr Year(attribute_id a) { return Scalar::DateExtract(QSX_DATE_YEAR, Scalar::Attribute(a)); }
ScalarPtr Month(attribute_id a) { return Scalar::DateExtract(QSX_DATE_MONTH, Scalar::Attribute(a)); }
ScalarPtr BrazilVolume(attribute_id nation, attribute_id volume) {
  return Scalar::Case({{Where({{nation, ComparisonID::kEqual, TypedLiteral::Char("BRAZIL")}}), Scalar::Attribute(volume)}}, Scalar::Literal(0.0));
}

template <typename T>
std::vector<T> column(StorageManager *storage, const std::vector<block_id> &blocks, attribute_id a, std::vector<bool> *is_null = nullptr,
                      std::size_t width = sizeof(T)) {
  std::vector<T> v;
  for (block_id b : blocks) {
    BlockReference blk = storage->getBlock(b);
    const std::size_t at = v.size(), k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    v.resize(at + k * (width / sizeof(T)));
    blk->copyAttributeToHost(a, v.data() + at);
    if (is_null != nullptr) {
      std::vector<std::uint64_t> nulls((k + 63) / 64 + 1, 0);
      blk->copyNullBitmapToHost(a, nulls.data());
      for (std::size_t r = 0; r < k; ++r) is_null->push_back((nulls[r >> 6] >> (63 - (r & 63))) & 1u);
    }
  }
  return v;
}

// select id, extract(year from o_commitdate), extract(month from o_commitdate), substring(c_phone from 1 for 2),
//        extract(year from o_commitdate) * 100 + extract(month from o_commitdate), substring(c_fax from 4 for 300) from t where volume >= 20000
void runSelect(const Orders &t, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), out(2, "out");
  StorageManager storage;
  load(t, &rel, &storage);
  out.addAttribute("id", Type::Int());
  out.addAttribute("o_year", Type::Int().getNullableVersion());
  out.addAttribute("o_month", Type::Int().getNullableVersion());
  out.addAttribute("cntrycode", Type::Char(2));
  out.addAttribute("yyyymm", Type::Int().getNullableVersion());
  out.addAttribute("fax_tail", Type::Char(12).getNullableVersion());
  QueryContext ctx;
  const auto pred = ctx.addPredicate(Where({{kVolume, ComparisonID::kGreaterOrEqual, TypedLiteral::Double(20000.0)}}));
  const auto dest = ctx.addInsertDestination(&out, &storage);
  const ScalarPtr yyyymm = Scalar::Binary(BinaryOperationID::kAdd, Scalar::Binary(BinaryOperationID::kMultiply, Year(kNullableDate), Scalar::IntLiteral(100)),
                                          Month(kNullableDate));
  SelectOperator select(0, rel, false, out, dest, pred,
                        std::vector<ScalarPtr>{Scalar::Attribute(kId), Year(kNullableDate), Month(kNullableDate),
                                               Scalar::Substring(0, 2, Scalar::Attribute(kPhone)), yyyymm,
                                               Scalar::Substring(3, 300, Scalar::Attribute(kNullablePhone))}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &storage);
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  std::vector<bool> year_null, month_null, digits_null, fax_null;
  const std::vector<std::int32_t> ids = column<std::int32_t>(&storage, blocks, 0);
  const std::vector<std::int32_t> years = column<std::int32_t>(&storage, blocks, 1, &year_null);
  const std::vector<std::int32_t> months = column<std::int32_t>(&storage, blocks, 2, &month_null);
  const std::vector<char> codes = column<char>(&storage, blocks, 3, nullptr, 2);
  const std::vector<std::int32_t> digits = column<std::int32_t>(&storage, blocks, 4, &digits_null);
  const std::vector<char> fax = column<char>(&storage, blocks, 5, &fax_null, 12);
  std::size_t want_rows = 0, nulls_seen = 0, values_seen = 0, short_seen = 0;
  for (std::size_t r = 0; r < t.n; ++r) want_rows += t.volume[r] >= 20000.0;
  EXPECT_EQ(ids.size(), want_rows);
  EXPECT_EQ(codes.size(), want_rows * 2);
  EXPECT_EQ(fax.size(), want_rows * 12);
  std::vector<bool> seen(t.n, false);
  for (std::size_t k = 0; k < ids.size() && codes.size() == want_rows * 2 && fax.size() == want_rows * 12; ++k) {
    const std::size_t r = static_cast<std::size_t>(ids[k]);
    EXPECT_TRUE(r < t.n && !seen[r] && t.volume[r] >= 20000.0);
    if (r >= t.n) continue;
    seen[r] = true;
    char want_code[2] = {0, 0}, want_fax[12] = {};
    const std::string prefix = t.phonePrefix(r, 2);
    std::memcpy(want_code, prefix.data(), prefix.size());
    EXPECT_TRUE(std::memcmp(&codes[k * 2], want_code, 2) == 0);                    // zero-filled to m
    short_seen += prefix.size() < 2 || ::strnlen(&t.phone[r * 15], 15) < 15;
    EXPECT_EQ(static_cast<bool>(fax_null[k]), static_cast<bool>(t.phone_null[r]));
    if (!t.phone_null[r]) {
      const std::size_t len = ::strnlen(&t.phone[r * 15], 15);
      if (len > 3) std::memcpy(want_fax, &t.phone[r * 15 + 3], len - 3);
      EXPECT_TRUE(std::memcmp(&fax[k * 12], want_fax, 12) == 0);
    }
    EXPECT_EQ(static_cast<bool>(year_null[k]), static_cast<bool>(t.date_null[r]));
    EXPECT_EQ(static_cast<bool>(month_null[k]), static_cast<bool>(t.date_null[r]));
    EXPECT_EQ(static_cast<bool>(digits_null[k]), static_cast<bool>(t.date_null[r]));
    if (t.date_null[r]) { ++nulls_seen; continue; }
    ++values_seen;
    EXPECT_EQ(years[k], t.date[r].year);
    EXPECT_EQ(months[k], static_cast<std::int32_t>(t.date[r].month));
    EXPECT_EQ(digits[k], t.date[r].year * 100 + t.date[r].month);
  }
  EXPECT_TRUE(nulls_seen > 100 && values_seen > 100 && short_seen > 100);
}

struct YearSums { double brazil = 0.0, all = 0.0; };
std::map<std::int32_t, YearSums> readYearSums(StorageManager *storage, const std::vector<block_id> &blocks) {
  const std::vector<std::int32_t> years = column<std::int32_t>(storage, blocks, 0);
  const std::vector<double> brazil = column<double>(storage, blocks, 1), all = column<double>(storage, blocks, 2);
  std::map<std::int32_t, YearSums> got;
  EXPECT_TRUE(years.size() == brazil.size() && years.size() == all.size());
  for (std::size_t k = 0; k < years.size() && k < brazil.size() && k < all.size(); ++k) {
    EXPECT_TRUE(got.count(years[k]) == 0);
    got[years[k]] = YearSums{brazil[k], all[k]};
  }
  return got;
}
bool sameSums(const std::map<std::int32_t, YearSums> &a, const std::map<std::int32_t, YearSums> &b) {
  if (a.size() != b.size()) return false;
  for (const auto &kv : a) {
    const auto it = b.find(kv.first);
    if (it == b.end() || it->second.brazil != kv.second.brazil || it->second.all != kv.second.all) return false;
  }
  return true;
}

// select extract(year from o_orderdate) as o_year, sum(case when nation = 'BRAZIL' then volume else 0 end), sum(volume)
// from t group by o_year
void runQ8(const Orders &t, std::size_t blocks_per_order, bool compress_date, qsx_agg_strategy_t strategy) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage, compress_date);
  result.addAttribute("o_year", Type::Int());
  result.addAttribute("brazil", Type::Double());
  result.addAttribute("all", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by = {kId};                      // (replaced by group_by_scalars)
  spec.group_by_scalars = {Year(kDate)};
  spec.aggregates = {AggregateSpec(AggregationID::kSum, BrazilVolume(kNation, kVolume)), AggregateSpec(AggregationID::kSum, kVolume)};
  spec.strategy = strategy;
  spec.estimated_num_groups = 16;
  spec.collision_free_num_entries = 1999;     // max year + 1
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::map<std::int32_t, YearSums> want;
  for (std::size_t r = 0; r < t.n; ++r) {
    YearSums &w = want[t.date[r].year];
    w.all += t.volume[r];
    if (t.brazil(r)) w.brazil += t.volume[r];
  }
  EXPECT_EQ(want.size(), std::size_t(7));
  EXPECT_TRUE(sameSums(readYearSums(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks()), want));
  AggregationOperationState *st = ctx.getAggregationState(state);
  // the run leg stays on the run path: its four non-empty blocks in one update, keys and CASE by the run forms
  if (blocks_per_order > 1) {
    EXPECT_EQ(st->numBlocksWithUnaryKeysEvaluatedInRuns(), std::int64_t(4));
    EXPECT_EQ(st->numBlocksWithCaseEvaluatedInRuns(), std::int64_t(4));
  } else {
    EXPECT_EQ(st->numBlocksWithUnaryKeysEvaluatedInRuns(), std::int64_t(0));
  }
  // a dictionary-compressed date is extracted from its dictionary: counted, and the 8-byte dates never decoded
  EXPECT_EQ(st->numBlocksWithDateExtractOnCodes(), compress_date ? std::int64_t(4) : std::int64_t(0));
  if (compress_date) {
    for (block_id b : rel.getBlocksInPartition(0)) {
      BlockReference blk = storage.getBlock(b);
      if (blk->numTuples() == 0) continue;
      EXPECT_TRUE(blk->compressedAttribute(kDate) != nullptr);
      EXPECT_TRUE(!blk->valuesMaterialized(kDate));
    }
  }
}

// the same as Select -> Aggregation: the Select projects (o_year, nation, volume), the aggregation groups by the attribute
void runQ8ThroughSelect(const Orders &t) {
  CatalogRelation rel(1, "t"), projected(2, "projected"), result(3, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  projected.addAttribute("o_year", Type::Int());
  projected.addAttribute("nation", Type::Char(25));
  projected.addAttribute("volume", Type::Double());
  result.addAttribute("o_year", Type::Int());
  result.addAttribute("brazil", Type::Double());
  result.addAttribute("all", Type::Double());
  QueryContext ctx;
  const auto select_dest = ctx.addInsertDestination(&projected, &storage);
  const auto dest = ctx.addInsertDestination(&result, &storage);
  SelectOperator select(0, rel, false, projected, select_dest, QueryContext::kInvalidPredicateId,
                        std::vector<ScalarPtr>{Year(kDate), Scalar::Attribute(kNation), Scalar::Attribute(kVolume)}, true);
  fetchAndExecuteWorkOrders(&select, &ctx, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &projected;
  spec.group_by = {0};
  spec.aggregates = {AggregateSpec(AggregationID::kSum, BrazilVolume(1, 2)), AggregateSpec(AggregationID::kSum, 2)};
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 16;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(1, projected, true, state);
  FinalizeAggregationOperator finalize(1, state, 1, false, 1, result, dest);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::map<std::int32_t, YearSums> want;
  for (std::size_t r = 0; r < t.n; ++r) {
    YearSums &w = want[t.date[r].year];
    w.all += t.volume[r];
    if (t.brazil(r)) w.brazil += t.volume[r];
  }
  EXPECT_TRUE(sameSums(readYearSums(&storage, ctx.getInsertDestination(dest)->getTouchedBlocks()), want));
}

// select substring(c_phone from 1 for m) as cntrycode, count(*), sum(c_acctbal) from t group by cntrycode
// m = 2: CHAR(2), packed; m = 3: CHAR(3), interned.  nullable: over c_fax, whose NULL rows are kept out like a NULL attribute key's.
void runQ22(const Orders &t, std::size_t blocks_per_order, int m, bool nullable) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  Type code_type = Type::Char(m);
  if (nullable) code_type = code_type.getNullableVersion();
  result.addAttribute("cntrycode", code_type);
  result.addAttribute("numcust", Type::Long());
  result.addAttribute("totacctbal", Type::Double());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by_scalars = {Scalar::Substring(0, m, Scalar::Attribute(nullable ? kNullablePhone : kPhone))};
  spec.aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID), AggregateSpec(AggregationID::kSum, kBal)};
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 64;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::map<std::string, std::pair<std::int64_t, double>> want, got;
  for (std::size_t r = 0; r < t.n; ++r) {
    if (nullable && t.phone_null[r]) continue;      // a NULL key is in no group (PackedPayloadHashTable.hpp:861-867)
    auto &w = want[t.phonePrefix(r, static_cast<std::size_t>(m))];
    w.first += 1;
    w.second += t.bal[r];
  }
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  const std::vector<std::int64_t> count = column<std::int64_t>(&storage, blocks, 1);
  const std::vector<double> sum = column<double>(&storage, blocks, 2);
  const std::vector<char> codes = column<char>(&storage, blocks, 0, nullptr, static_cast<std::size_t>(m));
  EXPECT_EQ(codes.size(), count.size() * static_cast<std::size_t>(m));
  for (std::size_t k = 0; k < count.size() && codes.size() == count.size() * static_cast<std::size_t>(m); ++k) {
    const std::string code(&codes[k * m], ::strnlen(&codes[k * m], static_cast<std::size_t>(m)));
    EXPECT_TRUE(got.count(code) == 0);
    got[code] = {count[k], sum[k]};
  }
  EXPECT_TRUE(want.size() >= std::size_t(25));      // 25 country codes (m = 3: "CC-"), and the short phones' "CC"
  EXPECT_TRUE(got == want);
  AggregationOperationState *st = ctx.getAggregationState(state);
  // a key over a nullable operand carries the operand's null bitmaps, which travel with single-block calls
  EXPECT_EQ(st->numBlocksWithUnaryKeysEvaluatedInRuns(), blocks_per_order > 1 && !nullable ? std::int64_t(4) : std::int64_t(0));
}

// select extract(month from o_commitdate), count(*) from t group by 1: the NULL dates are in no group
void runNullKeys(const Orders &t, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "t"), result(2, "result");
  StorageManager storage;
  load(t, &rel, &storage);
  result.addAttribute("o_month", Type::Int().getNullableVersion());
  result.addAttribute("orders", Type::Long());
  QueryContext ctx;
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by_scalars = {Month(kNullableDate)};
  spec.aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 16;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  // the reference for "treated as a NULL attribute key is": the same grouping by a nullable INT attribute holding the months
  std::map<std::int32_t, std::int64_t> want, got;
  for (std::size_t r = 0; r < t.n; ++r) if (!t.date_null[r]) want[t.date[r].month] += 1;
  const std::vector<block_id> blocks = ctx.getInsertDestination(dest)->getTouchedBlocks();
  const std::vector<std::int32_t> months = column<std::int32_t>(&storage, blocks, 0);
  const std::vector<std::int64_t> orders = column<std::int64_t>(&storage, blocks, 1);
  for (std::size_t k = 0; k < months.size() && k < orders.size(); ++k) got[months[k]] = orders[k];
  EXPECT_EQ(want.size(), std::size_t(12));
  EXPECT_TRUE(got == want);
}

int statusOf(const std::function<void()> &body) {
  try {
    body();
  } catch (const ExecutionError &e) {
    return e.status();
  }
  return QSX_OK;
}

void runRefusals(const Orders &t) {
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
  const auto aggregate = [&](const std::function<void(AggregationStateSpec *)> &fill) {
    return statusOf([&]() {
      CatalogRelation rel(1, "t");
      StorageManager storage;
      load(t, &rel, &storage);
      QueryContext ctx;
      AggregationStateSpec spec;
      spec.input_relation = &rel;
      spec.strategy = QSX_AGG_COMPACT_KEY;
      fill(&spec);
      ctx.addAggregationState(spec);
    });
  };
  const int unsupported = static_cast<int>(QSX_ERR_UNSUPPORTED), invalid = static_cast<int>(QSX_ERR_INVALID_ARGUMENT);
  const Predicate big = Where({{kVolume, ComparisonID::kGreaterOrEqual, TypedLiteral::Double(20000.0)}});
  EXPECT_EQ(select(Year(kDate), Type::Int()), static_cast<int>(QSX_OK));
  EXPECT_EQ(select(Scalar::Substring(0, 2, Scalar::Attribute(kPhone)), Type::Char(2)), static_cast<int>(QSX_OK));
  // anything but an attribute of the right type as the operand: a literal, an expression, a CASE, another unary, the wrong type
  EXPECT_EQ(select(Scalar::DateExtract(QSX_DATE_YEAR, Scalar::IntLiteral(1995)), Type::Int()), unsupported);
  EXPECT_EQ(select(Scalar::DateExtract(QSX_DATE_YEAR, Scalar::Binary(BinaryOperationID::kAdd, Scalar::Attribute(kId), Scalar::IntLiteral(1))), Type::Int()),
            unsupported);
  EXPECT_EQ(select(Scalar::DateExtract(QSX_DATE_YEAR, Scalar::Case({{big, Scalar::Attribute(kId)}}, Scalar::IntLiteral(0))), Type::Int()), unsupported);
  EXPECT_EQ(select(Scalar::DateExtract(QSX_DATE_YEAR, Year(kDate)), Type::Int()), unsupported);
  EXPECT_EQ(select(Scalar::Substring(0, 2, Scalar::Substring(0, 4, Scalar::Attribute(kPhone))), Type::Char(2)), unsupported);
  EXPECT_EQ(select(Scalar::Substring(0, 2, Scalar::Attribute(kDate)), Type::Char(2)), unsupported);
  EXPECT_EQ(select(Year(kPhone), Type::Int()), unsupported);
  // DAY / HOUR / MINUTE / SECOND belong to Datetime
  EXPECT_EQ(select(Scalar::DateExtract(2, Scalar::Attribute(kDate)), Type::Int()), unsupported);
  // a unary inside a CASE branch or WHEN's result, SUBSTRING inside arithmetic
  EXPECT_EQ(select(Scalar::Case({{big, Year(kDate)}}, Scalar::IntLiteral(0)), Type::Int()), unsupported);
  EXPECT_EQ(select(Scalar::Case({{big, Scalar::IntLiteral(0)}}, Month(kDate)), Type::Int()), unsupported);
  EXPECT_EQ(select(Scalar::Case({{big, Scalar::Substring(0, 2, Scalar::Attribute(kPhone))}}, nullptr), Type::Char(2).getNullableVersion()), unsupported);
  EXPECT_EQ(select(Scalar::Binary(BinaryOperationID::kAdd, Scalar::Substring(0, 2, Scalar::Attribute(kPhone)), Scalar::IntLiteral(1)), Type::Int()),
            unsupported);
  // a window the operation does not have, an output attribute of another type or not nullable
  EXPECT_EQ(select(Scalar::Substring(15, 2, Scalar::Attribute(kPhone)), Type::Char(2)), invalid);
  EXPECT_EQ(select(Scalar::Substring(-1, 2, Scalar::Attribute(kPhone)), Type::Char(2)), invalid);
  EXPECT_EQ(select(Scalar::Substring(0, 0, Scalar::Attribute(kPhone)), Type::Char(2)), invalid);
  EXPECT_EQ(select(Scalar::Substring(0, 2, Scalar::Attribute(kPhone)), Type::Char(3)), invalid);
  EXPECT_EQ(select(Year(kDate), Type::Long()), invalid);
  EXPECT_EQ(select(Year(kNullableDate), Type::Int()), invalid);
  // a unary as an aggregate's argument, also under arithmetic; DISTINCT beside a unary key; a key that is neither
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) { spec->aggregates = {AggregateSpec(AggregationID::kMax, Year(kDate))}; }), unsupported);
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) {
    spec->aggregates = {AggregateSpec(AggregationID::kSum, Scalar::Binary(BinaryOperationID::kAdd, Year(kDate), Scalar::IntLiteral(1)))};
  }), unsupported);
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) {
    spec->group_by_scalars = {Year(kDate)};
    spec->aggregates = {AggregateSpec(AggregationID::kCount, kId, true)};
  }), unsupported);
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) {
    spec->group_by_scalars = {Scalar::Binary(BinaryOperationID::kAdd, Scalar::Attribute(kId), Scalar::IntLiteral(1))};
    spec->aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  }), unsupported);
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) {
    spec->group_by_scalars = {Scalar::DateExtract(QSX_DATE_YEAR, Scalar::IntLiteral(7))};
    spec->aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  }), unsupported);
  // group_by_scalars of attributes only is the plain form
  EXPECT_EQ(aggregate([](AggregationStateSpec *spec) {
    spec->group_by_scalars = {Scalar::Attribute(kId)};
    spec->aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  }), static_cast<int>(QSX_OK));
  // a state with a unary key is not exchanged across ranks: refused in front of the first collective
  EXPECT_EQ(statusOf([&]() {
    CatalogRelation rel(1, "t");
    StorageManager storage;
    load(t, &rel, &storage);
    AggregationStateSpec spec;
    spec.input_relation = &rel;
    spec.strategy = QSX_AGG_COMPACT_KEY;
    spec.group_by_scalars = {Year(kDate)};
    spec.aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
    AggregationOperationState state(spec);
    state.mergeAcrossRanks(nullptr);
  }), unsupported);
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "unary_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Orders t;
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    runSelect(t, per_order);
    runQ8(t, per_order, false, QSX_AGG_COMPACT_KEY);
    runQ8(t, per_order, true, QSX_AGG_COMPACT_KEY);
    runQ8(t, per_order, false, QSX_AGG_COLLISION_FREE);
    runQ22(t, per_order, 2, false);
    runQ22(t, per_order, 3, false);
    runQ22(t, per_order, 2, true);
    runQ22(t, per_order, 3, true);
    runNullKeys(t, per_order);
  }
  runQ8ThroughSelect(t);
  runRefusals(t);
  return finish("unary_operator_test");
}
