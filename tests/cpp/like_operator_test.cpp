// LIKE / NOT LIKE terms (ComparisonID::kLike / kNotLike) through the operators: SelectOperator over plain CHAR(25) blocks,
// over dictionary-coded blocks (the pattern against every block's dictionary, then code membership: the values are never
// decoded), on a nullable attribute (a NULL is in neither result) and on the coded attribute as sort column; per block and
// over runs, with an empty block and block sizes that are no multiples of 64, alone and conjoined with a numeric term on
// either side.  Then Q14's shape — an aggregation whose predicate holds p_type LIKE 'PROMO%' — a join with a LIKE residual on
// a build-side attribute, and the uses that are refused.  The checker is a plain recursive matcher on the host columns.
#include <algorithm>
#include <cstring>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kPartkey = 0, kType, kName, kSize };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};

bool Like(const char *t, std::size_t tn, const char *p, std::size_t pn) {
  if (pn == 0) return tn == 0;
  if (*p == '%') return Like(t, tn, p + 1, pn - 1) || (tn > 0 && Like(t + 1, tn - 1, p, pn));
  return tn > 0 && (*p == '_' || *p == *t) && Like(t + 1, tn - 1, p + 1, pn - 1);
}
bool LikeField(const char *field, int width, const std::string &pattern) {
  return Like(field, ::strnlen(field, static_cast<std::size_t>(width)), pattern.data(), pattern.size());
}

struct Part {
  std::vector<std::int32_t> partkey, size;
  std::vector<char> type, name;   // CHAR(25) each
  std::vector<bool> name_null;
  std::vector<double> price;
  explicit Part(bool sorted_on_type) {
    const char *a[] = {"STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO"};
    const char *b[] = {"ANODIZED", "BURNISHED", "PLATED", "POLISHED", "BRUSHED"};
    const char *c[] = {"TIN", "NICKEL", "BRASS", "STEEL", "COPPER"};
    const char *colors[] = {"green", "blue", "forest", "red", "almond", "lime", "greenish"};
    std::uint64_t x = 0x2545F4914F6CDD1Dull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::int64_t total = 0;
    for (std::int64_t n : kBlockSizes) total += n;
    std::vector<std::string> types;
    for (std::int64_t i = 0; i < total; ++i) {
      types.push_back(std::string(a[rnd() % 6]) + " " + b[rnd() % 5] + " " + c[rnd() % 5]);   // up to 25 bytes: no terminator then
    }
    if (sorted_on_type) {   // every block sorted on its own
      std::int64_t at = 0;
      for (std::int64_t n : kBlockSizes) {
        std::sort(types.begin() + at, types.begin() + at + n);
        at += n;
      }
    }
    type.assign(static_cast<std::size_t>(total) * 25, 0);
    name.assign(static_cast<std::size_t>(total) * 25, 0);
    for (std::int64_t i = 0; i < total; ++i) {
      partkey.push_back(static_cast<std::int32_t>(i));
      size.push_back(static_cast<std::int32_t>(rnd() % 5));
      price.push_back(static_cast<double>(rnd() % 100000));
      char *t = &type[static_cast<std::size_t>(i) * 25], *nm = &name[static_cast<std::size_t>(i) * 25];
      for (int k = 0; k < 25; ++k) t[k] = nm[k] = static_cast<char>('!' + rnd() % 90);   // what lies behind a NUL is never looked at
      std::memcpy(t, types[i].data(), types[i].size());
      if (types[i].size() < 25) t[types[i].size()] = '\0';
      const std::string words = std::string(colors[rnd() % 7]) + " " + colors[rnd() % 7];
      std::memcpy(nm, words.data(), words.size());
      nm[words.size()] = '\0';
      name_null.push_back(rnd() % 4 == 0);
    }
  }
};

std::vector<std::uint64_t> packBits(const std::vector<bool> &bits, std::size_t from, std::size_t n) {
  std::vector<std::uint64_t> words(n / 64 + 2, 0);
  for (std::size_t i = 0; i < n; ++i) {
    if (bits[from + i]) words[i / 64] |= 1ull << (63 - i % 64);
  }
  return words;
}

void load(const Part &part, CatalogRelation *rel, StorageManager *storage, bool compressed, bool sorted_on_type) {
  rel->addAttribute("p_partkey", Type::Int());
  rel->addAttribute("p_type", Type::Char(25));
  rel->addAttribute("p_name", Type::Char(25).getNullableVersion());
  rel->addAttribute("p_size", Type::Int());
  const std::vector<bool> compress = {false, true, false, false};
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    const std::vector<std::uint64_t> nulls = packBits(part.name_null, at, static_cast<std::size_t>(n));
    const std::vector<const std::uint64_t *> bitmaps = {nullptr, nullptr, n > 0 ? nulls.data() : nullptr, nullptr};
    const block_id id = storage->loadBlock(rel, {part.partkey.data() + at, part.type.data() + at * 25, part.name.data() + at * 25, part.size.data() + at},
                                           n, 0, compressed ? &compress : nullptr, &bitmaps);
    if (sorted_on_type) storage->getBlock(id)->setSortColumn(kType);
    at += static_cast<std::size_t>(n);
  }
  if (compressed) {
    const CompressedAttribute *c = storage->getBlock(rel->getBlocksSnapshot().front())->compressedAttribute(kType);
    EXPECT_TRUE(c != nullptr && c->kind == CompressedAttribute::kDictionary && c->code_width == 1 && c->value_width == 25);
  }
}

bool RowPasses(const Part &part, std::size_t i, const Predicate &pred) {
  for (const ComparisonPredicate &term : pred.conjuncts) {
    if (term.attribute == kSize) {
      const std::int32_t v = part.size[i], lit = term.literal.v.i32;
      if (!(term.comparison == ComparisonID::kLess ? v < lit : v >= lit)) return false;
      continue;
    }
    if (term.attribute == kName && part.name_null[i]) return false;   // a NULL matches neither LIKE nor NOT LIKE
    const char *field = term.attribute == kType ? &part.type[i * 25] : &part.name[i * 25];
    if (LikeField(field, 25, term.literal.text) != (term.comparison == ComparisonID::kLike)) return false;
  }
  return true;
}

void runSelect(const Part &part, const Predicate &pred, bool compressed, bool sorted_on_type, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "part"), out(2, "out");
  StorageManager storage;
  load(part, &rel, &storage, compressed, sorted_on_type);
  out.addAttribute("p_partkey", Type::Int());
  QueryContext ctx;
  const auto pred_id = ctx.addPredicate(pred);
  const auto dest = ctx.addInsertDestination(&out, &storage);
  SelectOperator select(0, rel, false, out, dest, pred_id, std::vector<attribute_id>{kPartkey}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &storage);
  std::vector<std::int32_t> got, want;
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = storage.getBlock(b);
    const std::size_t at = got.size(), k = static_cast<std::size_t>(blk->numTuples());
    got.resize(at + k);
    if (k > 0) blk->copyAttributeToHost(0, got.data() + at);
  }
  for (std::size_t i = 0; i < part.partkey.size(); ++i) {
    if (RowPasses(part, i, pred)) want.push_back(part.partkey[i]);
  }
  std::sort(got.begin(), got.end());
  EXPECT_TRUE(!want.empty() && want.size() < part.partkey.size());   // a predicate that keeps nothing or everything shows nothing
  EXPECT_EQ(got.size(), want.size());
  EXPECT_TRUE(got == want);
  if (compressed) {   // the pattern met the dictionaries, the rows only their codes
    // (an empty block is never compressed: it keeps the plain, empty stripe it was created with)
    for (block_id b : rel.getBlocksSnapshot()) {
      BlockReference blk = storage.getBlock(b);
      if (blk->numTuples() == 0) continue;
      EXPECT_TRUE(blk->compressedAttribute(kType) != nullptr);
      if (blk->valuesMaterialized(kType)) std::fprintf(stderr, "p_type of a block of %lld tuples was decoded\n", static_cast<long long>(blk->numTuples()));
      EXPECT_TRUE(!blk->valuesMaterialized(kType));
    }
  }
}

// select p_size, sum(price), count(*) from part where p_type like 'PROMO%' [and p_size >= 1] group by p_size — Q14's filter inside
// the aggregation state
void runAggregation(const Part &part, bool compressed, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "part"), result(2, "result");
  StorageManager storage;
  rel.addAttribute("p_type", Type::Char(25));
  rel.addAttribute("p_size", Type::Int());
  rel.addAttribute("p_price", Type::Double());
  const std::vector<bool> compress = {true, false, false};
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    storage.loadBlock(&rel, {part.type.data() + at * 25, part.size.data() + at, part.price.data() + at}, n, 0, compressed ? &compress : nullptr);
    at += static_cast<std::size_t>(n);
  }
  result.addAttribute("p_size", Type::Int());
  result.addAttribute("sum_price", Type::Double());
  result.addAttribute("count", Type::Long());
  QueryContext ctx;
  Predicate pred;
  pred.conjuncts.push_back({0, ComparisonID::kLike, TypedLiteral::Char("PROMO%")});
  pred.conjuncts.push_back({1, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(1)});
  const auto dest = ctx.addInsertDestination(&result, &storage);
  AggregationStateSpec spec;
  spec.input_relation = &rel;
  spec.group_by = {1};
  spec.aggregates = {AggregateSpec(AggregationID::kSum, 2), AggregateSpec(AggregationID::kCount, kInvalidAttributeID)};
  spec.predicate = ctx.getPredicate(ctx.addPredicate(pred));
  spec.strategy = QSX_AGG_COMPACT_KEY;
  spec.estimated_num_groups = 8;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &storage);
  std::vector<double> want_sum(5, 0.0), got_sum(5, 0.0);
  std::vector<std::int64_t> want_count(5, 0), got_count(5, 0);
  for (std::size_t i = 0; i < part.partkey.size(); ++i) {
    if (part.size[i] >= 1 && LikeField(&part.type[i * 25], 25, "PROMO%")) {
      want_sum[part.size[i]] += part.price[i];
      ++want_count[part.size[i]];
    }
  }
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    std::vector<std::int32_t> key(k);
    std::vector<double> sum(k);
    std::vector<std::int64_t> cnt(k);
    blk->copyAttributeToHost(0, key.data());
    blk->copyAttributeToHost(1, sum.data());
    blk->copyAttributeToHost(2, cnt.data());
    for (std::size_t i = 0; i < k; ++i) {
      got_sum[key[i]] = sum[i];
      got_count[key[i]] = cnt[i];
    }
  }
  EXPECT_TRUE(want_count[1] > 0 && want_count[0] == 0);
  EXPECT_TRUE(got_count == want_count);
  EXPECT_TRUE(got_sum == want_sum);   // integer-valued doubles below 2^53: exact in any order
}

// select l_partkey, l_qty from part join lineitem on p_partkey = l_partkey where p_type [not] like '%BRASS'
void runJoin(const Part &part, ComparisonID comparison, std::size_t blocks_per_order) {
  CatalogRelation build(1, "part"), probe(2, "lineitem"), out(3, "joined");
  StorageManager storage;
  build.addAttribute("p_partkey", Type::Int());
  build.addAttribute("p_type", Type::Char(25));
  std::size_t at = 0;
  for (std::int64_t n : kBlockSizes) {
    storage.loadBlock(&build, {part.partkey.data() + at, part.type.data() + at * 25}, n);
    at += static_cast<std::size_t>(n);
  }
  probe.addAttribute("l_partkey", Type::Int());
  probe.addAttribute("l_qty", Type::Int());
  std::vector<std::int32_t> l_partkey, l_qty;
  std::uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const std::size_t parts = part.partkey.size();
  for (std::size_t i = 0; i < 20000; ++i) {
    l_partkey.push_back(static_cast<std::int32_t>(rnd() % (parts + 500)));   // some without a part
    l_qty.push_back(static_cast<std::int32_t>(i));
  }
  for (std::size_t from = 0; from < l_partkey.size(); from += 3333) {
    const std::size_t n = std::min<std::size_t>(3333, l_partkey.size() - from);
    storage.loadBlock(&probe, {l_partkey.data() + from, l_qty.data() + from}, static_cast<std::int64_t>(n));
  }
  out.addAttribute("l_partkey", Type::Int());
  out.addAttribute("l_qty", Type::Int());
  QueryContext ctx;
  const auto table = ctx.addJoinHashTable(kInt, static_cast<std::int64_t>(parts));
  const auto dest = ctx.addInsertDestination(&out, &storage);
  const auto selection = ctx.addScalarGroup({0, 1});
  const std::vector<bool> on_build = {false, false};
  Predicate residual;
  residual.conjuncts.push_back(ComparisonPredicate(1, comparison, TypedLiteral::Char("%BRASS"), /*build_side=*/true));
  const auto pred = ctx.addPredicate(residual);
  BuildHashOperator builder(0, build, true, {0}, false, 1, table);
  HashJoinOperator prober(0, build, probe, true, {0}, false, 1, false, out, dest, table, pred, selection, &on_build,
                          HashJoinOperator::JoinType::kInnerJoin);
  prober.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&builder, &ctx, &storage);
  fetchAndExecuteWorkOrders(&prober, &ctx, &storage);
  std::vector<std::pair<std::int32_t, std::int32_t>> got, want;
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    std::vector<std::int32_t> key(k), qty(k);
    blk->copyAttributeToHost(0, key.data());
    blk->copyAttributeToHost(1, qty.data());
    for (std::size_t i = 0; i < k; ++i) got.emplace_back(key[i], qty[i]);
  }
  for (std::size_t i = 0; i < l_partkey.size(); ++i) {
    const std::size_t p = static_cast<std::size_t>(l_partkey[i]);
    if (p < parts && LikeField(&part.type[p * 25], 25, "%BRASS") == (comparison == ComparisonID::kLike)) want.emplace_back(l_partkey[i], l_qty[i]);
  }
  std::sort(got.begin(), got.end());
  std::sort(want.begin(), want.end());
  EXPECT_TRUE(want.size() > 1000 && want.size() < l_partkey.size());
  EXPECT_EQ(got.size(), want.size());
  EXPECT_TRUE(got == want);
}

void expectUnsupported(const Part &part, const ComparisonPredicate &term, std::size_t blocks_per_order) {
  CatalogRelation rel(1, "part"), out(2, "out");
  StorageManager storage;
  load(part, &rel, &storage, false, false);
  out.addAttribute("p_partkey", Type::Int());
  QueryContext ctx;
  Predicate pred;
  pred.conjuncts.push_back(term);
  const auto pred_id = ctx.addPredicate(pred);
  const auto dest = ctx.addInsertDestination(&out, &storage);
  SelectOperator select(0, rel, false, out, dest, pred_id, std::vector<attribute_id>{kPartkey}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  int status = QSX_OK;
  try {
    fetchAndExecuteWorkOrders(&select, &ctx, &storage);
  } catch (const ExecutionError &e) {
    status = e.status();
  }
  EXPECT_EQ(status, static_cast<int>(QSX_ERR_UNSUPPORTED));
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "like_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  // the first six comparisons are the ABI's qsx_cmp_op_t; LIKE / NOT LIKE stand behind them
  EXPECT_EQ(static_cast<int>(ComparisonID::kGreaterOrEqual), static_cast<int>(QSX_GE));
  EXPECT_EQ(static_cast<int>(ComparisonID::kLike), 6);
  EXPECT_EQ(static_cast<int>(ComparisonID::kNotLike), 7);
  const auto like = [](attribute_id a, const char *p) { return ComparisonPredicate(a, ComparisonID::kLike, TypedLiteral::Char(p)); };
  const auto not_like = [](attribute_id a, const char *p) { return ComparisonPredicate(a, ComparisonID::kNotLike, TypedLiteral::Char(p)); };
  const ComparisonPredicate small(kSize, ComparisonID::kLess, TypedLiteral::Int(3)), large(kSize, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(2));
  std::vector<Predicate> predicates;
  for (const char *p : {"PROMO%", "%BRASS", "%ISH%", "MEDIUM POLISHED%", "%O%I%N", "_ROMO%", "STANDARD BURNISHED NICKEL", "%A%E%D T%"}) {
    predicates.push_back(Predicate{{like(kType, p)}});
    predicates.push_back(Predicate{{not_like(kType, p)}});
  }
  predicates.push_back(Predicate{{small, like(kType, "PROMO%")}});          // a numeric term in front of the LIKE term
  predicates.push_back(Predicate{{not_like(kType, "%BRASS"), large}});      // ... and behind it
  predicates.push_back(Predicate{{like(kType, "%E%"), not_like(kType, "%STEEL"), small}});
  predicates.push_back(Predicate{{like(kName, "%green%")}});                // a nullable attribute: NULLs are in neither result
  predicates.push_back(Predicate{{not_like(kName, "%green%")}});
  predicates.push_back(Predicate{{like(kName, "forest%"), like(kType, "%TIN")}});
  for (const bool sorted_on_type : {false, true}) {
    const Part part(sorted_on_type);
    for (const bool compressed : {false, true}) {
      if (sorted_on_type && !compressed) continue;   // (a plain CHAR sort column stays outside the run form, as before)
      for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
        for (const Predicate &pred : predicates) runSelect(part, pred, compressed, sorted_on_type, per_order);
      }
    }
    if (sorted_on_type) continue;
    for (const bool compressed : {false, true}) {
      for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) runAggregation(part, compressed, per_order);
    }
    for (const std::size_t per_order : {std::size_t(1), std::size_t(4)}) {
      runJoin(part, ComparisonID::kLike, per_order);
      runJoin(part, ComparisonID::kNotLike, per_order);
    }
    for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
      expectUnsupported(part, like(kSize, "1%"), per_order);                                     // not a CHAR(n) attribute
      expectUnsupported(part, like(kType, std::string(65, 'a').c_str()), per_order);             // a 65-byte pattern
    }
  }
  return finish("like_operator_test");
}
