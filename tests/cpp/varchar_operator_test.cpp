// VARCHAR attributes of adopted CompressedColumnStore blocks through the operators.  The images are written the way the
// reference's builder leaves them (varchar_block_image_util.hpp: p_type VARCHAR(25) behind 1-byte codes, p_name VARCHAR(55),
// nullable, behind 2-byte codes, a different dictionary in every block, the dictionaries at every byte alignment), copied to
// device memory and ADOPTED in place.  Then: Select with LIKE, NOT LIKE and the six comparisons against a string literal, per
// block and over runs; a nullable VARCHAR (a NULL is in no result); a predicate tree with a VARCHAR LIKE leaf; the projection of
// VARCHAR attributes; GROUP BY a VARCHAR(25) with COUNT and SUM; every use that is refused, with QSX_ERR_UNSUPPORTED; malformed
// dictionaries, with QSX_ERR_INVALID_ARGUMENT.  Expected results come from plain loops over the strings that built the images.
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "test_util.hpp"
#include "varchar_block_image_util.hpp"

using namespace quickstep;

namespace {
enum Attr : attribute_id { kPartkey = 0, kType, kName, kSize, kPrice };
const std::vector<std::int64_t> kBlockSizes = {2500, 1001, 0, 777, 3000};
constexpr std::size_t kBlockBytes = std::size_t(1) << 21;

bool Like(const char *t, std::size_t tn, const char *p, std::size_t pn) {
  if (pn == 0) return tn == 0;
  if (*p == '%') return Like(t, tn, p + 1, pn - 1) || (tn > 0 && Like(t + 1, tn - 1, p, pn));
  return tn > 0 && (*p == '_' || *p == *t) && Like(t + 1, tn - 1, p + 1, pn - 1);
}
bool LikeText(const std::string &text, const std::string &pattern) { return Like(text.data(), text.size(), pattern.data(), pattern.size()); }

struct Part {
  std::vector<std::int32_t> partkey, size;
  std::vector<double> price;
  std::vector<std::string> type, name;
  std::vector<bool> name_null;
  Part() {
    const char *a[] = {"STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO"};
    const char *b[] = {"ANODIZED", "BURNISHED", "PLATED", "POLISHED", "BRUSHED"};
    const char *c[] = {"TIN", "NICKEL", "BRASS", "STEEL", "COPPER"};
    const char *colors[] = {"green", "blue", "forest", "red", "almond", "lime", "greenish", "chartreuse", "lavender"};
    std::uint64_t x = 0x2545F4914F6CDD1Dull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::size_t block = 0;
    for (std::int64_t n : kBlockSizes) {
      for (std::int64_t i = 0; i < n; ++i) {
        partkey.push_back(static_cast<std::int32_t>(partkey.size()));
        size.push_back(static_cast<std::int32_t>(rnd() % 5));
        price.push_back(static_cast<double>(rnd() % 100000));
        // every block its own vocabulary (block k never holds the k-th first word), the empty string and a text of exactly 25
        // bytes ("STANDARD BURNISHED NICKEL") among the values
        std::size_t first = rnd() % 6;
        if (first == block % 6) first = (first + 1) % 6;
        std::string t = std::string(a[first]) + " " + b[rnd() % 5] + " " + c[rnd() % 5];
        if (rnd() % 50 == 0) t.clear();
        type.push_back(t);
        name.push_back(std::string(colors[rnd() % 9]) + " " + colors[rnd() % 9] + " " + std::to_string(rnd() % 400));
        name_null.push_back(rnd() % 4 == 0);
      }
      ++block;
    }
  }
};

struct Loaded {
  CatalogRelation rel{1, "part"};
  StorageManager storage;
  std::vector<void *> images;
  ~Loaded() { for (void *p : images) qsx_device_free(p); }
};

void *Upload(const std::vector<unsigned char> &image) {
  void *dev = nullptr;
  CheckStatus(qsx_device_alloc(image.size(), &dev), "qsx_device_alloc");
  CheckStatus(qsx_copy_to_device(dev, image.data(), image.size(), nullptr), "qsx_copy_to_device");
  CheckStatus(qsx_stream_synchronize(nullptr), "qsx_stream_synchronize");
  return dev;
}

void AddAttributes(CatalogRelation *rel) {
  rel->addAttribute("p_partkey", Type::Int());
  rel->addAttribute("p_type", Type::VarChar(25));
  rel->addAttribute("p_name", Type::VarChar(55).getNullableVersion());
  rel->addAttribute("p_size", Type::Int());
  rel->addAttribute("p_price", Type::Double());
}

// the images of the blocks, adopted: this is the step that a layer without VARCHAR refuses
void load(const Part &part, Loaded *l) {
  AddAttributes(&l->rel);
  std::size_t at = 0, block = 0, aligned_offsets = 0, copied_offsets = 0;
  for (std::int64_t n : kBlockSizes) {
    const std::size_t k = static_cast<std::size_t>(n);
    block_image::VarCharColumn type, name;
    type.values.assign(part.type.begin() + at, part.type.begin() + at + k);
    type.code_width = 1;
    name.values.assign(part.name.begin() + at, part.name.begin() + at + k);
    name.nulls.assign(part.name_null.begin() + at, part.name_null.begin() + at + k);
    name.code_width = 2;
    block_image::VarCharImageInfo where;
    const std::vector<unsigned char> image = block_image::BuildCompressedWithVarChar(
        l->rel, {part.partkey.data() + at, nullptr, nullptr, part.size.data() + at, part.price.data() + at}, {nullptr, &type, &name, nullptr, nullptr},
        n, kBlockBytes, /*info_padding=*/block, &where);
    EXPECT_TRUE(where.max_tuples >= n);
    l->images.push_back(Upload(image));
    const block_id id = l->storage.adoptBlockImage(&l->rel, l->images.back(), image.size());
    BlockReference blk = l->storage.getBlock(id);
    EXPECT_EQ(blk->numTuples(), n);
    for (const attribute_id a : {kType, kName}) {
      const CompressedAttribute *c = blk->compressedAttribute(a);
      EXPECT_TRUE(c != nullptr && c->kind == CompressedAttribute::kDictionary && c->variable_length);
      if (c == nullptr) continue;
      const block_image::VarCharColumn &column = a == kType ? type : name;
      const std::vector<std::string> dict = block_image::SortedDictionary(column, k);
      std::size_t bytes = 0;
      for (const std::string &v : dict) bytes += v.size() + 1;
      EXPECT_EQ(c->num_codes, dict.size());
      EXPECT_EQ(c->code_width, column.code_width);
      EXPECT_EQ(c->variable_value_bytes, bytes);
      // the values are read in place; the offsets too unless the image leaves them at an address that is no multiple of 4
      const char *base = static_cast<const char *>(l->images.back());
      EXPECT_TRUE(c->variable_values == base + where.dictionary_offset[a] + 8 + 4 * dict.size());
      const bool aligned = (where.dictionary_offset[a] + 8) % 4 == 0;
      if (dict.empty()) continue;
      EXPECT_TRUE(aligned == (c->variable_offsets_owned == nullptr));
      EXPECT_TRUE(!aligned || reinterpret_cast<const char *>(c->variable_offsets) == base + where.dictionary_offset[a] + 8);
      ++(aligned ? aligned_offsets : copied_offsets);
      EXPECT_TRUE(!blk->valuesMaterialized(a));
    }
    EXPECT_TRUE((blk->nullBitmap(kName) != nullptr) == (n > 0));   // the NULL code became the attribute's null bitmap
    at += k;
    ++block;
  }
  EXPECT_TRUE(aligned_offsets > 0 && copied_offsets > 0);   // both placements were met
}

int Compare(const std::string &value, const std::string &literal) { return value < literal ? -1 : (value == literal ? 0 : 1); }
bool TermPasses(const Part &part, std::size_t i, const ComparisonPredicate &term) {
  if (term.attribute == kSize) {
    const std::int32_t v = part.size[i], lit = term.literal.v.i32;
    return term.comparison == ComparisonID::kLess ? v < lit : v >= lit;
  }
  if (term.attribute == kName && part.name_null[i]) return false;   // a NULL passes no comparison
  const std::string &text = term.attribute == kType ? part.type[i] : part.name[i];
  switch (term.comparison) {
    case ComparisonID::kLike: return LikeText(text, term.literal.text);
    case ComparisonID::kNotLike: return !LikeText(text, term.literal.text);
    case ComparisonID::kEqual: return Compare(text, term.literal.text) == 0;
    case ComparisonID::kNotEqual: return Compare(text, term.literal.text) != 0;
    case ComparisonID::kLess: return Compare(text, term.literal.text) < 0;
    case ComparisonID::kLessOrEqual: return Compare(text, term.literal.text) <= 0;
    case ComparisonID::kGreater: return Compare(text, term.literal.text) > 0;
    default: return Compare(text, term.literal.text) >= 0;
  }
}
bool NodePasses(const Part &part, std::size_t i, const PredicateNode &node) {
  switch (node.kind) {
    case PredicateNode::kComparison: return TermPasses(part, i, node.comparison);
    case PredicateNode::kNegation: {
      // NOT over a comparison with a NULL operand selects the row (NegationPredicate.cpp:70-90: the comparison is not true)
      return !NodePasses(part, i, *node.children[0]);
    }
    case PredicateNode::kConjunction: {
      for (const auto &child : node.children) if (!NodePasses(part, i, *child)) return false;
      return true;
    }
    default: {
      for (const auto &child : node.children) if (NodePasses(part, i, *child)) return true;
      return false;
    }
  }
}
bool RowPasses(const Part &part, std::size_t i, const Predicate &pred) {
  for (const ComparisonPredicate &term : pred.conjuncts) if (!TermPasses(part, i, term)) return false;
  return pred.tree == nullptr || NodePasses(part, i, *pred.tree);
}

void runSelect(const Part &part, const Predicate &pred, std::size_t blocks_per_order, bool may_be_trivial = false) {
  Loaded l;
  load(part, &l);
  CatalogRelation out(2, "out");
  out.addAttribute("p_partkey", Type::Int());
  QueryContext ctx;
  const auto pred_id = ctx.addPredicate(pred);
  const auto dest = ctx.addInsertDestination(&out, &l.storage);
  SelectOperator select(0, l.rel, false, out, dest, pred_id, std::vector<attribute_id>{kPartkey}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &l.storage);
  std::vector<std::int32_t> got, want;
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = l.storage.getBlock(b);
    const std::size_t at = got.size(), k = static_cast<std::size_t>(blk->numTuples());
    got.resize(at + k);
    if (k > 0) blk->copyAttributeToHost(0, got.data() + at);
  }
  for (std::size_t i = 0; i < part.partkey.size(); ++i) if (RowPasses(part, i, pred)) want.push_back(part.partkey[i]);
  std::sort(got.begin(), got.end());
  if (!may_be_trivial) EXPECT_TRUE(!want.empty() && want.size() < part.partkey.size());   // a predicate that keeps nothing or everything shows nothing
  EXPECT_EQ(got.size(), want.size());
  EXPECT_TRUE(got == want);
  // predicates work on the dictionaries and the codes: no VARCHAR attribute was decoded
  for (block_id b : l.rel.getBlocksSnapshot()) {
    BlockReference blk = l.storage.getBlock(b);
    EXPECT_TRUE(!blk->valuesMaterialized(kType) && !blk->valuesMaterialized(kName));
  }
}

// select p_partkey, p_type, p_name from part where p_size >= 1: VARCHAR attributes in the output, as n-byte NUL-padded fields
void runProjection(const Part &part, std::size_t blocks_per_order) {
  Loaded l;
  load(part, &l);
  CatalogRelation out(2, "out");
  out.addAttribute("p_partkey", Type::Int());
  out.addAttribute("p_type", Type::VarChar(25));
  out.addAttribute("p_name", Type::VarChar(55).getNullableVersion());
  QueryContext ctx;
  Predicate pred;
  pred.conjuncts.push_back({kSize, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(1)});
  const auto pred_id = ctx.addPredicate(pred);
  const auto dest = ctx.addInsertDestination(&out, &l.storage);
  const std::int64_t fetches_before = NumVariableDictionaryValueFetches();
  SelectOperator select(0, l.rel, false, out, dest, pred_id, std::vector<attribute_id>{kPartkey, kType, kName}, true);
  select.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &l.storage);
  EXPECT_EQ(NumVariableDictionaryValueFetches(), fetches_before);   // decoding never fetches the values to the host
  std::size_t rows = 0, nulls_seen = 0, full_width = 0;
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = l.storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    std::vector<std::int32_t> key(k);
    std::vector<char> type(k * 25), name(k * 55);
    std::vector<std::uint64_t> nulls((k + 63) / 64);
    blk->copyAttributeToHost(0, key.data());
    blk->copyAttributeToHost(1, type.data());
    blk->copyAttributeToHost(2, name.data());
    blk->copyNullBitmapToHost(2, nulls.data());
    for (std::size_t i = 0; i < k; ++i) {
      const std::size_t p = static_cast<std::size_t>(key[i]);
      EXPECT_TRUE(part.size[p] >= 1);
      char want_type[25] = {}, want_name[55] = {};   // the text, NULs behind it; exactly 25 bytes: no terminator
      std::memcpy(want_type, part.type[p].data(), part.type[p].size());
      full_width += part.type[p].size() == 25 ? 1 : 0;
      const bool is_null = ((nulls[i >> 6] >> (63 - (i & 63))) & 1u) != 0;
      EXPECT_TRUE(is_null == part.name_null[p]);
      if (!part.name_null[p]) std::memcpy(want_name, part.name[p].data(), part.name[p].size());   // (a NULL's field is all NUL)
      nulls_seen += is_null ? 1 : 0;
      if (std::memcmp(&type[i * 25], want_type, 25) != 0 || std::memcmp(&name[i * 55], want_name, 55) != 0) {
        std::fprintf(stderr, "projection: row with p_partkey %d differs\n", key[i]);
        ++g_failures;
        return;
      }
    }
    rows += k;
  }
  std::size_t want_rows = 0;
  for (std::size_t i = 0; i < part.partkey.size(); ++i) want_rows += part.size[i] >= 1 ? 1 : 0;
  EXPECT_EQ(rows, want_rows);
  EXPECT_TRUE(nulls_seen > 100 && full_width > 10);
}

// select p_type, count(*), sum(p_price) from part where p_type not like '%TIN' group by p_type
void runGroupBy(const Part &part, std::size_t blocks_per_order) {
  Loaded l;
  load(part, &l);
  CatalogRelation result(2, "result");
  result.addAttribute("p_type", Type::VarChar(25));
  result.addAttribute("count", Type::Long());
  result.addAttribute("sum_price", Type::Double());
  QueryContext ctx;
  Predicate pred;
  pred.conjuncts.push_back({kType, ComparisonID::kNotLike, TypedLiteral::Char("%TIN")});
  const auto dest = ctx.addInsertDestination(&result, &l.storage);
  AggregationStateSpec spec;
  spec.input_relation = &l.rel;
  spec.group_by = {kType};
  spec.aggregates = {AggregateSpec(AggregationID::kCount, kInvalidAttributeID), AggregateSpec(AggregationID::kSum, kPrice)};
  spec.predicate = ctx.getPredicate(ctx.addPredicate(pred));
  spec.strategy = QSX_AGG_GENERIC;
  spec.estimated_num_groups = 64;
  const auto state = ctx.addAggregationState(spec);
  AggregationOperator aggregate(0, l.rel, true, state);
  FinalizeAggregationOperator finalize(0, state, 1, false, 1, result, dest);
  aggregate.setBlocksPerWorkOrder(blocks_per_order);
  fetchAndExecuteWorkOrders(&aggregate, &ctx, &l.storage);
  fetchAndExecuteWorkOrders(&finalize, &ctx, &l.storage);
  std::map<std::string, std::pair<std::int64_t, double>> want, got;
  for (std::size_t i = 0; i < part.partkey.size(); ++i) {
    if (LikeText(part.type[i], "%TIN")) continue;
    want[part.type[i]].first += 1;
    want[part.type[i]].second += part.price[i];
  }
  for (block_id b : ctx.getInsertDestination(dest)->getTouchedBlocks()) {
    BlockReference blk = l.storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    if (k == 0) continue;
    std::vector<char> key(k * 25);
    std::vector<std::int64_t> cnt(k);
    std::vector<double> sum(k);
    blk->copyAttributeToHost(0, key.data());
    blk->copyAttributeToHost(1, cnt.data());
    blk->copyAttributeToHost(2, sum.data());
    for (std::size_t i = 0; i < k; ++i) {
      const std::string text(&key[i * 25], ::strnlen(&key[i * 25], 25));
      for (std::size_t j = text.size(); j < 25; ++j) EXPECT_TRUE(key[i * 25 + j] == 0);   // a VarChar(25) field: NUL-padded
      EXPECT_TRUE(got.find(text) == got.end());
      got[text] = {cnt[i], sum[i]};
    }
  }
  EXPECT_TRUE(want.size() > 100 && want.count("") == 1 && want.count("STANDARD BURNISHED NICKEL") == 1);   // the empty string and 25 bytes are groups
  EXPECT_EQ(got.size(), want.size());
  EXPECT_TRUE(got == want);   // integer-valued doubles below 2^53: exact in any order
}

int StatusOf(const std::function<void()> &run, std::string *message = nullptr) {
  try {
    run();
  } catch (const ExecutionError &e) {
    if (message != nullptr) *message = e.what();
    return e.status();
  }
  return QSX_OK;
}
void expectRefused(const char *what, const char *word, const std::function<void()> &run) {
  std::string message;
  const int status = StatusOf(run, &message);
  if (status != QSX_ERR_UNSUPPORTED || message.find(word) == std::string::npos) {
    std::fprintf(stderr, "%s: status %d, message \"%s\" (expected QSX_ERR_UNSUPPORTED and a message naming %s)\n", what, status, message.c_str(), word);
    ++g_failures;
  }
}

void runSelectOf(Loaded *l, const Predicate &pred, std::size_t per_order) {
  CatalogRelation out(2, "out");
  out.addAttribute("p_partkey", Type::Int());
  QueryContext ctx;
  const auto pred_id = ctx.addPredicate(pred);
  const auto dest = ctx.addInsertDestination(&out, &l->storage);
  SelectOperator select(0, l->rel, false, out, dest, pred_id, std::vector<attribute_id>{kPartkey}, true);
  select.setBlocksPerWorkOrder(per_order);
  fetchAndExecuteWorkOrders(&select, &ctx, &l->storage);
}

void runRefusedCases(const Part &part) {
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    Loaded l;
    load(part, &l);
    expectRefused("IN list", "IN list on a VARCHAR", [&]() {
      Predicate pred;
      pred.tree = Predicate::In(kType, {TypedLiteral::Char("PROMO PLATED TIN"), TypedLiteral::Char("SMALL PLATED TIN")});
      runSelectOf(&l, pred, per_order);
    });
    expectRefused("attribute vs attribute", "VARCHAR", [&]() {
      Predicate pred;
      pred.conjuncts.push_back(ComparisonPredicate::Attributes(kType, false, ComparisonID::kLess, kName, false));
      runSelectOf(&l, pred, per_order);
    });
    expectRefused("SUBSTRING", "SUBSTRING", [&]() {
      CatalogRelation out(2, "out");
      out.addAttribute("prefix", Type::Char(5));
      QueryContext ctx;
      const auto pred_id = ctx.addPredicate(Predicate());
      const auto dest = ctx.addInsertDestination(&out, &l.storage);
      SelectOperator select(0, l.rel, false, out, dest, pred_id, std::vector<ScalarPtr>{Scalar::Substring(0, 5, Scalar::Attribute(kType))}, true);
      select.setBlocksPerWorkOrder(per_order);
      fetchAndExecuteWorkOrders(&select, &ctx, &l.storage);
    });
    expectRefused("aggregate argument", "aggregate's argument", [&]() {
      QueryContext ctx;
      AggregationStateSpec spec;
      spec.input_relation = &l.rel;
      spec.group_by = {kSize};
      spec.aggregates = {AggregateSpec(AggregationID::kMin, kType)};
      spec.strategy = QSX_AGG_COMPACT_KEY;
      spec.estimated_num_groups = 8;
      ctx.addAggregationState(spec);
    });
    expectRefused("join key (table)", "join key", [&]() {
      QueryContext ctx;
      ctx.addJoinHashTable(kVarChar, 1000);
    });
    expectRefused("join key (build)", "join key", [&]() {
      QueryContext ctx;
      const auto table = ctx.addJoinHashTable(kLong, 10000);
      BuildHashOperator builder(0, l.rel, true, {kType}, false, 1, table);
      builder.setBlocksPerWorkOrder(per_order);
      fetchAndExecuteWorkOrders(&builder, &ctx, &l.storage);
    });
    expectRefused("ORDER BY", "ORDER BY", [&]() {
      CatalogRelation runs(3, "runs"), output(4, "sorted");
      AddAttributes(&runs);
      AddAttributes(&output);
      QueryContext ctx;
      const auto config_id = ctx.addSortConfig(QueryContext::SortConfiguration{{kType}, {true}});
      const auto run_dest = ctx.addInsertDestination(&runs, &l.storage);
      SortRunGenerationOperator generate(0, l.rel, runs, run_dest, config_id, true);
      fetchAndExecuteWorkOrders(&generate, &ctx, &l.storage);
    });
  }
  // building a variable-length dictionary is not this layer's: loadBlock with `compress` set on a VARCHAR attribute
  expectRefused("loadBlock(compress)", "VARCHAR", [&]() {
    CatalogRelation rel(5, "padded");
    rel.addAttribute("v", Type::VarChar(8));
    StorageManager storage;
    const std::vector<char> fields(8 * 4, 0);
    const std::vector<bool> compress = {true};
    storage.loadBlock(&rel, {fields.data()}, 4, 0, &compress);
  });
  // a VARCHAR attribute in a basic column store image
  expectRefused("basic column store", "basic column store", [&]() {
    CatalogRelation rel(6, "basic");
    rel.addAttribute("k", Type::Int());
    rel.addAttribute("v", Type::VarChar(8));
    const std::vector<std::int32_t> k(10, 1);
    const std::vector<char> v(80, 0);
    const std::vector<unsigned char> image = block_image::Build(rel, {k.data(), v.data()}, {{}, {}}, 10, kBlockBytes);
    void *dev = Upload(image);
    StorageManager storage;
    try {
      storage.adoptBlockImage(&rel, dev, image.size());
    } catch (...) {
      qsx_device_free(dev);
      throw;
    }
    qsx_device_free(dev);
  });
}

void runMalformed(const Part &part) {
  for (const block_image::Damage damage : {block_image::Damage::kDescendingOffset, block_image::Damage::kNoFinalNul, block_image::Damage::kNone}) {
    Loaded l;
    AddAttributes(&l.rel);
    const std::size_t k = 500;
    block_image::VarCharColumn type, name;
    type.values.assign(part.type.begin(), part.type.begin() + k);
    name.values.assign(part.name.begin(), part.name.begin() + k);
    name.code_width = 2;
    // (the damage goes to every VARCHAR dictionary of the image; the undamaged image is adopted: the builder is sound)
    const std::vector<unsigned char> image = block_image::BuildCompressedWithVarChar(
        l.rel, {part.partkey.data(), nullptr, nullptr, part.size.data(), part.price.data()}, {nullptr, &type, &name, nullptr, nullptr},
        static_cast<std::int64_t>(k), kBlockBytes, 0, nullptr, damage);
    l.images.push_back(Upload(image));
    const int status = StatusOf([&]() { l.storage.adoptBlockImage(&l.rel, l.images.back(), image.size()); });
    EXPECT_EQ(status, static_cast<int>(damage == block_image::Damage::kNone ? QSX_OK : QSX_ERR_INVALID_ARGUMENT));
  }
  // a VARCHAR attribute of a compressed store without a dictionary: malformed
  Loaded l;
  l.rel.addAttribute("k", Type::Int());
  l.rel.addAttribute("v", Type::VarChar(4));
  const std::vector<std::int32_t> k(10, 1), v(10, 0);
  const std::vector<unsigned char> image = block_image::BuildCompressedWithVarChar(l.rel, {k.data(), v.data()}, {nullptr, nullptr}, 10, kBlockBytes, 0);
  l.images.push_back(Upload(image));
  EXPECT_EQ(StatusOf([&]() { l.storage.adoptBlockImage(&l.rel, l.images.back(), image.size()); }), static_cast<int>(QSX_ERR_INVALID_ARGUMENT));
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "varchar_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const Part part;
  const auto term = [](attribute_id a, ComparisonID c, const char *text) { return ComparisonPredicate(a, c, TypedLiteral::Char(text)); };
  const ComparisonPredicate small(kSize, ComparisonID::kLess, TypedLiteral::Int(3)), large(kSize, ComparisonID::kGreaterOrEqual, TypedLiteral::Int(2));
  std::vector<Predicate> predicates;
  for (const char *p : {"PROMO%", "%BRASS", "%ISH%", "MEDIUM POLISHED%", "%O%I%N", "_ROMO%", "STANDARD BURNISHED NICKEL", "%A%E%D T%", ""}) {
    predicates.push_back(Predicate{{term(kType, ComparisonID::kLike, p)}});
    predicates.push_back(Predicate{{term(kType, ComparisonID::kNotLike, p)}});
  }
  predicates.push_back(Predicate{{term(kName, ComparisonID::kLike, "%green%")}});            // a nullable attribute: NULLs are in neither result
  predicates.push_back(Predicate{{term(kName, ComparisonID::kNotLike, "%green%")}});
  predicates.push_back(Predicate{{term(kName, ComparisonID::kLike, "forest%1_"), term(kType, ComparisonID::kLike, "%TIN")}});
  predicates.push_back(Predicate{{small, term(kType, ComparisonID::kLike, "PROMO%")}});      // a numeric term in front of the LIKE term
  predicates.push_back(Predicate{{term(kType, ComparisonID::kNotLike, "%BRASS"), large}});   // ... and behind it
  // the six comparisons: a literal every dictionary holds, one that lies between two entries of every dictionary ("MEDIUM": = keeps
  // nothing and <> everything, the orderings cut the dictionaries), one that block 3's dictionary does not hold (its vocabulary
  // has no LARGE), and on the nullable attribute a value that the data holds
  std::size_t some_name = 0;
  while (part.name_null[some_name]) ++some_name;
  std::vector<Predicate> trivial;
  for (const ComparisonID c : {ComparisonID::kEqual, ComparisonID::kNotEqual, ComparisonID::kLess, ComparisonID::kLessOrEqual, ComparisonID::kGreater,
                               ComparisonID::kGreaterOrEqual}) {
    predicates.push_back(Predicate{{term(kType, c, "PROMO BRUSHED TIN")}});
    (c == ComparisonID::kEqual || c == ComparisonID::kNotEqual ? trivial : predicates).push_back(Predicate{{term(kType, c, "MEDIUM")}});
    predicates.push_back(Predicate{{term(kType, c, "LARGE PLATED STEEL")}});
    predicates.push_back(Predicate{{term(kName, c, part.name[some_name].c_str())}});
  }
  // a tree: a VARCHAR LIKE leaf under OR and NOT, beside a numeric leaf and a comparison leaf on the nullable VARCHAR
  Predicate tree;
  tree.tree = Predicate::Or({Predicate::And({Predicate::Compare(kType, ComparisonID::kLike, TypedLiteral::Char("PROMO%")),
                                             Predicate::Not(Predicate::Compare(kName, ComparisonID::kLike, TypedLiteral::Char("%blue%")))}),
                             Predicate::And({Predicate::Compare(kSize, ComparisonID::kLess, TypedLiteral::Int(1)),
                                             Predicate::Compare(kType, ComparisonID::kGreater, TypedLiteral::Char("SMALL"))})});
  predicates.push_back(tree);
  Predicate chained = tree;
  chained.conjuncts.push_back(term(kType, ComparisonID::kNotLike, "%STEEL"));
  predicates.push_back(chained);
  const std::int64_t fetches_at_start = NumVariableDictionaryValueFetches();
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    for (std::size_t k = 0; k < predicates.size(); ++k) {
      const std::int64_t before = NumVariableDictionaryValueFetches();
      runSelect(part, predicates[k], per_order);
      if (k < 21) EXPECT_EQ(NumVariableDictionaryValueFetches(), before);   // LIKE / NOT LIKE never fetch the value bytes
    }
  }
  EXPECT_TRUE(NumVariableDictionaryValueFetches() > fetches_at_start);        // the comparisons did, once per block
  // = against an absent literal keeps nothing, <> everything: trivial results, still right
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    for (const Predicate &pred : trivial) runSelect(part, pred, per_order, /*may_be_trivial=*/true);
  }
  for (const std::size_t per_order : {std::size_t(1), std::size_t(5)}) {
    runProjection(part, per_order);
    runGroupBy(part, per_order);
  }
  runRefusedCases(part);
  runMalformed(part);
  return finish("varchar_operator_test");
}
