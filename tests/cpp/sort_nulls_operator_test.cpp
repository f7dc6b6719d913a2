// ORDER BY over nullable and CHAR(n) attributes through SortRunGenerationOperator -> SortMergeRunOperator.  Mirrors the NULL
// cases of relational_operators/tests/SortRunGenerationOperator_unittest.cpp (1Column / 3Column, NullFirst / NullLast, Asc /
// Desc, MixedNullOrdering_MixedOrdering, :480-786) on that file's data (TestTuple :92-110: three columns cut out of the bits
// of a seed, NULL where the value is zero, :228-251), adds CHAR(10) / CHAR(25) keys, and checks what the reference's blocks do
// by construction: the output carries the null bitmaps of every nullable attribute, key or not.  Blocks of 2500 rows (not a
// multiple of 64: the bitmaps of the runs cannot be appended word-wise), with and without top-k, Foreman and synchronous.
#include <algorithm>
#include <cstring>
#include <string>

#include "test_util.hpp"

using namespace quickstep;

namespace {
constexpr std::int64_t kRows = 9000;
constexpr std::int64_t kBlockRows = 2500;   // 4 runs, the last one short
enum Attr : attribute_id { kN1 = 0, kN2, kN3, kTid, kS10, kS25, kX, kNumAttrs };

struct Row {
  std::int32_t n[3];
  bool null_n[3];
  std::int32_t tid;
  char s10[10];
  char s25[25];
  bool null_s25;
  double x;
  bool null_x;
};

std::vector<Row> makeRows() {
  std::vector<Row> rows;
  std::uint64_t state = 987654321ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto bits = [](int value, int offset, int length) { return (value >> offset) & (0xffff >> (16 - length)); };
  for (std::int64_t i = 0; i < kRows; ++i) {
    Row r{};
    const int seed = static_cast<int>(rnd() % 256);
    r.n[0] = bits(seed, 3, 5); r.n[1] = bits(seed, 6, 2); r.n[2] = bits(seed, 1, 3);
    for (int c = 0; c < 3; ++c) {
      r.null_n[c] = r.n[c] == 0;
      if (r.null_n[c]) r.n[c] = static_cast<std::int32_t>(rnd());   // the bytes under a NULL are never looked at
    }
    r.tid = static_cast<std::int32_t>(i);
    // CHAR(10): a priority-like word of 0..10 bytes, garbage behind the terminating NUL; bytes >= 0x80 among them
    const int len10 = static_cast<int>(rnd() % 11);
    for (int b = 0; b < 10; ++b) r.s10[b] = b < len10 ? static_cast<char>("AB\x80\xff"[rnd() % 4]) : (b == len10 ? '\0' : static_cast<char>(rnd()));
    // CHAR(25): "Name#" + 4 digits, NUL padded: the last two 8-byte words never vary
    std::memset(r.s25, 0, sizeof(r.s25));
    std::snprintf(r.s25, sizeof(r.s25), "Name#%04d", static_cast<int>(rnd() % 300));
    r.null_s25 = rnd() % 5 == 0;
    r.x = static_cast<double>(rnd() % 1000) / 4.0;
    r.null_x = rnd() % 3 == 0;
    rows.push_back(r);
  }
  return rows;
}

struct Config {
  std::vector<attribute_id> order_by;
  std::vector<bool> ordering, null_ordering;   // null_ordering may be empty: all last
};

std::string charValue(const char *p, int width) { return std::string(p, ::strnlen(p, static_cast<std::size_t>(width))); }

// -1 / 0 / +1: x before / with / behind y in the ORDER BY column k (StorageBlock::sortColumn: the NULLs of a column stand in
// front of or behind its sorted non-NULL values whatever the direction)
int CompareKey(const Row &x, const Row &y, const Config &config, std::size_t k) {
  const attribute_id a = config.order_by[k];
  const bool nulls_first = k < config.null_ordering.size() && config.null_ordering[k];
  bool xn = false, yn = false;
  if (a <= kN3) { xn = x.null_n[a]; yn = y.null_n[a]; }
  if (a == kS25) { xn = x.null_s25; yn = y.null_s25; }
  if (a == kX) { xn = x.null_x; yn = y.null_x; }
  if (xn || yn) return xn == yn ? 0 : ((xn == nulls_first) ? -1 : 1);
  int cmp = 0;
  if (a <= kN3) {
    cmp = x.n[a] < y.n[a] ? -1 : (x.n[a] > y.n[a] ? 1 : 0);
  } else if (a == kTid) {
    cmp = x.tid < y.tid ? -1 : (x.tid > y.tid ? 1 : 0);
  } else if (a == kX) {
    cmp = x.x < y.x ? -1 : (x.x > y.x ? 1 : 0);
  } else {
    const std::string sx = a == kS10 ? charValue(x.s10, 10) : charValue(x.s25, 25), sy = a == kS10 ? charValue(y.s10, 10) : charValue(y.s25, 25);
    const int c = std::char_traits<char>::compare(sx.data(), sy.data(), std::min(sx.size(), sy.size()));   // unsigned chars
    cmp = c != 0 ? (c < 0 ? -1 : 1) : (sx.size() < sy.size() ? -1 : (sx.size() > sy.size() ? 1 : 0));
  }
  return config.ordering[k] ? cmp : -cmp;
}

bool Before(const Row &x, const Row &y, const Config &config) {
  for (std::size_t k = 0; k < config.order_by.size(); ++k) {
    const int cmp = CompareKey(x, y, config, k);
    if (cmp != 0) return cmp < 0;
  }
  return false;
}

std::vector<std::uint64_t> packBits(const std::vector<bool> &bits) {
  std::vector<std::uint64_t> words((bits.size() + 63) / 64 + 1, 0);
  for (std::size_t i = 0; i < bits.size(); ++i) {
    if (bits[i]) words[i / 64] |= 1ull << (63 - i % 64);   // TupleIdSequence bit order
  }
  return words;
}

// The tuples of `blocks` with their null bits; what lies under a NULL is not compared later.
std::vector<Row> readRows(const std::vector<block_id> &blocks, StorageManager &storage, std::vector<std::size_t> *block_sizes) {
  std::vector<Row> out;
  for (block_id b : blocks) {
    BlockReference blk = storage.getBlock(b);
    const std::size_t k = static_cast<std::size_t>(blk->numTuples());
    std::vector<std::int32_t> n[3], tid(k);
    std::vector<char> s10(k * 10), s25(k * 25);
    std::vector<double> x(k);
    std::vector<std::uint64_t> nulls[kNumAttrs];
    for (int c = 0; c < 3; ++c) { n[c].resize(k); blk->copyAttributeToHost(static_cast<attribute_id>(c), n[c].data()); }
    blk->copyAttributeToHost(kTid, tid.data());
    blk->copyAttributeToHost(kS10, s10.data());
    blk->copyAttributeToHost(kS25, s25.data());
    blk->copyAttributeToHost(kX, x.data());
    for (attribute_id a = 0; a < kNumAttrs; ++a) {
      nulls[a].assign((k + 63) / 64 + 1, 0);
      blk->copyNullBitmapToHost(a, nulls[a].data());
    }
    auto bit = [&](attribute_id a, std::size_t i) { return ((nulls[a][i / 64] >> (63 - i % 64)) & 1u) != 0; };
    for (std::size_t i = 0; i < k; ++i) {
      Row r{};
      for (int c = 0; c < 3; ++c) { r.n[c] = n[c][i]; r.null_n[c] = bit(static_cast<attribute_id>(c), i); }
      r.tid = tid[i];
      std::memcpy(r.s10, &s10[i * 10], 10);
      std::memcpy(r.s25, &s25[i * 25], 25);
      r.null_s25 = bit(kS25, i);
      r.x = x[i];
      r.null_x = bit(kX, i);
      EXPECT_TRUE(!bit(kTid, i) && !bit(kS10, i));
      out.push_back(r);
    }
    if (block_sizes != nullptr) block_sizes->push_back(k);
  }
  return out;
}

// the tuple that came out is the input tuple with that tid: values where it is not NULL, and every null bit
void ExpectSameTuple(const Row &got, const std::vector<Row> &rows) {
  EXPECT_TRUE(got.tid >= 0 && got.tid < static_cast<std::int32_t>(rows.size()));
  if (got.tid < 0 || got.tid >= static_cast<std::int32_t>(rows.size())) return;
  const Row &want = rows[static_cast<std::size_t>(got.tid)];
  for (int c = 0; c < 3; ++c) {
    EXPECT_EQ(got.null_n[c], want.null_n[c]);
    if (!want.null_n[c]) EXPECT_EQ(got.n[c], want.n[c]);
  }
  EXPECT_TRUE(std::memcmp(got.s10, want.s10, 10) == 0);
  EXPECT_EQ(got.null_s25, want.null_s25);
  if (!want.null_s25) EXPECT_TRUE(std::memcmp(got.s25, want.s25, 25) == 0);
  EXPECT_EQ(got.null_x, want.null_x);           // a nullable attribute that is no ORDER BY key
  if (!want.null_x) EXPECT_TRUE(got.x == want.x);
}

void runCase(const std::vector<Row> &rows, const Config &config, std::size_t top_k, bool use_foreman, bool limit_runs) {
  CatalogRelation input(1, "input"), runs(2, "runs"), output(3, "output");
  StorageManager storage;
  for (CatalogRelation *r : {&input, &runs, &output}) {
    r->addAttribute("n1", Type::Int().getNullableVersion());
    r->addAttribute("n2", Type::Int().getNullableVersion());
    r->addAttribute("n3", Type::Int().getNullableVersion());
    r->addAttribute("tid", Type::Int());
    r->addAttribute("s10", Type::Char(10));
    r->addAttribute("s25", Type::Char(25).getNullableVersion());
    r->addAttribute("x", Type::Double().getNullableVersion());
  }
  for (std::int64_t at = 0; at < kRows; at += kBlockRows) {
    const std::int64_t k = std::min(kBlockRows, kRows - at);
    std::vector<std::int32_t> n[3], tid;
    std::vector<char> s10, s25;
    std::vector<double> x;
    std::vector<bool> null_bits[kNumAttrs];
    for (std::int64_t i = at; i < at + k; ++i) {
      const Row &r = rows[static_cast<std::size_t>(i)];
      for (int c = 0; c < 3; ++c) { n[c].push_back(r.n[c]); null_bits[c].push_back(r.null_n[c]); }
      tid.push_back(r.tid);
      s10.insert(s10.end(), r.s10, r.s10 + 10);
      s25.insert(s25.end(), r.s25, r.s25 + 25);
      null_bits[kS25].push_back(r.null_s25);
      x.push_back(r.x);
      null_bits[kX].push_back(r.null_x);
    }
    std::vector<std::vector<std::uint64_t>> words(kNumAttrs);
    std::vector<const std::uint64_t *> bitmaps(kNumAttrs, nullptr);
    for (attribute_id a : {kN1, kN2, kN3, kS25, kX}) {
      words[a] = packBits(null_bits[a]);
      bitmaps[a] = words[a].data();
    }
    storage.loadBlock(&input, {n[0].data(), n[1].data(), n[2].data(), tid.data(), s10.data(), s25.data(), x.data()}, k, 0, nullptr, &bitmaps);
  }
  QueryContext ctx;
  QueryContext::SortConfiguration sort_config;
  if (config.null_ordering.empty()) {
    sort_config = {config.order_by, config.ordering};             // the existing style: no null_ordering at all
  } else {
    sort_config = {config.order_by, config.ordering, config.null_ordering};
  }
  const auto config_id = ctx.addSortConfig(sort_config);
  const auto run_dest = ctx.addInsertDestination(&runs, &storage);
  const auto out_dest = ctx.addInsertDestination(&output, &storage);
  auto *generate = new SortRunGenerationOperator(0, input, runs, run_dest, config_id, true);
  if (limit_runs) generate->setTopK(top_k);
  auto *merge = new SortMergeRunOperator(0, runs, output, out_dest, runs, run_dest, config_id, /*merge_factor=*/4, top_k, false);
  std::unique_ptr<RelationalOperator> g, m;
  if (use_foreman) {
    QueryPlan plan;
    const auto gi = plan.addRelationalOperator(generate);
    const auto mi = plan.addRelationalOperator(merge);
    plan.addDirectDependency(mi, gi, false);
    ForemanSingleNode foreman(&plan, &ctx, &storage, 4);
    foreman.run();
  } else {
    g.reset(generate); m.reset(merge);
    fetchAndExecuteWorkOrders(g.get(), &ctx, &storage);
    for (block_id b : ctx.getInsertDestination(run_dest)->getTouchedBlocks()) m->feedInputBlock(b, runs.getID(), 0);
    m->doneFeedingInputBlocks(runs.getID());
    fetchAndExecuteWorkOrders(m.get(), &ctx, &storage);
  }
  // every run is sorted and carries its tuples' null bits
  std::vector<std::size_t> run_sizes;
  const std::vector<Row> run_rows = readRows(ctx.getInsertDestination(run_dest)->getTouchedBlocks(), storage, &run_sizes);
  EXPECT_EQ(run_sizes.size(), static_cast<std::size_t>((kRows + kBlockRows - 1) / kBlockRows));
  if (!limit_runs || top_k == 0) EXPECT_EQ(run_rows.size(), static_cast<std::size_t>(kRows));
  std::size_t at = 0;
  for (std::size_t sz : run_sizes) {
    if (limit_runs && top_k != 0) EXPECT_TRUE(sz <= top_k);
    for (std::size_t i = at; i < at + sz; ++i) {
      if (i > at) EXPECT_TRUE(!Before(run_rows[i], run_rows[i - 1], config));
      ExpectSameTuple(run_rows[i], rows);
    }
    at += sz;
  }
  // the merged output: the first top_k tuples of the total order, every tuple intact
  const std::vector<Row> out = readRows(ctx.getInsertDestination(out_dest)->getTouchedBlocks(), storage, nullptr);
  std::vector<Row> want = rows;
  std::stable_sort(want.begin(), want.end(), [&](const Row &x, const Row &y) { return Before(x, y, config); });
  const std::size_t expect_n = top_k != 0 && top_k < want.size() ? top_k : want.size();
  EXPECT_EQ(out.size(), expect_n);
  std::vector<bool> seen(rows.size(), false);
  for (std::size_t i = 0; i < out.size() && i < expect_n; ++i) {
    // (ties among equal keys may come in any order — the runs arrive in any order: compare the keys position by position)
    EXPECT_TRUE(!Before(out[i], want[i], config) && !Before(want[i], out[i], config));
    ExpectSameTuple(out[i], rows);
    if (out[i].tid >= 0 && out[i].tid < static_cast<std::int32_t>(rows.size())) {
      EXPECT_TRUE(!seen[static_cast<std::size_t>(out[i].tid)]);   // a permutation: no tuple twice
      seen[static_cast<std::size_t>(out[i].tid)] = true;
    }
  }
}
}  // namespace

int main() {
  if (qsx_device_count() < 1) {
    std::fprintf(stderr, "sort_nulls_operator_test needs an MI355X: %s\n", qsx_status_string(QSX_ERR_NO_DEVICE));
    return 2;
  }
  const bool kAsc = true, kDesc = false, kFirst = true, kLast = false;
  const std::vector<Config> cases = {
      {{kN1}, {kAsc}, {kLast}},                                                   // 1Column_NullLast_Asc
      {{kN1}, {kAsc}, {kFirst}},                                                  // 1Column_NullFirst_Asc
      {{kN1}, {kDesc}, {kLast}},                                                  // 1Column_NullLast_Desc
      {{kN1}, {kDesc}, {kFirst}},                                                 // 1Column_NullFirst_Desc
      {{kN1, kN2, kN3}, {kAsc, kAsc, kAsc}, {kLast, kLast, kLast}},               // 3Column_NullLast_Asc
      {{kN1, kN2, kN3}, {kDesc, kDesc, kDesc}, {kLast, kLast, kLast}},            // 3Column_NullLast_Desc
      {{kN1, kN2, kN3}, {kAsc, kAsc, kAsc}, {kFirst, kFirst, kFirst}},            // 3Column_NullFirst_Asc
      {{kN1, kN2, kN3}, {kDesc, kDesc, kDesc}, {kFirst, kFirst, kFirst}},         // 3Column_NullFirst_Desc
      {{kN1, kN2, kN3}, {kAsc, kDesc, kAsc}, {kFirst, kLast, kLast}},             // 3Column_MixedNullOrdering_MixedOrdering
      {{kS10}, {kAsc}, {kLast}},                                                  // ORDER BY a CHAR(10)
      {{kS10, kN2}, {kDesc, kAsc}, {kLast, kFirst}},
      {{kS25, kTid}, {kAsc, kDesc}, {kFirst, kLast}},                             // a nullable CHAR(25), NULLs first
      {{kS25}, {kDesc}, {kLast}},
      {{kN2, kTid}, {kDesc, kAsc}, {}},                                           // no null_ordering: NULLs last
      {{kTid}, {kDesc}, {}},                                                      // ... and the plain entry points as before
  };
  const std::vector<Row> rows = makeRows();
  for (const bool use_foreman : {false, true}) {
    for (const Config &config : cases) {
      runCase(rows, config, 0, use_foreman, false);
      runCase(rows, config, 10, use_foreman, false);
      runCase(rows, config, 1000, use_foreman, true);    // the LIMIT in the runs too (SortRunGenerationOperator::setTopK)
    }
  }
  return finish("sort_nulls_operator_test");
}
