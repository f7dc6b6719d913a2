// closed_domain_test.cpp — the guarantee a closed aggregation state rests on (quickstep_amd/csrc/aggregate.hip:
// closed_key_bits, hash_table_cap): a COMPACT_KEY state whose key code has b <= 16 bits gets a table in which the WHOLE
// domain of 2^b codes leaves no run of kGlobalMaxProbes occupied slots.  Linear probing occupies the same slots in whatever
// order the keys arrive and the set only grows with the key set, so no subset of the domain can exhaust a probe sequence of
// global_find_or_insert: the state never overflows, and its finalize need not ask.  No device: the slots come from the
// library's own code_slot (mix64) and the capacities from its own sizing, through libqsx.so's test hooks.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/qsx.h"

extern "C" int qsx_debug_agg_table_geometry(const qsx_agg_config_t *config, int *out_closed_bits, unsigned long long *out_cap);
extern "C" unsigned long long qsx_debug_agg_closed_cap(int64_t est_groups, int key_bits);
extern "C" unsigned long long qsx_debug_agg_code_slot(unsigned long long code, unsigned long long cap);
extern "C" unsigned long long qsx_debug_agg_max_probes(void);

static int g_failures = 0;
static char g_case[64] = "";
#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_case); \
      ++g_failures;                                                                       \
    }                                                                                     \
  } while (0)

// Every code of [0, 2^bits) inserted by linear probing from the library's slot; the longest circular run of occupied slots.
static unsigned long long longest_run_of_full_domain(int bits, unsigned long long cap) {
  std::vector<unsigned char> occupied(cap, 0);
  for (unsigned long long code = 0; code < (1ull << bits); ++code) {
    unsigned long long s = qsx_debug_agg_code_slot(code, cap);
    if (s >= cap) return cap;   // (reported as a failure by the caller's bound)
    while (occupied[s]) s = (s + 1) & (cap - 1);
    occupied[s] = 1;
  }
  unsigned long long first_free = 0;
  while (first_free < cap && occupied[first_free]) ++first_free;
  if (first_free == cap) return cap;   // a full table
  unsigned long long longest = 0, run = 0;
  for (unsigned long long i = 1; i <= cap; ++i) {   // once around, starting behind a free slot
    if (occupied[(first_free + i) & (cap - 1)]) {
      ++run;
      if (run > longest) longest = run;
    } else {
      run = 0;
    }
  }
  return longest;
}

// A COMPACT_KEY plan over `nkeys` CHAR keys of `width` bytes (or one INT key when width == 0) and COUNT(*).
static qsx_agg_config_t plan(int nkeys, int width, int64_t est) {
  qsx_agg_config_t c;
  std::memset(&c, 0, sizeof(c));
  c.strategy = QSX_AGG_COMPACT_KEY;
  c.num_columns = nkeys;
  c.num_keys = nkeys;
  for (int k = 0; k < nkeys; ++k) {
    c.column_type[k] = width == 0 ? QSX_INT : QSX_CHAR;
    c.column_width[k] = width == 0 ? 4 : width;
    c.key_column[k] = k;
  }
  c.num_aggs = 1;
  c.aggs[0].fn = QSX_AGG_COUNT_STAR;
  c.est_groups = est;
  return c;
}

int main() {
  const unsigned long long max_probes = qsx_debug_agg_max_probes();
  CHECK(max_probes == 128);

  // every domain of 1..16 bits at the capacity a closed state over it gets (the smallest estimate: the domain decides)
  for (int bits = 1; bits <= 16; ++bits) {
    std::snprintf(g_case, sizeof(g_case), "b = %d", bits);
    const unsigned long long cap = qsx_debug_agg_closed_cap(1, bits);
    CHECK(cap != 0 && (cap & (cap - 1)) == 0);
    CHECK(cap >= (2ull << bits));
    const unsigned long long run = longest_run_of_full_domain(bits, cap);
    std::printf("b = %2d  cap = %7llu  longest run = %llu\n", bits, cap, run);
    CHECK(run < max_probes);
  }
  // a large estimate only makes the table larger
  std::snprintf(g_case, sizeof(g_case), "b = 16, est = 100000");
  CHECK(qsx_debug_agg_closed_cap(100000, 16) >= qsx_debug_agg_closed_cap(1, 16));
  CHECK(longest_run_of_full_domain(16, qsx_debug_agg_closed_cap(100000, 16)) < max_probes);
  // (why twice the domain: at 2^b slots the table is full, so a probe for an absent key would never end)
  CHECK(longest_run_of_full_domain(16, 1ull << 16) >= max_probes);

  // which plans are closed, and that their states get that capacity
  struct Case { const char *name; int nkeys, width; int64_t est; int want_bits; };
  const Case cases[] = {
      {"one CHAR(1)", 1, 1, 6, 8},           {"two CHAR(1) (Q1)", 2, 1, 6, 16},        {"one CHAR(2)", 1, 2, 1, 16},
      {"two CHAR(1), est 100000", 2, 1, 100000, 16}, {"three CHAR(1)", 3, 1, 1, 0},    {"CHAR(2) + CHAR(1)", 2, 2, 1, 0},
      {"one INT", 1, 0, 6, 0},
  };
  for (const Case &cs : cases) {
    std::snprintf(g_case, sizeof(g_case), "%s", cs.name);
    const qsx_agg_config_t c = plan(cs.nkeys, cs.width, cs.est);
    int bits = -1;
    unsigned long long cap = 0;
    CHECK(qsx_debug_agg_table_geometry(&c, &bits, &cap) == QSX_OK);
    CHECK(bits == cs.want_bits);
    CHECK(cap == qsx_debug_agg_closed_cap(cs.est, cs.want_bits));
    if (cs.want_bits != 0) {
      CHECK(cap >= (2ull << cs.want_bits));
      CHECK(longest_run_of_full_domain(cs.want_bits, cap) < max_probes);
    }
  }
  // an open plan keeps the capacity it had: 8 x the estimate + 1024, rounded up to a power of two
  CHECK(qsx_debug_agg_closed_cap(6, 0) == 2048);
  // the 8-bit domain already fits that table: a closed state over one CHAR(1) key is no larger than before
  CHECK(qsx_debug_agg_closed_cap(6, 8) == 2048);
  CHECK(qsx_debug_agg_closed_cap(6, 16) == (1ull << 17));

  if (g_failures == 0) {
    std::printf("[  PASSED  ] closed_domain_test\n");
    return 0;
  }
  std::printf("[  FAILED  ] closed_domain_test (%d failures)\n", g_failures);
  return 1;
}
