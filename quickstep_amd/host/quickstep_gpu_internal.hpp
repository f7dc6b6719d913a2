// quickstep_gpu_internal.hpp — what the host layer's translation units share and the public header does not show:
// the scratch buffer of a work order, the pooled allocations behind it, and the helpers more than one of the files uses.
// (host_runtime.cpp: errors, streams, pools; storage.cpp: catalog, blocks, compression, block images; query_context.cpp:
// predicates, destinations, aggregation state, LIP filters; select_build_operators.cpp, hash_join_operator.cpp,
// aggregation_sort_operators.cpp: the operators and their work orders; foreman.cpp: plan, Foreman, Worker threads.)
#ifndef QUICKSTEP_GPU_INTERNAL_HPP_
#define QUICKSTEP_GPU_INTERNAL_HPP_

#include "quickstep_gpu.hpp"

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>

namespace quickstep {
namespace host_internal {

// Scratch owned by one work order.  A device allocation of a few MB costs ~170 us (hipMalloc + hipFree, whatever the
// size; 0.7 us up to 64 KiB: tools/ubench/alloc_cost.hip) — more than the kernels of a work order over a 4 MB block take —
// and the stream-ordered pool is not an option on this stack (csrc/common.hpp, CallScratch).  So buffers above 64 KiB come
// from a per-thread cache of plain allocations in power-of-two size classes: a worker thread issues all its work on one
// stream, so a buffer handed back while its last kernel is still queued can be handed out again to the same thread —
// the next use is ordered behind it.  (A buffer built by one thread and consumed by another — DISTINCT chunks — is
// published after a stream synchronisation, like a storage block.)  The cache keeps at most kCacheBytes per thread.
void TrimBlockSlabPool();   // (host_runtime.cpp, BlockSlabPool)
void *TakePooled(std::size_t bytes, std::size_t *granted);
void GivePooled(void *p, std::size_t granted);
struct DeviceBuffer {
  // Every scratch buffer is cached per thread, the 8-byte count words of a work order included: a plain allocation is a
  // hipMalloc + hipFree pair, and hipFree waits for everything queued on the device — with eight Workers in flight a step of
  // the operators' bench stalled 6-9 ms on one of them every few steps (366 hipFree calls in 28 steps, 0.65 ms on average,
  // 9 ms at worst: rocprofv3 --hip-trace).  (Until round 5 only buffers above 64 KiB were cached.)
  static constexpr std::size_t kCacheFrom = 1;
  static constexpr std::size_t kCacheBytes = std::size_t(2) << 30;
  // (device, size class): a thread that moves to another device (qsx_set_current_device) must not be handed the other
  // device's memory — Worker threads stay on one device, callers of the layer need not
  static std::pair<int, std::size_t> classKey(std::size_t size_class) {
    int device = 0;
    (void)qsx_current_device(&device);
    return std::make_pair(device, size_class);
  }
  struct Cache {
    std::map<std::pair<int, std::size_t>, std::vector<void *>> free_by_class;
    std::size_t bytes = 0;
    ~Cache() {
      for (auto &cls : free_by_class) for (void *p : cls.second) qsx_device_free(p);
    }
  };
  static Cache &cache() {
    thread_local Cache c;
    return c;
  }
  static void trimThisThread() {
    Cache &c = cache();
    for (auto &cls : c.free_by_class) {
      for (void *q : cls.second) qsx_device_free(q);
      cls.second.clear();
    }
    c.bytes = 0;
  }
  void *ptr = nullptr;
  std::pair<int, std::size_t> class_key{0, 0};   // (device the buffer was allocated on, size class): where a release files it
  std::size_t size_class = 0;   // 0: a plain allocation of its own
  std::size_t pooled = 0;       // != 0: from the shared pool (its size class there)
  // (1 MiB, 32 MiB until late in round 5: the per-block bitmaps of a run — two sets of 16 MiB — were cached per thread, and every
  // Worker paid ~7 ms of first allocations the first time a work order of that kind came its way, thirty steps into a run at times)
  static constexpr std::size_t kSharedFrom = std::size_t(1) << 20;
  static bool cacheEnabled() {   // QSX_HOST_SCRATCH_CACHE=0: every buffer a plain allocation (debugging)
    static const bool on = []() {
      const char *e = std::getenv("QSX_HOST_SCRATCH_CACHE");
      return e == nullptr || e[0] != '0';
    }();
    return on;
  }
  explicit DeviceBuffer(std::size_t bytes) {
    if (bytes >= kSharedFrom && cacheEnabled()) {
      // pair lists / operand columns of a run of blocks: hundreds of MB — from the process-wide pool of the output blocks,
      // not one cached copy per Worker thread (whichever thread happens to pick the join next would allocate its own)
      ptr = TakePooled(bytes, &pooled);
      return;
    }
    if (bytes >= kCacheFrom && cacheEnabled()) {
      size_class = bytes <= 64 * 1024 ? 256 : 128 * 1024;   // (small ones in classes of their own: 256 B, 512 B, ...)
      while (size_class < bytes) size_class *= 2;
      Cache &c = cache();
      // (the key is taken once, here: a thread that changes its device between constructor and destructor must still file
      // the buffer under the device that owns the memory)
      class_key = classKey(size_class);
      auto it = c.free_by_class.find(class_key);
      if (it != c.free_by_class.end() && !it->second.empty()) {
        ptr = it->second.back();
        it->second.pop_back();
        c.bytes -= size_class;
        return;
      }
      if (qsx_device_alloc(size_class, &ptr) != QSX_OK) {
        // this thread's cached buffers, the pooled block allocations and what libqsx.so keeps for this thread go back first
        // (the library has already called HostOutOfMemoryHook once from inside qsx_device_alloc)
        trimThisThread();
        TrimBlockSlabPool();
        (void)qsx_trim_scratch(nullptr);
        CheckStatus(qsx_device_alloc(size_class, &ptr), "qsx_device_alloc");
      }
      return;
    }
    CheckStatus(qsx_device_alloc(bytes ? bytes : 8, &ptr), "qsx_device_alloc");
  }
  ~DeviceBuffer() {
    if (pooled != 0) {
      (void)qsx_stream_synchronize(CurrentStream());   // another thread may take it next: this thread's queued work first
      GivePooled(ptr, pooled);
      return;
    }
    if (size_class != 0) {
      Cache &c = cache();
      if (c.bytes + size_class <= kCacheBytes) {
        c.free_by_class[class_key].push_back(ptr);
        c.bytes += size_class;
        return;
      }
    }
    qsx_device_free(ptr);
  }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
};

std::int64_t ReadCount(const void *dev_count);
std::uint64_t NowMicros();

// A pointer from qsx_device_alloc that a callee hands out (the bitmaps of a LIPFilterAdaptiveProber), freed at scope exit.
struct DeviceAllocation {
  void *ptr = nullptr;
  DeviceAllocation() = default;
  ~DeviceAllocation() { qsx_device_free(ptr); }
  DeviceAllocation(const DeviceAllocation &) = delete;
  DeviceAllocation &operator=(const DeviceAllocation &) = delete;
};

// The selected tuples of a run of blocks, block after block, compacted into ONE output block of `destination` with room for
// `capacity` tuples (one qsx_compact_gather_blocks): output attribute i takes attribute selection[i], bitmaps[b] selects block
// b's tuples (nullptr as a whole: every tuple).  want_tids: also the tuple id of every output tuple — base_tids[b] + row, or
// the run-global row number without base_tids — for the null bits that follow the values.  Waits for the count (ReadCount
// on count_dev); the block is the caller's to return.  The workspace and the tuple ids travel with the result: scratch of a
// megabyte waits for the stream when it goes, so it goes when the caller is done, not in between the caller's launches.
struct CompactedRun {
  BlockReference out;
  block_id out_id = 0;
  std::int64_t written = 0;
  std::unique_ptr<DeviceBuffer> workspace, tids;
};
inline CompactedRun CompactRunInto(const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows,
                                   const std::vector<attribute_id> &selection, const std::uint64_t *const *bitmaps,
                                   const std::int32_t *base_tids, std::int64_t capacity, bool want_tids,
                                   InsertDestination *destination, void *count_dev) {
  CompactedRun run;
  const std::size_t nb = blocks.size(), nc = selection.size();
  run.out = destination->getBlockForInsertion(capacity > 0 ? capacity : 1, &run.out_id);
  std::vector<const void *> src(nb * nc);
  std::vector<void *> dst;
  std::vector<std::int32_t> widths;
  for (std::size_t i = 0; i < nc; ++i) {
    dst.push_back(run.out->stripe(static_cast<attribute_id>(i)));
    widths.push_back(blocks.front()->getRelation().getAttributeType(selection[i]).width);
    for (std::size_t b = 0; b < nb; ++b) src[b * nc + i] = blocks[b]->stripe(selection[i]);
  }
  const std::size_t ws_bytes = qsx_compact_blocks_workspace_bytes(static_cast<std::int64_t>(nb), rows.data());
  run.workspace.reset(new DeviceBuffer(ws_bytes + 8));
  if (want_tids) run.tids.reset(new DeviceBuffer(static_cast<std::size_t>(capacity > 0 ? capacity : 1) * 4 + 8));
  CheckStatus(qsx_compact_gather_blocks(static_cast<int>(nc), widths.data(), static_cast<std::int64_t>(nb), rows.data(), src.data(), bitmaps,
                                        want_tids ? base_tids : nullptr, dst.data(),
                                        want_tids ? static_cast<std::int32_t *>(run.tids->ptr) : nullptr,
                                        static_cast<std::int64_t *>(count_dev), run.workspace->ptr, ws_bytes, CurrentStream()),
              "qsx_compact_gather_blocks");
  run.written = ReadCount(count_dev);   // (synchronises the stream: the block's tuples are written)
  return run;
}

// NULL handling shared by the aggregation state and the operators (storage.cpp)
std::unique_ptr<DeviceBuffer> NotNullFilter(const StorageBlock &block, const std::vector<attribute_id> &attrs, const std::uint64_t *filter);
void GatherBlockNulls(const StorageBlock &block, attribute_id attr, const void *tids, std::int64_t n, std::uint64_t *dst);
// derived: nullptr, or per output attribute a null bitmap over the block's tuples that is not an attribute's (a CASE's) or nullptr
void ProjectNullBitmaps(const StorageBlock &block, const std::vector<attribute_id> &selection, const void *bitmap,
                        std::int64_t num_selected, StorageBlock *out, const std::vector<const std::uint64_t *> *derived = nullptr);

// ---- the join key of a block / of a run of blocks as the join table sees it (BuildHash and HashJoin work orders) ----
// The single key column the join table sees for one block: the attribute's stripe, or — for a
// composite key — the LONG fold of the components (qsx_join_key_pack; the QueryContext creates
// the table of a composite key with key type kLong).  `exact` is false when the fold is the
// reference's composite hash and joined pairs still need their components compared.
// A CHAR(n <= 8) key attribute of `block` as a LONG stripe (qsx_join_key_pack_char); wider strings are not join keys here.
inline std::unique_ptr<DeviceBuffer> CharKeyAsLong(const StorageBlock &block, attribute_id a) {
  const Type &t = block.getRelation().getAttributeType(a);
  if (t.width > 8) throw ExecutionError("join key CHAR(n): n > 8 is not supported", QSX_ERR_UNSUPPORTED);
  std::unique_ptr<DeviceBuffer> out(new DeviceBuffer(static_cast<std::size_t>(block.numTuples()) * 8 + 8));
  CheckStatus(qsx_join_key_pack_char(block.stripe(a), t.width, block.numTuples(), static_cast<std::int64_t *>(out->ptr), CurrentStream()),
              "qsx_join_key_pack_char");
  return out;
}

// VARCHAR is no join key of this layer (alone or as a component): refused before a key stripe is made of it.
inline void RefuseVarCharJoinKey(const CatalogRelation &relation, const std::vector<attribute_id> &attrs) {
  for (attribute_id a : attrs) {
    if (relation.getAttributeType(a).id == kVarChar) throw ExecutionError("a VARCHAR attribute as a join key", QSX_ERR_UNSUPPORTED);
  }
}

struct JoinKeys {
  const void *ptr = nullptr;
  bool exact = true;
  std::unique_ptr<DeviceBuffer> packed;
  std::vector<std::unique_ptr<DeviceBuffer>> char_keys;
  JoinKeys(const StorageBlock &block, const std::vector<attribute_id> &attrs) {
    RefuseVarCharJoinKey(block.getRelation(), attrs);
    if (attrs.size() == 1) {
      if (block.getRelation().getAttributeType(attrs.front()).id == kChar) {
        char_keys.push_back(CharKeyAsLong(block, attrs.front()));
        ptr = char_keys.back()->ptr;
        return;
      }
      ptr = block.stripe(attrs.front());
      return;
    }
    std::vector<const void *> cols;
    std::vector<std::int32_t> types;
    for (attribute_id a : attrs) {
      if (block.getRelation().getAttributeType(a).id == kChar) {
        char_keys.push_back(CharKeyAsLong(block, a));
        cols.push_back(char_keys.back()->ptr);
        types.push_back(kLong);
        continue;
      }
      cols.push_back(block.stripe(a));
      types.push_back(block.getRelation().getAttributeType(a).id);
    }
    packed.reset(new DeviceBuffer(static_cast<std::size_t>(block.numTuples()) * 8 + 8));
    int is_exact = 0;
    CheckStatus(qsx_join_key_pack(static_cast<int>(cols.size()), cols.data(), types.data(), block.numTuples(),
                                  static_cast<std::int64_t *>(packed->ptr), &is_exact, CurrentStream()),
                "qsx_join_key_pack");
    ptr = packed->ptr;
    exact = is_exact != 0;
  }
};

// The key stripes of a run of blocks as the join table sees them: the attribute's stripes, or — composite key — one stripe of
// packed keys for the whole run (qsx_join_key_pack_blocks), block b's keys at row first_rows[b] of it.
//
// A single INT / LONG key attribute that a block holds COMPRESSED (CompressedColumnStore: truncated values or dictionary codes,
// each block its own choice) is presented as it lies — ptr[b] = the code stripe, code_width[b] / dictionary[b] its coding — for
// the *_blocks_coded entry points (include/qsx.h qsx_key_coding_t): the kernels widen or look up the codes themselves, the
// attribute is never decoded into a stripe of values (StorageBlock::stripe would on first use).  coding() is nullptr when no
// block of the run is compressed in its key.
struct RunJoinKeys {
  std::vector<const void *> ptr;          // per block
  std::vector<std::int32_t> code_width;   // per block: 0 = values
  std::vector<const void *> dictionary;   // per block: nullptr = values / truncated values
  bool coded = false;
  bool exact = true;
  std::unique_ptr<DeviceBuffer> packed;
  std::vector<std::unique_ptr<DeviceBuffer>> char_keys;
  qsx_key_coding_t coding_{nullptr, nullptr};
  const qsx_key_coding_t *coding() const { return coded ? &coding_ : nullptr; }
  RunJoinKeys(const std::vector<BlockReference> &blocks, const std::vector<attribute_id> &attrs, const std::vector<std::int64_t> &rows) {
    const CatalogRelation &relation = blocks.front()->getRelation();
    RefuseVarCharJoinKey(relation, attrs);
    if (attrs.size() == 1) {
      const TypeID key_type = relation.getAttributeType(attrs.front()).id;
      for (const BlockReference &b : blocks) {
        const CompressedAttribute *c = (key_type == kInt || key_type == kLong) ? b->compressedAttribute(attrs.front()) : nullptr;
        if (key_type == kChar) {
          char_keys.push_back(CharKeyAsLong(*b, attrs.front()));
          ptr.push_back(char_keys.back()->ptr);
        } else if (c != nullptr && b->numTuples() > 0) {
          ptr.push_back(c->codes);
          coded = true;
        } else {
          ptr.push_back(b->stripe(attrs.front()));
          c = nullptr;
        }
        code_width.push_back(c != nullptr && key_type != kChar ? c->code_width : 0);
        dictionary.push_back(c != nullptr && key_type != kChar && c->kind == CompressedAttribute::kDictionary ? c->dictionary : nullptr);
      }
      coding_.block_code_width = code_width.data();
      coding_.block_dictionaries = dictionary.data();
      return;
    }
    std::vector<const void *> cols;
    std::vector<std::int32_t> types;
    for (attribute_id a : attrs) types.push_back(relation.getAttributeType(a).id == kChar ? static_cast<std::int32_t>(kLong) : relation.getAttributeType(a).id);
    // (a component that a block holds compressed is packed from its code stripe: qsx_join_key_pack_blocks_coded)
    std::vector<std::int32_t> widths;
    std::vector<const void *> dicts;
    std::int64_t total = 0;
    for (std::size_t b = 0; b < blocks.size(); ++b) {
      for (attribute_id a : attrs) {
        const TypeID id = relation.getAttributeType(a).id;
        const CompressedAttribute *c = (id == kInt || id == kLong) && blocks[b]->numTuples() > 0 ? blocks[b]->compressedAttribute(a) : nullptr;
        if (id == kChar) {
          char_keys.push_back(CharKeyAsLong(*blocks[b], a));
          cols.push_back(char_keys.back()->ptr);
        } else if (c != nullptr) {
          cols.push_back(c->codes);
        } else {
          cols.push_back(blocks[b]->stripe(a));
        }
        widths.push_back(c != nullptr ? c->code_width : 0);
        dicts.push_back(c != nullptr && c->kind == CompressedAttribute::kDictionary ? c->dictionary : nullptr);
      }
      total += rows[b];
    }
    packed.reset(new DeviceBuffer(static_cast<std::size_t>(total) * 8 + 8));
    int is_exact = 0;
    CheckStatus(qsx_join_key_pack_blocks_coded(static_cast<int>(attrs.size()), types.data(), static_cast<std::int64_t>(blocks.size()), rows.data(),
                                               cols.data(), widths.data(), dicts.data(), static_cast<std::int64_t *>(packed->ptr), &is_exact,
                                               CurrentStream()),
                "qsx_join_key_pack_blocks");
    exact = is_exact != 0;
    std::int64_t at = 0;
    for (std::size_t b = 0; b < blocks.size(); ++b) {
      ptr.push_back(static_cast<const std::int64_t *>(packed->ptr) + at);
      at += rows[b];
    }
  }
};

}  // namespace host_internal
using namespace host_internal;   // (this header is included by the layer's own sources only)

void CheckRepartition(const char *op, bool has_repartition, const InsertDestination *dest);   // (query_context.cpp)

// A predicate over a run of blocks (query_context.cpp): per-block TupleIdSequences in two device allocations.
struct RunMatches {
  std::unique_ptr<DeviceBuffer> set_a, set_b, counts;
  std::vector<std::uint64_t *> bitmaps;   // block b's bitmap under the whole conjunction
  std::vector<std::unique_ptr<DeviceBuffer>> scratch;   // code sets, a tree's leaf bitmaps: read by queued kernels
};
// LIKE / NOT LIKE terms (query_context.cpp).  CheckLikeTerm: QSX_ERR_UNSUPPORTED unless the term is CHAR(n) or VARCHAR(n)
// attribute against a pattern literal of at most QSX_MAX_LIKE_PATTERN bytes.  SelectCharTerm: a CHAR(n) attribute against a string literal over a
// plain stripe of n values — qsx_select_like for the two, qsx_select_cmp_char for the six orderings (whose ComparisonID is
// the ABI's op).
inline bool IsLikeComparison(ComparisonID c) { return c == ComparisonID::kLike || c == ComparisonID::kNotLike; }
// CHAR(n) and VARCHAR(n): outside an adopted variable-length dictionary both are n-byte NUL-padded fields (Type::VarChar), so
// a plain stripe of either goes through the CHAR(n) kernels.
inline bool IsTextType(TypeID id) { return id == kChar || id == kVarChar; }
void CheckLikeTerm(const ComparisonPredicate &term, const Type &type);
// attribute OP attribute as a conjunct of a Select's, an aggregation's or a WHEN's predicate (query_context.cpp): throws unless both
// attributes are `relation`'s own (no build side: QSX_ERR_INVALID_ARGUMENT), numeric with numeric or DATE with DATE, no LIKE
// (QSX_ERR_UNSUPPORTED).
void CheckAttributeComparison(const ComparisonPredicate &term, const CatalogRelation &relation);
// A term over a unary operation (ComparisonPredicate::operand).  CheckUnaryTerm: the operand is EXTRACT / SUBSTRING of an attribute
// that is no VARCHAR, the comparison no LIKE, no rhs_attribute; returns the operand's type (INT, CHAR(m)).  CheckUnaryLiteral: a
// literal of that type.
Type CheckUnaryTerm(const ComparisonPredicate &term, const CatalogRelation &relation);
void CheckUnaryLiteral(const Type &operand_type, const TypedLiteral &literal);
void SelectCharTerm(const ComparisonPredicate &term, const void *stripe, int width, std::int64_t n, const std::uint64_t *filter,
                    std::uint64_t *out_bitmap, std::int64_t *out_count);
// ONE evaluator turns a term into bitmaps (query_context.cpp, SelectTerm over a BlockSpan) and ONE function evaluates a tree
// (EvaluateTree); Predicate::getMatchesForBlock hands them a single block (the qsx_select_* entry points), RunPredicateMatches a
// run (the _blocks entry points, also for a run of one block).  What differs between the two on purpose is marked where it
// happens: a single block scans an every-code / no-code rewrite on a compressed sort column where a run searches; a unary term
// on a compressed attribute without a dictionary it can be evaluated over (truncated values, a date dictionary that is not
// 8-byte aligned) reads the decoded stripe() per block, and RunPredicateCovers keeps that shape off the run path; an IN list
// over truncated codes that reaches the evaluator is QSX_ERR_INVALID_ARGUMENT, IN on VARCHAR QSX_ERR_UNSUPPORTED; an empty
// single block has no compressed attribute and takes the plain entry with n = 0.
// RunPredicateCovers: can the run forms evaluate `predicate` over these blocks in one launch per term?  RunPredicateMatches: do so.
bool RunPredicateCovers(const Predicate &predicate, const std::vector<BlockReference> &blocks);
void RunPredicateMatches(const Predicate &predicate, const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows,
                         const std::uint64_t *const *in_filters, RunMatches *out);


// A Scalar::kCaseExpression ready to be evaluated (query_context.cpp): the branch values flattened into ONE program — integer
// subtrees as integer instructions when integer_arithmetic, a subexpression two branches share once — and the qsx_case_desc_t
// over it.  QSX_ERR_UNSUPPORTED: no or more than QSX_MAX_CASE_WHENS WHENs, a CASE nested in a branch, a CHAR-typed branch.
struct CaseEvaluator {
  CaseEvaluator(const ScalarPtr &scalar, const CatalogRelation &relation, bool integer_arithmetic);
  ScalarPtr scalar;
  std::vector<attribute_id> attrs;                 // program column -> attribute
  std::vector<std::int32_t> types;
  std::vector<qsx_expr_instr_t> instrs;
  double consts[QSX_MAX_CONSTS] = {};
  qsx_case_desc_t desc;
  TypeID out_type = kDouble;
  bool has_null_branch = false;
  bool nullable = false;                           // a NULL branch, or a nullable operand attribute: the value can be NULL
  int width() const { return out_type == kInt ? 4 : 8; }
  // The CASE over the whole block: n values into out_dev and, when `nullable`, the null bitmap into out_nulls_dev.  The WHEN
  // bitmaps live until the call's wait: this synchronises.
  void evalBlock(const StorageBlock &block, void *out_dev, std::uint64_t *out_nulls_dev) const;
  // The same over a run in one launch per WHEN term and one qsx_eval_case_blocks; false (nothing done) when the run forms do
  // not cover it: a value that can be NULL, a WHEN RunPredicateCovers refuses, a block with a null bitmap on an operand.
  // The bitmaps stay in `keep` until the caller has waited for the stream.
  bool evalBlocks(const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows, void *const *outs,
                  std::vector<std::unique_ptr<RunMatches>> *keep) const;
};

// A Scalar::kUnaryExpression ready to be evaluated (query_context.cpp): EXTRACT over a DATE attribute or SUBSTRING over a
// CHAR(n) attribute.  QSX_ERR_UNSUPPORTED: an operand that is not an attribute of that type, a unit a Date does not have;
// QSX_ERR_INVALID_ARGUMENT: a SUBSTRING window the C ABI refuses.
struct UnaryEvaluator {
  UnaryEvaluator(const ScalarPtr &scalar, const CatalogRelation &relation);
  ScalarPtr scalar;
  attribute_id operand = kInvalidAttributeID;   // the result takes this attribute's null bitmap
  Type operand_type = Type::Int();
  Type result = Type::Int();                    // INT or CHAR(m), nullable when the operand is
  typedef std::vector<std::unique_ptr<DeviceBuffer>> Scratch;
  // A dictionary-coded DATE that has not been decoded yet is not decoded here either: EXTRACT runs over the block's dictionary
  // (num_codes entries, and a 0 behind them for the NULL code num_codes, which qsx_decode_codes looks up like any other) and the
  // code stripe is mapped through the result.  A coded CHAR operand of SUBSTRING goes through stripe(): qsx_decode_codes
  // knows 4- and 8-byte values only.
  bool extractsOnCodes(const StorageBlock &block) const;
  // n results into out_dev, stream-ordered; scratch the device work reads lives in `keep` until the caller has waited.
  // Returns whether the block's dictionary was used.
  bool evalBlock(const StorageBlock &block, void *out_dev, Scratch *keep) const;
  // The same over a run: one _blocks launch for the blocks that present a stripe, the dictionary form block by block.
  // Returns the number of blocks whose dictionary was used.
  std::int64_t evalBlocks(const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows, void *const *outs,
                          Scratch *keep) const;
};

}  // namespace quickstep

#endif  // QUICKSTEP_GPU_INTERNAL_HPP_
