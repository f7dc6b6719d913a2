// predicate_tree.hip — the AND / OR / NOT nodes of a predicate tree, evaluated over the bitmaps of its leaves in one launch
// (qsx_bitmap_eval, qsx_bitmap_eval_blocks).  The leaves are what the select kernels write (select.hip, like.hip: comparisons,
// IN lists, LIKE, code sets, sorted-column ranges) and null bitmaps.
//
// Replaces the recursion of ConjunctionPredicate / DisjunctionPredicate / NegationPredicate::getAllMatches
// (expressions/predicate/DisjunctionPredicate.cpp:109-157: union of the children's matches; NegationPredicate.cpp:70-90: the
// child's matches inverted inside the filter and the existence map).  Two-valued like the reference: NOT over a leaf that is
// false for a NULL operand selects the row (include/qsx.h, qsx_bitmap_eval).
//
// The tree arrives as a postfix program.  A lane evaluates one bitmap word; the program counter and the stack pointer are the
// same in every lane.  The stack is in LDS, indexed by that wave-uniform stack pointer, with its top in a register: no indexed
// private array, no scratch memory.  The program and the leaf addresses lie in a table of 64-bit words in device memory, read
// with wave-uniform indices; a lane's words of the leaves wait in LDS for the program to push them.
#include "common.hpp"
#include "block_runs.hpp"

namespace qsx {
namespace predicate_tree {

constexpr int kBlock = 128;
constexpr int kTileWords = kBlock;                   // bitmap words a workgroup takes at a time, one per lane: 8192 rows
constexpr long long kTileRows = static_cast<long long>(kTileWords) * 64;
constexpr int kDepth = QSX_MAX_BOOL_DEPTH;
// LDS of a workgroup: a column of num_leaves + kDepth - 1 words per lane (the leaves' words, then the covered part of the stack)
static size_t eval_lds_bytes(int num_leaves) { return static_cast<size_t>(num_leaves + kDepth - 1) * kBlock * sizeof(uint64_t); }   // <= 39 KiB

// Program words: [0] number of instructions, then the codes.
// One tile: words [word0, word0 + kTileWords) of a block of n rows, one word per lane.  `program`, `leaves` (num_leaves
// addresses) and every other argument are uniform over the workgroup.
// A lane first brings its word of EVERY leaf into its own column of LDS: the loads are issued one behind the other and wait for
// nothing.  The stack lives there too, behind the leaves: the value on top in a register, the covered ones at an index that is
// the same in every lane — a push is one ds_write, a binary operator one ds_read.  (The alternative the issue names, the stack in
// registers behind wave-uniform selects, costs 28 v_cndmask per push and per operator; measured, it is bound by them: 0.13-0.15 ms
// per 100 M rows and 20 leaves whether the leaves come by 8- or 16-byte loads, from LDS or straight from memory.)  A lane reads back only what it wrote
// itself, so no barrier stands anywhere.
__device__ __forceinline__ void eval_tile(const long long *__restrict__ program, const long long *__restrict__ leaves, int num_leaves, int64_t n,
                                          const uint64_t *__restrict__ filter, uint64_t *__restrict__ out, int64_t word0, uint64_t *s_words,
                                          unsigned long long &count) {
  const int64_t num_words = (n + 63) >> 6;
  const int64_t at = word0 + threadIdx.x;
  const bool have = at < num_words;
  const int64_t safe = have ? at : num_words - 1;   // clamped, not guarded: a lane behind the last word computes and drops it
  uint64_t *const mine = s_words + threadIdx.x;     // leaf k at mine[k * kBlock], stack level d at mine[(num_leaves + d) * kBlock]
#pragma unroll 8
  for (int k = 0; k < num_leaves; ++k) {
    const uint64_t *leaf = as_global(reinterpret_cast<const uint64_t *>(leaves[k]));
    // an absent leaf is the all-zero bitmap: the load goes to a valid word all the same (the output's, whose value is dropped),
    // so that the loop holds no branch and the loads of its iterations overlap
    const uint64_t v = load_global_nt(&(leaf != nullptr ? leaf : static_cast<const uint64_t *>(out))[safe]);
    mine[k * kBlock] = leaf != nullptr ? v : 0ull;
  }
  uint64_t *const stack = mine + num_leaves * kBlock;
  uint64_t top = 0;
  int sp = 0;   // values on the stack: the last in `top`, the others at stack[0 .. sp - 2]
  const int num_instrs = static_cast<int>(program[0]);
  for (int pc = 0; pc < num_instrs; ++pc) {
    const int code = static_cast<int>(program[1 + pc]);
    if (code >= 0) {
      if (sp > 0) stack[(sp - 1) * kBlock] = top;   // the old top is covered (sp <= kDepth - 1 here: the host checked the depth)
      top = mine[code * kBlock];
      ++sp;
    } else if (code == QSX_BOOL_NOT) {
      top = ~top;
    } else {
      const uint64_t a = stack[(sp - 2) * kBlock];   // the value under the top (sp >= 2: the host checked for underflow)
      top = code == QSX_BOOL_AND ? (a & top) : (a | top);
      --sp;
    }
  }
  if (!have) return;
  uint64_t r = top;
  if (filter != nullptr) r &= filter[at];
  const int tail = static_cast<int>(n & 63);
  if (at == num_words - 1 && tail != 0) r &= ~0ull << (64 - tail);   // bits behind row n stay zero, under NOT too
  out[at] = r;
  count += __popcll(r);
}

// table: the program, then num_leaves leaf addresses at word `leaves_at`.
__global__ __launch_bounds__(kBlock) void bitmap_eval_kernel(const long long *__restrict__ table, long long leaves_at, int num_leaves, int64_t n,
                                                            const uint64_t *__restrict__ filter, uint64_t *__restrict__ out,
                                                            unsigned long long *__restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_leaves[];
  const int64_t num_tiles = (((n + 63) >> 6) + kTileWords - 1) / kTileWords;
  unsigned long long count = 0;
  for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    eval_tile(table, table + leaves_at, num_leaves, n, filter, out, tile * kTileWords, s_leaves, count);
  }
  if (out_count != nullptr) {
    __shared__ unsigned long long block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    count = wave_reduce_add(count);
    if (lane_id() == 0 && count != 0) atomicAdd(&block_count, count);
    __syncthreads();
    if (threadIdx.x == 0 && block_count != 0) atomicAdd(out_count, block_count);
  }
}

// Over a run of blocks (block_runs.hpp; the table's `in` array is unused): the program lies behind the run table at word
// `program_at`, leaf k of block b at word leaves_at + b * num_leaves + k.  A workgroup takes a contiguous range of the run's
// tiles and adds its matches to a block's counter when it moves on to another block (as like_runs_kernel).
__global__ __launch_bounds__(kBlock) void bitmap_eval_runs_kernel(const long long *__restrict__ runs, long long program_at, long long leaves_at,
                                                                 int num_leaves, unsigned long long *__restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_leaves[];
  const int lane = lane_id();
  const long long num_tiles = runs[2];
  const int first = static_cast<int>(num_tiles * blockIdx.x / gridDim.x);
  const int end = static_cast<int>(num_tiles * (blockIdx.x + 1) / gridDim.x);
  unsigned long long count = 0;
  int counted_block = -1;
  for (int tile = first; tile < end; ++tile) {
    const RunTile at = run_locate(runs, tile);
    if (at.block != counted_block) {
      if (out_counts != nullptr && counted_block >= 0) {
        count = wave_reduce_add(count);
        if (lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
      }
      count = 0;
      counted_block = at.block;
    }
    eval_tile(runs + program_at, runs + leaves_at + static_cast<long long>(at.block) * num_leaves, num_leaves, run_rows(runs, at.block),
              run_filter(runs, at.block), run_out<uint64_t>(runs, at.block), static_cast<int64_t>(at.tile_in_block) * kTileWords, s_leaves, count);
  }
  if (out_counts != nullptr && counted_block >= 0) {
    count = wave_reduce_add(count);
    if (lane == 0 && count != 0) atomicAdd(&out_counts[counted_block], count);
  }
}

// A well-formed program: known codes, leaves below num_leaves, no underflow, never more than QSX_MAX_BOOL_DEPTH values,
// exactly one at the end.
static bool program_ok(int num_leaves, int num_instrs, const int32_t *program) {
  if (num_leaves < 1 || num_leaves > QSX_MAX_BOOL_LEAVES || num_instrs < 1 || num_instrs > QSX_MAX_BOOL_INSTRS || program == nullptr) return false;
  int depth = 0;
  for (int pc = 0; pc < num_instrs; ++pc) {
    const int code = program[pc];
    if (code >= 0) {
      if (code >= num_leaves || ++depth > QSX_MAX_BOOL_DEPTH) return false;
    } else if (code == QSX_BOOL_NOT) {
      if (depth < 1) return false;
    } else if (code == QSX_BOOL_AND || code == QSX_BOOL_OR) {
      if (depth < 2) return false;
      --depth;
    } else {
      return false;
    }
  }
  return depth == 1;
}

// Do two bitmaps of n bits share a byte?  (An absent one shares none.)
static bool bitmaps_overlap(const uint64_t *a, const uint64_t *b, int64_t n) {
  if (a == nullptr || b == nullptr || n <= 0) return false;
  const uintptr_t bytes = static_cast<uintptr_t>((n + 63) / 64) * 8, pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace predicate_tree
}  // namespace qsx

using namespace qsx;
using namespace qsx::predicate_tree;

extern "C" {

int qsx_bitmap_eval(int num_leaves, const uint64_t *const *leaves_dev, int num_instrs, const int32_t *program, int64_t n,
                    const uint64_t *filter_dev, uint64_t *out_bitmap_dev, int64_t *out_count_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (n < 0 || leaves_dev == nullptr || !program_ok(num_leaves, num_instrs, program) || (n > 0 && out_bitmap_dev == nullptr)) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < num_leaves; ++k) {
    if (bitmaps_overlap(leaves_dev[k], out_bitmap_dev, n)) return QSX_ERR_INVALID_ARGUMENT;   // the output must not overlap an input
  }
  if (bitmaps_overlap(filter_dev, out_bitmap_dev, n)) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  if (out_count_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return QSX_OK;
  long long words[1 + QSX_MAX_BOOL_INSTRS + QSX_MAX_BOOL_LEAVES];
  words[0] = num_instrs;
  for (int pc = 0; pc < num_instrs; ++pc) words[1 + pc] = program[pc];
  const long long leaves_at = 1 + num_instrs;
  for (int k = 0; k < num_leaves; ++k) words[leaves_at + k] = RunTable::word_of(leaves_dev[k]);
  const long long *table = nullptr;
  const int rc = staged_table(s, words, sizeof(long long) * static_cast<size_t>(leaves_at + num_leaves), &table);
  if (rc != QSX_OK) return rc;
  const int64_t tiles = (((n + 63) >> 6) + kTileWords - 1) / kTileWords;
  hipLaunchKernelGGL(bitmap_eval_kernel, dim3(grid_for(tiles, 1)), dim3(kBlock), eval_lds_bytes(num_leaves), s, table, leaves_at, num_leaves, n, filter_dev, out_bitmap_dev,
                     reinterpret_cast<unsigned long long *>(out_count_dev));
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

int qsx_bitmap_eval_blocks(int num_leaves, int num_instrs, const int32_t *program, int64_t num_blocks, const int64_t *block_rows,
                           const uint64_t *const *block_leaves, const uint64_t *const *block_filters, uint64_t *const *block_out_bitmaps,
                           int64_t *out_counts_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (num_blocks < 0 || !program_ok(num_leaves, num_instrs, program) ||
      (num_blocks > 0 && (block_rows == nullptr || block_leaves == nullptr || block_out_bitmaps == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (!run_blocks_ok(num_blocks, block_rows, nullptr, reinterpret_cast<const void *const *>(block_out_bitmaps))) return QSX_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < num_blocks; ++b) {
    if (block_rows[b] == 0) continue;
    for (int k = 0; k < num_leaves; ++k) {
      if (bitmaps_overlap(block_leaves[b * num_leaves + k], block_out_bitmaps[b], block_rows[b])) return QSX_ERR_INVALID_ARGUMENT;
    }
    if (block_filters != nullptr && bitmaps_overlap(block_filters[b], block_out_bitmaps[b], block_rows[b])) return QSX_ERR_INVALID_ARGUMENT;
  }
  if (num_blocks == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  if (out_counts_dev != nullptr) QSX_HIP_TRY(hipMemsetAsync(out_counts_dev, 0, sizeof(int64_t) * static_cast<size_t>(num_blocks), s));
  RunTable table;
  const long long tiles = table.index(kTileRows, num_blocks, block_rows, kRunPlainArrays - 1);   // (no `in` stripe: the leaves follow)
  if (tiles < 0) return QSX_ERR_INVALID_ARGUMENT;
  if (tiles == 0) return QSX_OK;
  for (int64_t b = 0; b < num_blocks; ++b) {
    if (block_filters != nullptr) table.at(kRunFilter)[b] = RunTable::word_of(block_filters[b]);
    table.at(kRunOut)[b] = RunTable::word_of(block_out_bitmaps[b]);
  }
  const long long program_at = table.append(1 + static_cast<size_t>(num_instrs));
  table.words()[program_at] = num_instrs;
  for (int pc = 0; pc < num_instrs; ++pc) table.words()[program_at + 1 + pc] = program[pc];
  const long long leaves_at = table.append(static_cast<size_t>(num_blocks) * num_leaves);
  for (int64_t e = 0; e < num_blocks * num_leaves; ++e) table.words()[leaves_at + e] = RunTable::word_of(block_leaves[e]);
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  hipLaunchKernelGGL(bitmap_eval_runs_kernel, dim3(tile_grid(tiles)), dim3(kBlock), eval_lds_bytes(num_leaves), s, table.dev(), program_at, leaves_at, num_leaves,
                     reinterpret_cast<unsigned long long *>(out_counts_dev));
  QSX_CHECK_LAUNCH();
  return QSX_OK;
}

}  // extern "C"
