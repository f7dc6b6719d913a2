// char_dict.hip — a device dictionary of CHAR(width) values: every distinct text gets a dense INT id, so that a CHAR(n)
// group-by component of any width can travel through the INT-key aggregation paths and be turned back into bytes at
// finalize.
//
// Stands in for the key side of PackedPayloadHashTable's upsert loop (storage/PackedPayloadHashTable.hpp:838-909: hash the
// key, walk the chain, compare, insert when absent) over a CHAR key: TypedValue::getHashAsciiString hashes the text up to
// its NUL and fastEqualCheck compares it (types/TypedValue.hpp:575-592, 693-701).  Hash values never show in results, so the
// hash here is the library's own (hash_text below, exported as qsx_char_dict_hash).
//
// One intern call is up to three launches on its stream — claim, settle, resolve — and NO lane ever waits for another:
//   claim    one lane per row.  The tile goes through LDS as in like.hip.  A lane hashes its text and probes the slot table
//            linearly from its home slot.  A slot word is 0 (empty) or {pending bit, 31-bit index + 1, 32-bit fingerprint};
//            index field 0x7FFFFFFF marks a tombstone.  Empty: atomicCAS(0 -> pending | this row's position | fingerprint), and on
//            failure go on with the word the CAS returned.  Equal fingerprint: compare the text — a PENDING slot belongs to
//            this call, its text is row `index` of this call's immutable input; a FINAL slot's text is value `index` of the
//            value store, written by an earlier launch.  Equal text: the row's result is the id (final) or a reference to the
//            owner row (pending, -3 - position; the winner of the CAS refers to itself).
//            Invariant: within claim a slot only ever goes empty -> pending, so any non-empty word a plain load shows is good
//            for the whole launch (a stale L1 line can only show "empty", and then the CAS tells).  No launch reads bytes
//            that another workgroup of the same launch wrote: the one word two workgroups share is the slot word, and only
//            through the return value of the compare-and-swap.
//   settle   the owner rows (result == -3 - own position) find their slot again, take id = atomicAdd(count), write the
//            canonical bytes to store[id], rewrite the slot as final and their result as the id.  An id that does not fit:
//            the slot becomes a tombstone and the result -2.  (Not "empty" again: another value of this call may have
//            probed past the slot while it was pending, and an empty word in front of it would cut its chain — the next
//            call would insert that value a second time.  reserve() re-hashes and drops the tombstones.)
//   resolve  a row that refers to an owner takes the owner's result (written by settle, an earlier launch); -2 and
//            references to a dropped owner become -1 and are counted in `dropped`.
// settle and resolve return at once when claim met nothing new (a flag word zeroed per call by a memset on the stream):
// the steady state of a scan — every value already present — is the claim launch alone.
//
// In front of the slot table every workgroup keeps a small LDS cache text -> result (cache entries are filled once and never
// replaced: the text is written before the 64-bit entry word that publishes it, both by the same wave, LDS operations of
// a wave complete in order).  A hit is verified against the cached text, so it is exact; it spares the slot word, the value
// store and, on a cleared dictionary, the CAS that every lane would otherwise issue on a line its L1 still shows as empty.
// A field of at most 32 bytes is read once, branch-free, into up to four 64-bit words in registers: the hash runs over the
// words and a cache hit is four word compares against LDS, not a second walk over the bytes.
#include <cstdlib>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "block_runs.hpp"

namespace qsx {
namespace char_dict {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr uint64_t kMinSlots = 16;
constexpr int64_t kMaxValues = int64_t(1) << 30;
constexpr long long kMaxPositions = 0x7FFFFFFCll;        // -3 - position must fit an int32
constexpr uint64_t kPending = uint64_t(1) << 63;
constexpr uint32_t kTombIndex = 0x7FFFFFFFu;
constexpr uint64_t kTombstone = static_cast<uint64_t>(kTombIndex) << 32;
constexpr int kCacheEntries = 256;                       // at most; fewer for wide values (cache_entries_for)
constexpr int kCacheProbes = 4;
constexpr int kCacheBytes = 8 * 1024;
constexpr uint32_t kCacheBusy = 0xFFFFFFFFu;             // result -1 is never cached

// The 64-bit hash of a text (the field up to its first NUL or `width` bytes): the text as little-endian 64-bit words, zero
// filled, one multiply-xorshift round per word, then the length.  Bytes behind the NUL never take part.
__host__ __device__ __forceinline__ uint64_t hash_round(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 32);
}
__host__ __device__ __forceinline__ uint64_t hash_finish(uint64_t h, int len) {
  h = (h ^ static_cast<uint64_t>(len)) * 0xD6E8FEB86659FD93ull;
  h ^= h >> 29;
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 32);
}
__host__ __device__ __forceinline__ uint64_t hash_text(const unsigned char *t, int width, int *out_len) {
  uint64_t h = 0x243F6A8885A308D3ull, w = 0;
  int len = 0;
  for (; len < width; ++len) {
    const unsigned char c = t[len];
    if (c == 0) break;
    w |= static_cast<uint64_t>(c) << ((len & 7) * 8);
    if ((len & 7) == 7) {
      h = hash_round(h, w);
      w = 0;
    }
  }
  if ((len & 7) != 0) h = hash_round(h, w);
  *out_len = len;
  return hash_finish(h, len);
}
// A text of at most 8 W bytes as W little-endian 64-bit words in registers, zero-filled behind its end (the canonical value):
// one branch-free pass over the field, and the same hash from the words.
template <int W>
__device__ __forceinline__ void load_words(const unsigned char *t, int width, uint64_t (&words)[W], int *out_len) {
  uint32_t part[2 * W];
#pragma unroll
  for (int i = 0; i < 2 * W; ++i) part[i] = 0;
  bool alive = true;
  int len = 0;
#pragma unroll
  for (int j = 0; j < 8 * W; ++j) {
    uint32_t c = t[j < width ? j : width - 1];   // (never past the row's own bytes)
    alive = alive && j < width && c != 0;
    c = alive ? c : 0u;
    len += alive ? 1 : 0;
    part[j >> 2] |= c << ((j & 3) * 8);
  }
#pragma unroll
  for (int i = 0; i < W; ++i) words[i] = part[2 * i] | (static_cast<uint64_t>(part[2 * i + 1]) << 32);
  *out_len = len;
}
template <int W>
__device__ __forceinline__ uint64_t hash_words(const uint64_t (&words)[W], int len) {
  uint64_t h = 0x243F6A8885A308D3ull;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const uint64_t r = hash_round(h, words[j]);
    h = len > 8 * j ? r : h;
  }
  return hash_finish(h, len);
}
__host__ __device__ __forceinline__ uint32_t fingerprint_of(uint64_t h) { return static_cast<uint32_t>(h >> 32); }
__host__ __device__ __forceinline__ uint32_t home_of(uint64_t h, uint32_t mask) { return static_cast<uint32_t>(h) & mask; }

// What the kernels walk: one stripe, or a run of blocks (block_runs.hpp; `out` of the run table = the id stripes).
struct Source {
  const long long *runs;
  const unsigned char *col;
  long long n;
  const uint64_t *filter;
  int32_t *out;
  long long tiles;
};
struct Block {
  const unsigned char *col;
  long long n;
  const uint64_t *filter;
  int32_t *out;
  long long row0;
};
__device__ __forceinline__ Block locate(const Source &src, long long tile, int tile_rows) {
  if (src.runs == nullptr) return Block{src.col, src.n, src.filter, src.out, tile * tile_rows};
  const RunTile at = run_locate(src.runs, static_cast<int>(tile));
  return Block{run_in<unsigned char>(src.runs, at.block), run_rows(src.runs, at.block), run_filter(src.runs, at.block),
               run_out<int32_t>(src.runs, at.block), static_cast<long long>(at.tile_in_block) * tile_rows};
}

struct Dict {
  int width;
  uint32_t mask;                 // slots - 1
  unsigned long long slots;
  long long capacity;
  unsigned long long *table;
  unsigned char *store;
  unsigned long long *count;     // count[0]: ids handed out (may overshoot capacity after a drop), count[1]: dropped rows
  uint32_t *flag;                // nonzero: this call's claim left rows for settle / resolve
  int lds_cache;                 // 0: claim goes to the slot table for every row (measuring only)
};

// Text a (LDS or registers' source) against text b: equal up to the first NUL or `width` bytes.
template <bool kGlobalB>
__device__ __forceinline__ bool text_equal(const unsigned char *a, const unsigned char *b, int width) {
  for (int j = 0; j < width; ++j) {
    const unsigned char ca = a[j];
    const unsigned char cb = kGlobalB ? load_global(b + j) : b[j];
    if (ca != cb) return false;
    if (ca == 0) return true;
  }
  return true;
}

__device__ __forceinline__ int cache_entries_for(int width) {
  int e = kCacheEntries;
  while (e * width > kCacheBytes) e >>= 1;   // 255 bytes: 32 entries
  return e;
}

// The slot-table walk of one row (text t in LDS, hash h): the row's result.
__device__ __forceinline__ int32_t probe_table(const Dict &d, const Source &src, int tile_rows, const unsigned char *t, uint64_t h,
                                               long long pos) {
  const uint32_t fp = fingerprint_of(h);
  const unsigned long long mine = kPending | (static_cast<unsigned long long>(pos + 1) << 32) | fp;
  uint32_t s = home_of(h, d.mask);
  for (unsigned long long probe = 0; probe < d.slots; ++probe, s = (s + 1) & d.mask) {
    unsigned long long word = load_global(&d.table[s]);
    if (word == 0) {
      const unsigned long long old = atomicCAS(&d.table[s], 0ull, mine);
      if (old == 0) return static_cast<int32_t>(-3 - pos);
      word = old;
    }
    if (static_cast<uint32_t>(word) != fp) continue;
    const uint32_t index = static_cast<uint32_t>(word >> 32) & 0x7FFFFFFFu;
    if (index == kTombIndex) continue;
    if ((word & kPending) != 0) {
      const long long owner = static_cast<long long>(index) - 1;
      const Block at = locate(src, owner / tile_rows, tile_rows);
      const unsigned char *other = at.col + (at.row0 + owner % tile_rows) * d.width;
      if (text_equal<true>(t, other, d.width)) return static_cast<int32_t>(-3 - owner);
    } else {
      const long long id = static_cast<long long>(index) - 1;
      if (text_equal<true>(t, d.store + id * d.width, d.width)) return static_cast<int32_t>(id);
    }
  }
  return -2;   // the table has no room for the text
}

// W > 0: the field fits W 64-bit words (width <= 8 W); a lane holds its text in registers, and the LDS cache holds words.
// W == 0: any width, the text is walked where it lies in LDS.
template <int W>
__global__ __launch_bounds__(kBlock) void claim_kernel(Dict d, Source src, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  // [cache words | cache texts | 16-byte aligned tile]
  const bool cache = d.lds_cache != 0;
  const int width = d.width;
  const int entries = W > 0 ? kCacheEntries : cache_entries_for(width);
  unsigned long long *s_entry = reinterpret_cast<unsigned long long *>(s_mem);
  unsigned char *s_text = s_mem + kCacheEntries * 8;
  uint64_t *s_text_words = reinterpret_cast<uint64_t *>(s_text);
  unsigned char *s_tile = s_mem + kCacheEntries * 8 + kCacheBytes;
  static_assert(kCacheEntries * 8 * 4 <= kCacheBytes, "W <= 4 words per cached text");
  for (int i = threadIdx.x; i < kCacheEntries; i += kBlock) s_entry[i] = 0;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  bool left_work = false;
  for (long long tile = blockIdx.x; tile < src.tiles; tile += gridDim.x) {
    const Block at = locate(src, tile, tile_rows);
    const int rows = static_cast<int>(at.n - at.row0 < tile_rows ? at.n - at.row0 : tile_rows);
    const unsigned char *from = at.col + at.row0 * width;
    const int bytes = rows * width;
    const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(from) & 15);
    unsigned char *data = s_tile + shift;   // data + o is 16-byte aligned where from + o is (like.hip)
    int head = shift != 0 ? 16 - shift : 0;
    if (head > bytes) head = bytes;
    const int full = (bytes - head) & ~15;
    __syncthreads();   // every wave is done with the previous tile (and the cache words are zero)
    for (int o = threadIdx.x; o < head; o += kBlock) data[o] = load_global(from + o);
    for (int o = head + threadIdx.x * 16; o < head + full; o += kBlock * 16) *reinterpret_cast<uint4 *>(data + o) = stream_load16(from + o);
    for (int o = head + full + threadIdx.x; o < bytes; o += kBlock) data[o] = load_global(from + o);
    __syncthreads();
    for (int w = wave; w * 64 < rows; w += kWavesPerBlock) {
      const int r = w * 64 + lane;
      if (r >= rows) continue;
      bool keep = true;
      if (at.filter != nullptr) keep = msb_bit(load_global(&at.filter[(at.row0 >> 6) + w]), lane);
      int32_t result = -1;
      if (keep) {
        const unsigned char *t = data + r * width;
        int len;
        uint64_t h;
        uint64_t words[W > 0 ? W : 1];
        if constexpr (W > 0) {
          load_words<W>(t, width, words, &len);
          h = hash_words<W>(words, len);
        } else {
          h = hash_text(t, width, &len);
        }
        const long long pos = tile * tile_rows + r;
        const uint32_t tag = fingerprint_of(h) | 1u;
        bool found = false;
        int free_entry = -1;
        if (cache) {
          const uint32_t first = (static_cast<uint32_t>(h) * 0x9E3779B1u) >> 8;
          for (int k = 0; k < kCacheProbes; ++k) {
            const int e = static_cast<int>((first + k) & (entries - 1));
            const unsigned long long entry = __hip_atomic_load(&s_entry[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (entry == 0) {
              free_entry = e;
              break;
            }
            if (static_cast<uint32_t>(entry >> 32) != tag || static_cast<uint32_t>(entry) == kCacheBusy) continue;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // the entry's text is read behind its word
            bool equal;
            if constexpr (W > 0) {
              equal = true;
#pragma unroll
              for (int j = 0; j < W; ++j) equal = equal && s_text_words[e * W + j] == words[j];
            } else {
              equal = text_equal<false>(t, s_text + e * width, width);
            }
            if (equal) {
              result = static_cast<int32_t>(static_cast<uint32_t>(entry));
              found = true;
              break;
            }
          }
        }
        if (!found) {
          result = probe_table(d, src, tile_rows, t, h, pos);
          if (cache && free_entry >= 0 && result != -2) {
            const unsigned long long busy = (static_cast<unsigned long long>(tag) << 32) | kCacheBusy;
            if (atomicCAS(&s_entry[free_entry], 0ull, busy) == 0) {
              if constexpr (W > 0) {
#pragma unroll
                for (int j = 0; j < W; ++j) s_text_words[free_entry * W + j] = words[j];
              } else {
                unsigned char *c = s_text + free_entry * width;
                for (int j = 0; j < width; ++j) c[j] = j < len ? t[j] : 0;
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the text is in LDS before the word that publishes it
              __hip_atomic_store(&s_entry[free_entry], (static_cast<unsigned long long>(tag) << 32) | static_cast<uint32_t>(result),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
        if (result <= -2) left_work = true;
      }
      store_global(result, &at.out[at.row0 + r]);
    }
  }
  if (left_work) store_global(1u, d.flag);
}

__global__ __launch_bounds__(kBlock) void settle_kernel(Dict d, Source src, int tile_rows) {
  if (load_global(d.flag) == 0) return;
  const int width = d.width;
  for (long long tile = blockIdx.x; tile < src.tiles; tile += gridDim.x) {
    const Block at = locate(src, tile, tile_rows);
    const int rows = static_cast<int>(at.n - at.row0 < tile_rows ? at.n - at.row0 : tile_rows);
    for (int r = threadIdx.x; r < rows; r += kBlock) {
      const long long pos = tile * tile_rows + r;
      int32_t *mine = &at.out[at.row0 + r];
      if (load_global(mine) != static_cast<int32_t>(-3 - pos)) continue;
      // the owner of a pending slot: its text again (from the input), its slot again (the one word that names this row)
      const unsigned char *t = at.col + (at.row0 + r) * width;
      unsigned char text[QSX_MAX_CHAR_DICT_WIDTH];
      for (int j = 0; j < width; ++j) text[j] = load_global(t + j);
      int len;
      const uint64_t h = hash_text(text, width, &len);
      const unsigned long long word = kPending | (static_cast<unsigned long long>(pos + 1) << 32) | fingerprint_of(h);
      uint32_t s = home_of(h, d.mask);
      bool have = false;
      for (unsigned long long probe = 0; probe < d.slots; ++probe, s = (s + 1) & d.mask) {
        if (load_global(&d.table[s]) == word) {
          have = true;
          break;
        }
      }
      if (!have) {   // cannot happen: claim wrote the word
        store_global(-2, mine);
        continue;
      }
      const unsigned long long id = atomicAdd(&d.count[0], 1ull);
      if (id < static_cast<unsigned long long>(d.capacity)) {
        unsigned char *v = d.store + id * width;
        for (int j = 0; j < width; ++j) store_global(static_cast<unsigned char>(j < len ? text[j] : 0), v + j);
        store_global(((id + 1) << 32) | fingerprint_of(h), &d.table[s]);
        store_global(static_cast<int32_t>(id), mine);
      } else {
        store_global(static_cast<unsigned long long>(kTombstone), &d.table[s]);
        store_global(-2, mine);
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void resolve_kernel(Dict d, Source src, int tile_rows) {
  if (load_global(d.flag) == 0) return;
  unsigned long long dropped = 0;
  for (long long tile = blockIdx.x; tile < src.tiles; tile += gridDim.x) {
    const Block at = locate(src, tile, tile_rows);
    const int rows = static_cast<int>(at.n - at.row0 < tile_rows ? at.n - at.row0 : tile_rows);
    for (int r = threadIdx.x; r < rows; r += kBlock) {
      int32_t *mine = &at.out[at.row0 + r];
      const int32_t v = load_global(mine);
      if (v >= -1) continue;
      int32_t id = -1;
      if (v <= -3) {   // the owner's result: settle wrote it (an id, or -2 which this launch may be turning into -1)
        const long long owner = -3 - static_cast<long long>(v);
        const Block o = locate(src, owner / tile_rows, tile_rows);
        const int32_t ov = load_global(&o.out[o.row0 + owner % tile_rows]);
        if (ov >= 0) id = ov;
      }
      if (id < 0) ++dropped;
      store_global(id, mine);
    }
  }
  dropped = wave_reduce_add(dropped);
  if (lane_id() == 0 && dropped != 0) atomicAdd(&d.count[1], dropped);
}

// reserve: the ids handed out so far (count may have overshot the old capacity), no dropped rows; then every value of the
// store into the new table.  The values are distinct: an empty slot is all a value needs.
__global__ void settle_count_kernel(unsigned long long *count, long long capacity) {
  if (count[0] > static_cast<unsigned long long>(capacity)) count[0] = static_cast<unsigned long long>(capacity);
  count[1] = 0;
}
__global__ __launch_bounds__(kBlock) void rehash_kernel(Dict d) {
  const long long size = static_cast<long long>(load_global(&d.count[0]));
  for (long long id = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; id < size; id += static_cast<long long>(gridDim.x) * kBlock) {
    unsigned char text[QSX_MAX_CHAR_DICT_WIDTH];
    for (int j = 0; j < d.width; ++j) text[j] = load_global(d.store + id * d.width + j);
    int len;
    const uint64_t h = hash_text(text, d.width, &len);
    const unsigned long long word = (static_cast<unsigned long long>(id + 1) << 32) | fingerprint_of(h);
    uint32_t s = home_of(h, d.mask);
    for (unsigned long long probe = 0; probe < d.slots; ++probe, s = (s + 1) & d.mask) {
      if (atomicCAS(&d.table[s], 0ull, word) == 0) break;
    }
  }
}

// out[i] = store[ids[i]], zero bytes for -1 and for any id outside [0, size): one thread per byte.
__global__ __launch_bounds__(kBlock) void values_kernel(Dict d, const int32_t *__restrict__ ids, long long n, unsigned char *__restrict__ out) {
  unsigned long long size = load_global(&d.count[0]);
  if (size > static_cast<unsigned long long>(d.capacity)) size = static_cast<unsigned long long>(d.capacity);
  const long long total = n * d.width;
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * kBlock) {
    const long long row = i / d.width;
    const int j = static_cast<int>(i - row * d.width);
    const int32_t id = ids[row];
    unsigned char c = 0;
    if (id >= 0 && static_cast<unsigned long long>(id) < size) c = load_global(d.store + static_cast<long long>(id) * d.width + j);
    out[i] = c;
  }
}

static int tile_rows_for(int width) {   // as like.hip: whole bitmap words, at most 48 KiB of LDS
  int tile_rows = (48 * 1024 / width) / 64 * 64;
  if (tile_rows > 1024) tile_rows = 1024;
  if (tile_rows < 64) tile_rows = 64;
  return tile_rows;
}
static size_t claim_lds_bytes(int tile_rows, int width) {
  return kCacheEntries * 8 + kCacheBytes + (static_cast<size_t>(tile_rows) * width + 15) / 16 * 16 + 16;
}
static uint64_t slots_for(int64_t max_values) {
  const uint64_t s = next_pow2(2 * static_cast<uint64_t>(max_values));
  return s < kMinSlots ? kMinSlots : s;
}

}  // namespace char_dict
}  // namespace qsx

using namespace qsx;
using namespace qsx::char_dict;

// control block: [flag, 12 bytes of padding | count, dropped] — the first 16 bytes are what every intern call zeroes
struct qsx_char_dict {
  int width = 0;
  int64_t capacity = 0;
  uint64_t slots = 0;
  unsigned char *store = nullptr;
  unsigned long long *table = nullptr;
  unsigned char *control = nullptr;
  bool lds_cache = true;
  // The calls on a dictionary are serialised: the mutex covers the enqueue, the event lets a call on another stream start
  // behind the previous one (as the join table's building streams).  No call waits for the device.
  std::mutex mutex;
  hipEvent_t event = nullptr;
  hipStream_t last_stream = nullptr;
  bool recorded = false;
};

namespace {

Dict device_view(const qsx_char_dict *d) {
  return Dict{d->width, static_cast<uint32_t>(d->slots - 1), d->slots, d->capacity, d->table, d->store,
              reinterpret_cast<unsigned long long *>(d->control + 16), reinterpret_cast<uint32_t *>(d->control), d->lds_cache ? 1 : 0};
}

int order_behind_previous(qsx_char_dict *d, hipStream_t s) {
  if (d->recorded && d->last_stream != s) QSX_HIP_TRY(hipStreamWaitEvent(s, d->event, 0));
  return QSX_OK;
}
int mark_issued(qsx_char_dict *d, hipStream_t s) {
  QSX_HIP_TRY(hipEventRecord(d->event, s));
  d->last_stream = s;
  d->recorded = true;
  return QSX_OK;
}

int allocate(int width, int64_t max_values, unsigned char **store, unsigned long long **table, uint64_t *slots) {
  *slots = slots_for(max_values);
  QSX_HIP_TRY(device_malloc(store, static_cast<size_t>(max_values) * width));
  if (device_malloc(table, *slots * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    (void)device_free(*store);
    *store = nullptr;
    return QSX_ERR_OUT_OF_MEMORY;
  }
  return QSX_OK;
}

// claim, settle, resolve over `src` (the caller holds the mutex)
int launch_intern(qsx_char_dict *d, const Source &src, hipStream_t s) {
  int rc = order_behind_previous(d, s);
  if (rc != QSX_OK) return rc;
  const Dict view = device_view(d);
  const int tile_rows = tile_rows_for(d->width);
  QSX_HIP_TRY(hipMemsetAsync(d->control, 0, 16, s));
  const int grid = tile_grid(src.tiles);
  const size_t lds = claim_lds_bytes(tile_rows, d->width);
  switch (d->width <= 32 ? (d->width + 7) / 8 : 0) {
    case 1: hipLaunchKernelGGL(claim_kernel<1>, dim3(grid), dim3(kBlock), lds, s, view, src, tile_rows); break;
    case 2: hipLaunchKernelGGL(claim_kernel<2>, dim3(grid), dim3(kBlock), lds, s, view, src, tile_rows); break;
    case 3: hipLaunchKernelGGL(claim_kernel<3>, dim3(grid), dim3(kBlock), lds, s, view, src, tile_rows); break;
    case 4: hipLaunchKernelGGL(claim_kernel<4>, dim3(grid), dim3(kBlock), lds, s, view, src, tile_rows); break;
    default: hipLaunchKernelGGL(claim_kernel<0>, dim3(grid), dim3(kBlock), lds, s, view, src, tile_rows); break;
  }
  QSX_CHECK_LAUNCH();
  hipLaunchKernelGGL(settle_kernel, dim3(grid), dim3(kBlock), 0, s, view, src, tile_rows);
  QSX_CHECK_LAUNCH();
  hipLaunchKernelGGL(resolve_kernel, dim3(grid), dim3(kBlock), 0, s, view, src, tile_rows);
  QSX_CHECK_LAUNCH();
  return mark_issued(d, s);
}

}  // namespace

extern "C" {

uint64_t qsx_char_dict_hash(const void *text, int width) {
  if (text == nullptr || width < 1 || width > QSX_MAX_CHAR_DICT_WIDTH) return 0;
  int len;
  return hash_text(static_cast<const unsigned char *>(text), width, &len);
}

int qsx_char_dict_create(int width, int64_t max_values, qsx_char_dict_t **out) {
  QSX_REQUIRE_DEVICE();
  if (out == nullptr || width < 1 || width > QSX_MAX_CHAR_DICT_WIDTH || max_values < 1 || max_values > kMaxValues) return QSX_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  qsx_char_dict *d = new qsx_char_dict;
  d->width = width;
  d->capacity = max_values;
  const char *knob = std::getenv("QSX_CHAR_DICT_LDS_CACHE");   // "0": measure without the LDS cache (tools/char_dict_probe.py)
  d->lds_cache = !(knob != nullptr && knob[0] == '0');
  int rc = allocate(width, max_values, &d->store, &d->table, &d->slots);
  if (rc == QSX_OK && device_malloc(&d->control, 32) != hipSuccess) {
    (void)hipGetLastError();
    rc = QSX_ERR_OUT_OF_MEMORY;
  }
  if (rc == QSX_OK && hipEventCreateWithFlags(&d->event, hipEventDisableTiming) != hipSuccess) rc = QSX_ERR_HIP;
  // the table and the counters start empty; the null stream orders this in front of nothing, so wait for it here, once
  if (rc == QSX_OK && (hipMemset(d->table, 0, d->slots * sizeof(unsigned long long)) != hipSuccess || hipMemset(d->control, 0, 32) != hipSuccess ||
                       hipDeviceSynchronize() != hipSuccess)) {
    rc = QSX_ERR_HIP;
  }
  if (rc != QSX_OK) {
    if (d->event != nullptr) (void)hipEventDestroy(d->event);
    if (d->store != nullptr) (void)device_free(d->store);
    if (d->table != nullptr) (void)device_free(d->table);
    if (d->control != nullptr) (void)device_free(d->control);
    delete d;
    return rc;
  }
  *out = d;
  return QSX_OK;
}

int qsx_char_dict_destroy(qsx_char_dict_t *d) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr) return QSX_ERR_INVALID_ARGUMENT;
  (void)synchronize_owner_device(d->control);
  (void)device_free_idle(d->store);
  (void)device_free_idle(d->table);
  (void)device_free_idle(d->control);
  (void)hipEventDestroy(d->event);
  delete d;
  return QSX_OK;
}

int qsx_char_dict_clear(qsx_char_dict_t *d, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  std::lock_guard<std::mutex> lock(d->mutex);
  const int rc = order_behind_previous(d, s);
  if (rc != QSX_OK) return rc;
  QSX_HIP_TRY(hipMemsetAsync(d->table, 0, d->slots * sizeof(unsigned long long), s));
  QSX_HIP_TRY(hipMemsetAsync(d->control, 0, 32, s));
  return mark_issued(d, s);
}

int qsx_char_dict_reserve(qsx_char_dict_t *d, int64_t max_values, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr || max_values < 1 || max_values > kMaxValues) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  std::lock_guard<std::mutex> lock(d->mutex);
  int rc = order_behind_previous(d, s);
  if (rc != QSX_OK) return rc;
  unsigned long long *count = reinterpret_cast<unsigned long long *>(d->control + 16);
  hipLaunchKernelGGL(settle_count_kernel, dim3(1), dim3(1), 0, s, count, static_cast<long long>(d->capacity));
  QSX_CHECK_LAUNCH();
  if (max_values <= d->capacity) return mark_issued(d, s);   // never smaller: every id stays
  unsigned char *store = nullptr;
  unsigned long long *table = nullptr;
  uint64_t slots = 0;
  rc = allocate(d->width, max_values, &store, &table, &slots);
  if (rc != QSX_OK) return rc;
  unsigned char *old_store = d->store;
  unsigned long long *old_table = d->table;
  if (hipMemcpyAsync(store, old_store, static_cast<size_t>(d->capacity) * d->width, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemsetAsync(table, 0, slots * sizeof(unsigned long long), s) != hipSuccess) {
    set_last_error("qsx_char_dict_reserve", hipGetLastError());
    (void)device_free(store);
    (void)device_free(table);
    return QSX_ERR_HIP;
  }
  const int64_t old_capacity = d->capacity;
  d->store = store;
  d->table = table;
  d->slots = slots;
  d->capacity = max_values;
  hipLaunchKernelGGL(rehash_kernel, dim3(grid_for(old_capacity, kBlock)), dim3(kBlock), 0, s, device_view(d));
  QSX_CHECK_LAUNCH();
  rc = mark_issued(d, s);
  // the old store and table go back once the work queued on them has finished (reserve follows a qsx_char_dict_size that
  // has just waited for the stream: the copy and the re-hash are all there is to wait for)
  QSX_HIP_TRY(hipStreamSynchronize(s));
  (void)device_free_idle(old_store);
  (void)device_free_idle(old_table);
  return rc;
}

int qsx_char_dict_intern(qsx_char_dict_t *d, const void *col_dev, int64_t n, const uint64_t *filter_dev, int32_t *out_ids_dev,
                         qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr || n < 0 || (n > 0 && (col_dev == nullptr || out_ids_dev == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  if (n == 0) return QSX_OK;
  const int tile_rows = tile_rows_for(d->width);
  const long long tiles = (n + tile_rows - 1) / tile_rows;
  if (tiles * tile_rows > kMaxPositions) return QSX_ERR_UNSUPPORTED;
  const Source src{nullptr, static_cast<const unsigned char *>(col_dev), n, filter_dev, out_ids_dev, tiles};
  std::lock_guard<std::mutex> lock(d->mutex);
  return launch_intern(d, src, as_stream(stream));
}

int qsx_char_dict_intern_blocks(qsx_char_dict_t *d, int64_t num_blocks, const int64_t *block_rows, const void *const *block_cols,
                                const uint64_t *const *block_filters, int32_t *const *block_out_ids, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr || num_blocks < 0 || (num_blocks > 0 && (block_rows == nullptr || block_cols == nullptr || block_out_ids == nullptr))) {
    return QSX_ERR_INVALID_ARGUMENT;
  }
  if (!run_blocks_ok(num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_out_ids))) return QSX_ERR_INVALID_ARGUMENT;
  if (num_blocks == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  const int tile_rows = tile_rows_for(d->width);
  RunTable table;
  const long long tiles = table.build(tile_rows, num_blocks, block_rows, block_cols, reinterpret_cast<const void *const *>(block_filters),
                                      reinterpret_cast<void *const *>(block_out_ids), nullptr);
  if (tiles < 0 || tiles * tile_rows > kMaxPositions) return QSX_ERR_UNSUPPORTED;
  if (tiles == 0) return QSX_OK;
  const int rc = table.upload(s);
  if (rc != QSX_OK) return rc;
  const Source src{table.dev(), nullptr, 0, nullptr, nullptr, tiles};
  std::lock_guard<std::mutex> lock(d->mutex);
  return launch_intern(d, src, s);
}

int qsx_char_dict_size(qsx_char_dict_t *d, int64_t *out_values, int64_t *out_dropped, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr || (out_values == nullptr && out_dropped == nullptr)) return QSX_ERR_INVALID_ARGUMENT;
  hipStream_t s = as_stream(stream);
  unsigned long long counts[2] = {0, 0};
  int64_t capacity;
  {
    std::lock_guard<std::mutex> lock(d->mutex);
    const int rc = order_behind_previous(d, s);   // a call on another stream counts too
    if (rc != QSX_OK) return rc;
    QSX_HIP_TRY(hipMemcpyAsync(counts, d->control + 16, sizeof(counts), hipMemcpyDeviceToHost, s));
    capacity = d->capacity;
  }
  QSX_HIP_TRY(hipStreamSynchronize(s));
  if (out_values != nullptr) *out_values = counts[0] > static_cast<unsigned long long>(capacity) ? capacity : static_cast<int64_t>(counts[0]);
  if (out_dropped != nullptr) *out_dropped = static_cast<int64_t>(counts[1]);
  return QSX_OK;
}

int qsx_char_dict_values(qsx_char_dict_t *d, const int32_t *ids_dev, int64_t n, void *out_dev, qsx_stream_t stream) {
  QSX_REQUIRE_DEVICE();
  if (d == nullptr || n < 0 || (n > 0 && (ids_dev == nullptr || out_dev == nullptr))) return QSX_ERR_INVALID_ARGUMENT;
  if (n == 0) return QSX_OK;
  hipStream_t s = as_stream(stream);
  std::lock_guard<std::mutex> lock(d->mutex);
  const int rc = order_behind_previous(d, s);
  if (rc != QSX_OK) return rc;
  hipLaunchKernelGGL(values_kernel, dim3(grid_for(n * d->width, kBlock)), dim3(kBlock), 0, s, device_view(d), ids_dev, static_cast<long long>(n),
                     static_cast<unsigned char *>(out_dev));
  QSX_CHECK_LAUNCH();
  return mark_issued(d, s);
}

}  // extern "C"
