// like_match.hpp — the LIKE matcher shared by like.hip (CHAR(width) stripes) and varchar.hip (variable-length
// dictionaries): the pattern as the kernels take it, the match of one text that lies in LDS, and the host code that lays a
// pattern out.  Semantics and their source in the reference: like.hip's header.
//
// The matcher needs no backtracking: the pattern is cut at its '%' into segments of fixed length.  The first is anchored at
// the start of the text, the last at its end, every one in between takes its leftmost fit behind the one before.  A lane
// walks its row once: the text's length is only looked for when a last segment has to be placed (`lit%` reads no further
// than the literal, `%lit%` stops at its first fit).
#ifndef QSX_CSRC_LIKE_MATCH_HPP_
#define QSX_CSRC_LIKE_MATCH_HPP_

#include "common.hpp"

namespace qsx {
namespace like {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxSegments = QSX_MAX_LIKE_PATTERN / 2 + 2;

// The pattern as the kernels take it (by value, as select.hip's CharLiteral): the bytes of its segments one behind the
// other (no '%'), and where each segment lies.  nseg = number of '%' (runs collapsed) + 1; the first and the last segment
// may be empty, no other is.
struct LikePattern {
  unsigned char bytes[QSX_MAX_LIKE_PATTERN];
  unsigned char seg_off[kMaxSegments];
  unsigned char seg_len[kMaxSegments];
  int nseg;
};
static_assert(sizeof(LikePattern) % 4 == 0, "kernel argument");

// len bytes of the pattern (q) at t[0 .. len): every byte there is part of the text (not NUL) and is the pattern's byte or
// under a '_'.  The caller has checked that len bytes lie inside the field.
__device__ __forceinline__ bool segment_at(const unsigned char *t, const unsigned char *q, int len) {
  for (int j = 0; j < len; ++j) {
    const unsigned char c = t[j];
    if (c == 0 || (q[j] != '_' && q[j] != c)) return false;
  }
  return true;
}

// t: the row in LDS; pat: the pattern in LDS too (every lane reads the same byte of it: a broadcast.  As a by-value kernel
// argument its bytes were fetched with one global_load_ubyte per lane and comparison).
__device__ __forceinline__ bool like_match(const unsigned char *t, int width, const LikePattern &pat) {
  const int nseg = pat.nseg;
  int pos = pat.seg_len[0];   // the first segment: at the start
  if (pos > width || !segment_at(t, pat.bytes, pos)) return false;
  if (nseg == 1) return pos == width || t[pos] == 0;   // no '%': the text ends where the pattern does
  for (int s = 1; s + 1 < nseg; ++s) {                 // leftmost fit, never past the text's end
    const int len = pat.seg_len[s];
    const unsigned char *q = pat.bytes + pat.seg_off[s];
    const unsigned char q0 = q[0];                     // most positions are turned down by the segment's first byte
    bool found = false;
    for (; pos + len <= width; ++pos) {
      const unsigned char c = t[pos];
      if (c == 0) break;
      if ((q0 == '_' || q0 == c) && segment_at(t + pos + 1, q + 1, len - 1)) {
        found = true;
        break;
      }
    }
    if (!found) return false;
    pos += len;
  }
  const int len = pat.seg_len[nseg - 1];               // the last segment: at the end, not overlapping what is placed
  if (len == 0) return true;
  int end = pos;
  while (end < width && t[end] != 0) ++end;
  if (end - len < pos) return false;
  return segment_at(t + (end - len), pat.bytes + pat.seg_off[nseg - 1], len);
}

// The by-value pattern into LDS, by the whole workgroup.
__device__ __forceinline__ void stage_pattern(const LikePattern &pat, LikePattern *s_pat) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(&pat);
  uint32_t *dst = reinterpret_cast<uint32_t *>(s_pat);
  for (unsigned i = threadIdx.x; i < sizeof(LikePattern) / 4; i += kBlock) dst[i] = src[i];
  __syncthreads();
}

// The pattern as the kernels take it: cut at its first NUL, runs of '%' collapsed, segments laid out.
static LikePattern clean_pattern(const void *pattern, int pattern_length) {
  LikePattern pat{};
  const unsigned char *p = static_cast<const unsigned char *>(pattern);
  int used = 0, seg = 0;
  pat.seg_off[0] = 0;
  bool after_percent = false;
  for (int i = 0; i < pattern_length && p[i] != 0; ++i) {
    if (p[i] == '%') {
      if (after_percent) continue;
      after_percent = true;
      ++seg;
      pat.seg_off[seg] = static_cast<unsigned char>(used);
      continue;
    }
    after_percent = false;
    pat.bytes[used++] = p[i];
    pat.seg_len[seg] += 1;
  }
  pat.nseg = seg + 1;
  return pat;
}

}  // namespace like
}  // namespace qsx

#endif  // QSX_CSRC_LIKE_MATCH_HPP_
