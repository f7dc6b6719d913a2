// char_predicates.hpp — the literals of a CHAR test and of an IN list as the kernels hold them, and the host code that makes
// them.  Shared by select.hip (qsx_select_cmp_char, qsx_select_in, qsx_select_in_char) and unary_predicate.hip (the same tests
// over a unary operation's result): one form of a literal, one reading of "a NUL ends it", one padding of a list.
#ifndef QSX_CSRC_CHAR_PREDICATES_HPP_
#define QSX_CSRC_CHAR_PREDICATES_HPP_

#include "common.hpp"

namespace qsx {

struct CharLiteral {
  unsigned char bytes[QSX_MAX_CHAR_LITERAL];
  int length;   // bytes before the first NUL
};
// The literal of a comparison as the kernels take it: cut at its first NUL.  (literal_length <= QSX_MAX_CHAR_LITERAL)
inline CharLiteral char_literal(const void *literal, int literal_length) {
  CharLiteral lit{};
  lit.length = 0;
  while (lit.length < literal_length && static_cast<const unsigned char *>(literal)[lit.length] != 0) {   // a NUL ends it
    lit.bytes[lit.length] = static_cast<const unsigned char *>(literal)[lit.length];
    ++lit.length;
  }
  return lit;
}

template <typename T>
struct InListPred {
  T lits[QSX_MAX_IN_LIST];   // padded by the host to a multiple of four with copies of the first literal
  int count;                 // multiple of 4
  bool negate;
  // Equality is the type's own ==: NaN is in no list, -0.0 equals 0.0 (LiteralComparators-inl.hpp:330-370 with EqualFunctor).
  __device__ __forceinline__ bool operator()(T v) const {
    bool any = false;
#pragma unroll
    for (int g = 0; g < QSX_MAX_IN_LIST; g += 4) {   // constant indices: the literals stay in scalar registers
      if (g >= count) break;                         // wave-uniform
      any = any || v == lits[g] || v == lits[g + 1] || v == lits[g + 2] || v == lits[g + 3];
    }
    return any != negate;
  }
};
template <typename T>
inline InListPred<T> in_list_pred(const void *literals, int num_literals, int negate) {
  InListPred<T> pred{};
  std::memcpy(pred.lits, literals, sizeof(T) * static_cast<size_t>(num_literals));
  pred.count = (num_literals + 3) / 4 * 4;
  for (int i = num_literals; i < pred.count; ++i) pred.lits[i] = pred.lits[0];   // duplicates change nothing
  pred.negate = negate != 0;
  return pred;
}

// A CHAR list in device memory (staged alone, or behind the run table): read with wave-uniform indices.  Only the literals
// that can equal a field of the stripe's width are kept (no longer than it), so on fields of width <= 16 every literal lies
// in `first` / `second`.  The host pads the list to a multiple of four with copies of its first literal: the register path
// fetches four literals at a time and compares without a branch.
struct CharInList {
  long long count, negate;                                              // count: a multiple of 4 (0: no literal can match)
  long long wide;                                                       // some literal is longer than 8 bytes: `second` takes part
  long long direct;                                                     // the host sized tiles and LDS for the register path (below)
  unsigned long long first[QSX_MAX_IN_LIST], second[QSX_MAX_IN_LIST];   // bytes 0-7 / 8-15, big-endian, zero-padded
  long long length[QSX_MAX_IN_LIST];                                    // bytes before the first NUL
  unsigned char bytes[QSX_MAX_IN_LIST][QSX_MAX_CHAR_LITERAL];
};
static_assert(sizeof(CharInList) % 8 == 0, "lies in a table of 64-bit words");
struct CharInCompare {
  const CharInList *__restrict__ list;
  struct Key16 {};
  // The register path only where the host chose it for the whole launch (fields of width <= 16, EVERY stripe of the run on a
  // 4-byte boundary): its tile size and its LDS strips are the host's to provide, so host and kernel must not decide apart.
  __device__ __forceinline__ bool fits16() const { return list->direct != 0; }
  __device__ __forceinline__ Key16 key16() const { return Key16{}; }
  // strcmpHelper equality (AsciiStringComparators.hpp:218-251) of zero-padded texts: both 64-bit halves are the same.
  // (`|` and `&`, not `||` and `&&`: one literal at a time behind a branch waited for a scalar load per comparison —
  // 0.62 ms per 100 M CHAR(2) rows against 7 literals.)
  __device__ __forceinline__ bool match16(const Key16 &, unsigned long long x_first, unsigned long long x_second) const {
    bool any = false;
    const int count = static_cast<int>(list->count);
    if (list->wide != 0) {
      for (int i = 0; i < count; i += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) any |= (x_first == list->first[i + j]) & (x_second == list->second[i + j]);
      }
    } else {   // no literal reaches the second half: the text must end inside the first
      for (int i = 0; i < count; i += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) any |= x_first == list->first[i + j];
      }
      any &= x_second == 0ull;
    }
    return any != (list->negate != 0);
  }
  __device__ __forceinline__ bool match(const unsigned char *v, int width) const {
    bool any = false;
    const int count = static_cast<int>(list->count);
    for (int i = 0; i < count && !any; ++i) {
      const int len = static_cast<int>(list->length[i]);          // <= width
      bool same = len == width || v[len] == 0;                    // the text ends where the literal does
      for (int j = 0; j < len && same; ++j) same = v[j] == list->bytes[i][j];
      any = same;
    }
    return any != (list->negate != 0);
  }
};

// The list as the CHAR kernels read it, or QSX_ERR_UNSUPPORTED for a literal of more than QSX_MAX_CHAR_LITERAL bytes.
inline int char_in_list(int width, const void *literals, const int32_t *literal_lengths, int num_literals, int negate, CharInList *list) {
  std::memset(list, 0, sizeof(CharInList));
  list->negate = negate;
  for (int k = 0; k < num_literals; ++k) {
    if (literal_lengths[k] < 0) return QSX_ERR_INVALID_ARGUMENT;
    if (literal_lengths[k] > QSX_MAX_CHAR_LITERAL) return QSX_ERR_UNSUPPORTED;
  }
  for (int k = 0; k < num_literals; ++k) {
    const unsigned char *text = static_cast<const unsigned char *>(literals) + static_cast<size_t>(k) * QSX_MAX_CHAR_LITERAL;
    int len = 0;
    while (len < literal_lengths[k] && text[len] != 0) ++len;   // a NUL ends it
    if (len > width) continue;                                  // equals no field of this width
    const long long at = list->count++;
    list->length[at] = len;
    if (len > 8) list->wide = 1;
    for (int i = 0; i < len; ++i) {
      list->bytes[at][i] = text[i];
      if (i < 8) list->first[at] |= static_cast<unsigned long long>(text[i]) << (8 * (7 - i));
      else if (i < 16) list->second[at] |= static_cast<unsigned long long>(text[i]) << (8 * (15 - i));
    }
  }
  for (; list->count % 4 != 0; ++list->count) {   // a multiple of four, by copies of the first literal: duplicates change nothing
    list->first[list->count] = list->first[0];
    list->second[list->count] = list->second[0];
    list->length[list->count] = list->length[0];
    std::memcpy(list->bytes[list->count], list->bytes[0], QSX_MAX_CHAR_LITERAL);
  }
  return QSX_OK;
}
// rows per LDS tile of a CHAR(width) stripe: a multiple of 64 (whole bitmap words), at most 1024, at most 48 KiB of LDS
inline int char_tile_rows(int width) {
  int tile_rows = (48 * 1024 / width) / 64 * 64;
  if (tile_rows > 1024) tile_rows = 1024;
  if (tile_rows < 64) tile_rows = 64;
  return tile_rows;
}

}  // namespace qsx

#endif  // QSX_CSRC_CHAR_PREDICATES_HPP_
