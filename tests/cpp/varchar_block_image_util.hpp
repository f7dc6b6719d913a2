// varchar_block_image_util.hpp — test helper: WRITES a CompressedColumnStore block image that holds VARCHAR attributes the way
// CompressedBlockBuilder leaves them (storage/CompressedBlockBuilder.cpp:262-420, 452-455: a variable-length attribute always
// sits behind a dictionary): every VARCHAR attribute as a stripe of 1/2/4-byte codes into a variable-length dictionary
// (compression/CompressionDictionaryBuilder.cpp:53-66, CompressionDictionaryLite.hpp:248-290)
//     uint32 num_codes | uint32 null_code | uint32 offset[num_codes] | the values, each with its terminating NUL
// every other attribute as a stripe of its values.  The dictionary is computed here from the strings — a std::set under the
// byte order of the reference's comparator — independently of the code under test.  Shares the header and the protobuf writers
// with block_image_util.hpp.
#ifndef QSX_TESTS_CPP_VARCHAR_BLOCK_IMAGE_UTIL_HPP_
#define QSX_TESTS_CPP_VARCHAR_BLOCK_IMAGE_UTIL_HPP_

#include <set>
#include <string>

#include "block_image_util.hpp"

namespace block_image {

struct VarCharColumn {
  std::vector<std::string> values;   // num_tuples texts, no NUL inside
  std::vector<bool> nulls;           // empty = no NULLs
  int code_width = 1;
};
enum class Damage { kNone, kDescendingOffset, kNoFinalNul };

struct VarCharImageInfo {
  std::vector<std::size_t> dictionary_offset;   // per attribute: where the 8-byte dictionary header lies in the image (0: none)
  std::vector<std::size_t> dictionary_bytes;
  std::int64_t max_tuples = 0;
};

// strcmp order on unsigned bytes (AsciiStringComparators.hpp): std::string's own order
inline std::vector<std::string> SortedDictionary(const VarCharColumn &column, std::size_t n) {
  std::set<std::string> distinct;
  for (std::size_t i = 0; i < n; ++i) {
    if (column.nulls.empty() || !column.nulls[i]) distinct.insert(column.values[i]);
  }
  return std::vector<std::string>(distinct.begin(), distinct.end());
}

// fixed[a]: num_tuples values of a fixed-width attribute, or nullptr where varchar[a] describes a VARCHAR attribute.
// info_padding: bytes of an unknown length-delimited field appended to the CompressedBlockInfo — the dictionaries follow the
// protobuf, so this moves them (and their offset arrays) to any byte alignment.
inline std::vector<unsigned char> BuildCompressedWithVarChar(const quickstep::CatalogRelation &relation, const std::vector<const void *> &fixed,
                                                            const std::vector<const VarCharColumn *> &varchar, std::int64_t num_tuples,
                                                            std::size_t block_bytes, std::size_t info_padding, VarCharImageInfo *where = nullptr,
                                                            Damage damage = Damage::kNone) {
  const std::size_t n = static_cast<std::size_t>(num_tuples), attrs = relation.size();
  std::vector<int> compressed_ids;
  for (std::size_t a = 0; a < attrs; ++a) if (varchar[a] != nullptr) compressed_ids.push_back(static_cast<int>(a));
  const std::size_t header_bytes = HeaderCompressed(block_bytes >> 21, 0, 0, compressed_ids).size();
  const std::size_t tuple_store_size = block_bytes - 4 - header_bytes;
  const std::vector<unsigned char> header = HeaderCompressed(block_bytes >> 21, tuple_store_size, 0, compressed_ids);
  std::vector<std::vector<std::string>> dict(attrs);
  std::vector<unsigned char> dictionaries;
  std::vector<std::uint64_t> attribute_size(attrs), dictionary_size(attrs, 0);
  std::vector<std::size_t> dictionary_at(attrs, 0);
  for (std::size_t a = 0; a < attrs; ++a) {
    if (varchar[a] == nullptr) {
      attribute_size[a] = static_cast<std::uint64_t>(relation.getAttributeType(static_cast<quickstep::attribute_id>(a)).width);
      continue;
    }
    attribute_size[a] = static_cast<std::uint64_t>(varchar[a]->code_width);
    dict[a] = SortedDictionary(*varchar[a], n);
    bool any_null = false;
    for (std::size_t i = 0; i < n && !varchar[a]->nulls.empty(); ++i) any_null = any_null || varchar[a]->nulls[i];
    const std::uint32_t head[2] = {static_cast<std::uint32_t>(dict[a].size()), any_null ? static_cast<std::uint32_t>(dict[a].size()) : 0xFFFFFFFFu};
    std::vector<std::uint32_t> offsets;
    std::string bytes;
    for (const std::string &v : dict[a]) {
      offsets.push_back(static_cast<std::uint32_t>(bytes.size()));
      bytes += v;
      bytes.push_back('\0');
    }
    if (damage == Damage::kDescendingOffset && offsets.size() > 2) std::swap(offsets[1], offsets[2]);
    if (damage == Damage::kNoFinalNul && !bytes.empty()) bytes.back() = 'x';
    dictionary_at[a] = dictionaries.size();
    const unsigned char *h = reinterpret_cast<const unsigned char *>(head), *o = reinterpret_cast<const unsigned char *>(offsets.data());
    dictionaries.insert(dictionaries.end(), h, h + 8);
    dictionaries.insert(dictionaries.end(), o, o + offsets.size() * 4);
    dictionaries.insert(dictionaries.end(), bytes.begin(), bytes.end());
    dictionary_size[a] = dictionaries.size() - dictionary_at[a];
  }
  // CompressedBlockInfo (StorageBlockLayout.proto:128-150); no uncompressed attribute has NULLs here: no null bitmaps
  std::vector<unsigned char> info, packed;
  for (std::uint64_t v : attribute_size) PutFixed64(&packed, v);
  PutVarint(&info, (1 << 3) | 2);
  PutBytes(&info, packed);
  packed.clear();
  for (std::uint64_t v : dictionary_size) PutFixed64(&packed, v);
  PutVarint(&info, (2 << 3) | 2);
  PutBytes(&info, packed);
  PutVarint(&info, (3 << 3) | 1);
  PutFixed64(&info, 0);
  packed.assign(attrs, 0);
  PutVarint(&info, (4 << 3) | 2);
  PutBytes(&info, packed);
  if (info_padding > 0) {   // a field this layer does not know (number 15): skipped by a protobuf reader
    PutVarint(&info, (15 << 3) | 2);
    PutBytes(&info, std::vector<unsigned char>(info_padding - 1, 0x5A));
  }

  std::vector<unsigned char> image(block_bytes, 0xCD);
  const std::int32_t header_length = static_cast<std::int32_t>(header.size());
  std::memcpy(image.data(), &header_length, 4);
  std::memcpy(image.data() + 4, header.data(), header.size());
  unsigned char *at = image.data() + 4 + header.size();
  const std::int32_t sub_header[2] = {static_cast<std::int32_t>(num_tuples), static_cast<std::int32_t>(info.size())};
  std::memcpy(at, sub_header, 8);
  at += 8;
  std::memcpy(at, info.data(), info.size());
  at += info.size();
  if (where != nullptr) {
    where->dictionary_offset.assign(attrs, 0);
    where->dictionary_bytes.assign(attrs, 0);
    for (std::size_t a = 0; a < attrs; ++a) {
      if (varchar[a] == nullptr) continue;
      where->dictionary_offset[a] = static_cast<std::size_t>(at - image.data()) + dictionary_at[a];
      where->dictionary_bytes[a] = static_cast<std::size_t>(dictionary_size[a]);
    }
  }
  std::memcpy(at, dictionaries.data(), dictionaries.size());
  at += dictionaries.size();
  std::size_t tuple_length = 0;
  for (std::uint64_t v : attribute_size) tuple_length += static_cast<std::size_t>(v);
  const std::size_t max_tuples = static_cast<std::size_t>(image.data() + block_bytes - at) / tuple_length;
  if (where != nullptr) where->max_tuples = static_cast<std::int64_t>(max_tuples);
  for (std::size_t a = 0; a < attrs; ++a) {
    const std::size_t size = static_cast<std::size_t>(attribute_size[a]);
    for (std::size_t i = 0; i < n && i < max_tuples; ++i) {
      if (varchar[a] == nullptr) {
        std::memcpy(at + i * size, static_cast<const char *>(fixed[a]) + i * size, size);
        continue;
      }
      const bool is_null = !varchar[a]->nulls.empty() && varchar[a]->nulls[i];
      const std::uint64_t code = is_null ? dict[a].size()
                                         : static_cast<std::uint64_t>(std::lower_bound(dict[a].begin(), dict[a].end(), varchar[a]->values[i]) - dict[a].begin());
      std::memcpy(at + i * size, &code, size);   // (little-endian: the low `size` bytes)
    }
    at += max_tuples * size;
  }
  return image;
}

}  // namespace block_image

#endif  // QSX_TESTS_CPP_VARCHAR_BLOCK_IMAGE_UTIL_HPP_
