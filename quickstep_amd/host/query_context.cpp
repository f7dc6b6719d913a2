// query_context.cpp — predicates, insert destinations, the aggregation state, QueryContext, LIP filters, the work-order container (see quickstep_gpu.hpp; what the files share: quickstep_gpu_internal.hpp)
#include "quickstep_gpu_internal.hpp"

namespace quickstep {

// ---------------------------------------------------------------------------
// Predicate
// ---------------------------------------------------------------------------
void CheckLikeTerm(const ComparisonPredicate &term, const Type &type) {
  if (!IsTextType(type.id)) throw ExecutionError("LIKE / NOT LIKE on an attribute that is neither CHAR(n) nor VARCHAR(n)", QSX_ERR_UNSUPPORTED);
  if (term.rhs_attribute != kInvalidAttributeID) throw ExecutionError("LIKE / NOT LIKE between two attributes", QSX_ERR_UNSUPPORTED);
  if (term.literal.text.size() > QSX_MAX_LIKE_PATTERN) throw ExecutionError("LIKE pattern longer than QSX_MAX_LIKE_PATTERN bytes", QSX_ERR_UNSUPPORTED);
}

void SelectCharTerm(const ComparisonPredicate &term, const void *stripe, int width, std::int64_t n, const std::uint64_t *filter,
                    std::uint64_t *out_bitmap, std::int64_t *out_count) {
  if (IsLikeComparison(term.comparison)) {
    // PatternMatchingUncheckedComparator (PatternMatchingComparators-inl.hpp:190-268)
    CheckStatus(qsx_select_like(stripe, width, n, term.literal.text.data(), static_cast<int>(term.literal.text.size()),
                                term.comparison == ComparisonID::kNotLike ? 1 : 0, filter, out_bitmap, out_count, CurrentStream()),
                "qsx_select_like");
    return;
  }
  // CHAR(n) OP string literal (AsciiStringUncheckedComparator, AsciiStringComparators.hpp:218-251)
  CheckStatus(qsx_select_cmp_char(stripe, width, n, static_cast<int>(term.comparison), term.literal.text.data(),
                                  static_cast<int>(term.literal.text.size()), filter, out_bitmap, out_count, CurrentStream()),
              "qsx_select_cmp_char");
}

// ---------------------------------------------------------------------------
// Predicate trees: builders, the leaves of a tree and its postfix program
// ---------------------------------------------------------------------------
PredicateNodePtr Predicate::Compare(const ComparisonPredicate &term) {
  auto n = std::make_shared<PredicateNode>();
  n->kind = PredicateNode::kComparison;
  n->comparison = term;
  return n;
}
PredicateNodePtr Predicate::In(attribute_id operand, std::vector<TypedLiteral> literals) {
  auto n = std::make_shared<PredicateNode>();
  n->kind = PredicateNode::kInList;
  n->comparison.attribute = operand;
  n->comparison.comparison = ComparisonID::kEqual;
  n->in_literals = std::move(literals);
  return n;
}
static PredicateNodePtr NodeOver(PredicateNode::Kind kind, std::vector<PredicateNodePtr> children) {
  auto n = std::make_shared<PredicateNode>();
  n->kind = kind;
  n->children = std::move(children);
  return n;
}
PredicateNodePtr Predicate::And(std::vector<PredicateNodePtr> children) { return NodeOver(PredicateNode::kConjunction, std::move(children)); }
PredicateNodePtr Predicate::Or(std::vector<PredicateNodePtr> children) { return NodeOver(PredicateNode::kDisjunction, std::move(children)); }
PredicateNodePtr Predicate::Not(PredicateNodePtr child) { return NodeOver(PredicateNode::kNegation, {std::move(child)}); }

PredicateNodePtr Predicate::In(ScalarPtr operand, std::vector<TypedLiteral> literals) {
  auto n = std::make_shared<PredicateNode>();
  n->kind = PredicateNode::kInList;
  n->comparison = ComparisonPredicate::OnScalar(std::move(operand), ComparisonID::kEqual, TypedLiteral::Long(0));   // (the literals: in_literals)
  n->in_literals = std::move(literals);
  return n;
}

// ---------------------------------------------------------------------------
// Terms over a unary operation (ComparisonPredicate::operand)
// ---------------------------------------------------------------------------
ComparisonPredicate ComparisonPredicate::OnScalar(ScalarPtr scalar, ComparisonID c, TypedLiteral l) {
  // `attribute`: the operation's attribute, whose null bitmap is the term's (kInvalidAttributeID for a scalar CheckUnaryTerm refuses)
  const bool unary_of_attribute = scalar != nullptr && scalar->kind == Scalar::kUnaryExpression && scalar->operand != nullptr &&
                                  scalar->operand->kind == Scalar::kAttribute;
  ComparisonPredicate p(unary_of_attribute ? scalar->operand->attribute : kInvalidAttributeID, c, std::move(l));
  p.operand = std::move(scalar);
  return p;
}

// The operand of such a term: a unary operation of an attribute (no VARCHAR), no LIKE, no second attribute.  Returns the
// operand's type — INT, or CHAR(m) — which the literal(s) must have (CheckUnaryLiteral).
Type CheckUnaryTerm(const ComparisonPredicate &term, const CatalogRelation &relation) {
  const ScalarPtr &s = term.operand;
  if (term.rhs_attribute != kInvalidAttributeID) {
    throw ExecutionError("a predicate term with a scalar operand and rhs_attribute: the right side of a unary operation is a literal", QSX_ERR_INVALID_ARGUMENT);
  }
  if (s == nullptr || s->kind != Scalar::kUnaryExpression || s->operand == nullptr || s->operand->kind != Scalar::kAttribute) {
    throw ExecutionError("a predicate term's scalar operand that is not EXTRACT / SUBSTRING of an attribute", QSX_ERR_UNSUPPORTED);
  }
  if (IsLikeComparison(term.comparison)) throw ExecutionError("LIKE / NOT LIKE over a unary operation (EXTRACT / SUBSTRING)", QSX_ERR_UNSUPPORTED);
  if (relation.getAttributeType(s->operand->attribute).id == kVarChar) {
    throw ExecutionError("a predicate term over a unary operation of a VARCHAR attribute", QSX_ERR_UNSUPPORTED);
  }
  return UnaryResultType(s, relation);   // (the operation's own rules: a DATE / a CHAR(n) attribute, the unit, the window)
}
void CheckUnaryLiteral(const Type &operand_type, const TypedLiteral &literal) {
  if (literal.type != operand_type.id) {
    throw ExecutionError("a predicate term over a unary operation: EXTRACT wants an INT literal, SUBSTRING a CHAR literal", QSX_ERR_UNSUPPORTED);
  }
  if (operand_type.id == kChar && literal.text.size() > QSX_MAX_CHAR_LITERAL) {
    throw ExecutionError("a CHAR literal longer than QSX_MAX_CHAR_LITERAL bytes", QSX_ERR_UNSUPPORTED);
  }
}
static bool SameOperand(const ScalarPtr &a, const ScalarPtr &b) {
  if (a == nullptr || b == nullptr) return a == b;
  if (a == b) return true;
  if (a->kind != Scalar::kUnaryExpression || b->kind != Scalar::kUnaryExpression || a->unary_operation != b->unary_operation) return false;
  if (a->operand == nullptr || b->operand == nullptr || a->operand->kind != Scalar::kAttribute || b->operand->kind != Scalar::kAttribute ||
      a->operand->attribute != b->operand->attribute) {
    return false;
  }
  return a->unary_operation == UnaryOperationID::kDateExtract ? a->date_extract_unit == b->date_extract_unit
                                                              : a->substring_start == b->substring_start && a->substring_length == b->substring_length;
}
static qsx_unary_operand_t UnaryOperandOf(const Scalar &s) {
  qsx_unary_operand_t operand = {};
  if (s.unary_operation == UnaryOperationID::kDateExtract) {
    operand.kind = QSX_UNARY_DATE_FIELD;
    operand.unit = s.date_extract_unit;
  } else {
    operand.kind = QSX_UNARY_SUBSTRING;
    operand.start = s.substring_start;
    operand.length = s.substring_length;
  }
  return operand;
}
// The stripe width the entry points take for an attribute of type t: 8 for a date, n for CHAR(n).
static int UnaryStripeWidth(const Type &t) { return t.id == kDate ? 8 : t.width; }
// May the term be evaluated over block's dictionary of attribute a (its result: the code set)?  A fixed-width dictionary; a
// dictionary of dates inside an adopted image may lie anywhere, and the date kernels want 8-byte alignment.
static bool UnaryOnDictionary(const StorageBlock &block, attribute_id a, const Type &t) {
  const CompressedAttribute *c = block.compressedAttribute(a);
  return c != nullptr && c->kind == CompressedAttribute::kDictionary && !c->variable_length && c->num_codes > 0 &&
         (t.id != kDate || (reinterpret_cast<std::uintptr_t>(c->dictionary) & 7) == 0);
}

// attribute OP attribute outside a join residual: both attributes are the input relation's, numeric with numeric or DATE with DATE
void CheckAttributeComparison(const ComparisonPredicate &term, const CatalogRelation &relation) {
  if (term.on_build_side || term.rhs_on_build_side) {
    throw ExecutionError("a comparison of two attributes names the build side outside a join residual", QSX_ERR_INVALID_ARGUMENT);
  }
  const Type &lhs = relation.getAttributeType(term.attribute), &rhs = relation.getAttributeType(term.rhs_attribute);
  if (IsLikeComparison(term.comparison)) CheckLikeTerm(term, lhs);   // (LIKE / NOT LIKE between two attributes: refused there)
  if (lhs.id == kVarChar || rhs.id == kVarChar) throw ExecutionError("a comparison of two attributes, one of them VARCHAR(n)", QSX_ERR_UNSUPPORTED);
  if (lhs.id == kChar || rhs.id == kChar) throw ExecutionError("a comparison of two attributes, one of them CHAR(n)", QSX_ERR_UNSUPPORTED);
  if ((lhs.id == kDate) != (rhs.id == kDate)) throw ExecutionError("a comparison of a DATE attribute with an attribute that is no DATE", QSX_ERR_UNSUPPORTED);
}

namespace {
std::atomic<std::int64_t> tree_block_evaluations{0}, tree_run_evaluations{0};
std::atomic<std::int64_t> attribute_comparison_block_evaluations{0}, attribute_comparison_run_evaluations{0};
std::atomic<std::int64_t> unary_block_evaluations{0}, unary_run_evaluations{0};

// One side of `attribute OP attribute` over nb blocks as the blocks hold it (qsx_operand_coding_t): values, or the codes of a
// compressed attribute with the block's code width, dictionary and number of codes — nothing is decoded.
struct OperandOfBlocks {
  std::vector<const void *> stripes, dictionaries;
  std::vector<std::int32_t> code_widths;
  std::vector<std::int64_t> num_codes;
  qsx_operand_coding_t coding;
  OperandOfBlocks(const StorageBlock *const *blocks, std::size_t nb, attribute_id a)
      : stripes(nb, nullptr), dictionaries(nb, nullptr), code_widths(nb, 0), num_codes(nb, 0) {
    for (std::size_t b = 0; b < nb; ++b) {
      if (blocks[b]->numTuples() == 0) continue;
      const CompressedAttribute *c = blocks[b]->compressedAttribute(a);
      if (c == nullptr) {
        stripes[b] = blocks[b]->stripe(a);
        continue;
      }
      stripes[b] = c->codes;
      code_widths[b] = c->code_width;
      if (c->kind == CompressedAttribute::kDictionary) {
        dictionaries[b] = c->dictionary;
        num_codes[b] = c->num_codes;
      }
    }
    coding.block_code_width = code_widths.data();
    coding.block_dictionaries = dictionaries.data();
    coding.block_num_codes = num_codes.data();
  }
};

// term.attribute OP term.rhs_attribute over nb blocks in one launch (qsx_select_cmp_columns_blocks); a single block is a run of
// one.  No sort-column case: a search does not apply to two attributes.  NULLs are the caller's.
void SelectAttributeComparison(const StorageBlock *const *blocks, std::size_t nb, const std::int64_t *rows, const ComparisonPredicate &term,
                               const std::uint64_t *const *in_filters, std::uint64_t *const *outs, std::int64_t *counts) {
  if (nb == 0) return;
  const CatalogRelation &relation = blocks[0]->getRelation();
  CheckAttributeComparison(term, relation);
  const OperandOfBlocks lhs(blocks, nb, term.attribute), rhs(blocks, nb, term.rhs_attribute);
  CheckStatus(qsx_select_cmp_columns_blocks(relation.getAttributeType(term.attribute).id, relation.getAttributeType(term.rhs_attribute).id,
                                            static_cast<std::int64_t>(nb), rows, lhs.stripes.data(), &lhs.coding, rhs.stripes.data(), &rhs.coding,
                                            static_cast<int>(term.comparison), in_filters, outs, counts, CurrentStream()),
              "qsx_select_cmp_columns_blocks");
}

// The literals of an IN leaf as the C ABI takes them (qsx_select_in / qsx_select_in_char): at most QSX_MAX_IN_LIST of them.
struct InListLiterals {
  std::vector<unsigned char> values;   // numeric / DATE: the operand type's bytes, one literal behind the other
  std::vector<char> slots;             // CHAR: QSX_MAX_CHAR_LITERAL bytes each
  std::vector<std::int32_t> lengths;
  int count = 0;
};
InListLiterals MakeInList(const Type &t, const std::vector<TypedLiteral> &literals, std::size_t begin, std::size_t end) {
  InListLiterals out;
  out.count = static_cast<int>(end - begin);
  for (std::size_t k = begin; k < end; ++k) {
    const TypedLiteral &l = literals[k];
    if (l.type != t.id) throw ExecutionError("IN list: a literal whose type differs from the operand's", QSX_ERR_UNSUPPORTED);
    if (t.id == kChar) {
      if (l.text.size() > QSX_MAX_CHAR_LITERAL) throw ExecutionError("IN list: a literal longer than QSX_MAX_CHAR_LITERAL bytes", QSX_ERR_UNSUPPORTED);
      out.slots.resize(out.slots.size() + QSX_MAX_CHAR_LITERAL, 0);
      std::memcpy(out.slots.data() + out.slots.size() - QSX_MAX_CHAR_LITERAL, l.text.data(), l.text.size());
      out.lengths.push_back(static_cast<std::int32_t>(l.text.size()));
    } else {
      const unsigned char *bytes = reinterpret_cast<const unsigned char *>(&l.v);
      out.values.insert(out.values.end(), bytes, bytes + t.width);
    }
  }
  return out;
}

// A leaf of a compiled tree: a term (a comparison, or an IN list when `in` is set) or an attribute's null bitmap.
struct TreeLeaf {
  ComparisonPredicate term;
  std::shared_ptr<InListLiterals> in;
  const std::vector<TypedLiteral> *in_source = nullptr;   // the literals [in_begin, in_end) of it (to recognise the same list twice)
  std::size_t in_begin = 0, in_end = 0;
  attribute_id null_of = kInvalidAttributeID;              // != invalid: the null bitmap of this attribute
};
struct TreeProgram {
  std::vector<TreeLeaf> leaves;
  std::vector<std::int32_t> program;
};
bool SameLiteral(const TypedLiteral &a, const TypedLiteral &b) { return a.type == b.type && a.v.i64 == b.v.i64 && a.text == b.text; }

// has_nulls(a): some block at hand holds a null bitmap for a.  expand_in(a): an IN list over a is written as equalities
// (a truncated attribute without a dictionary: TransformPredicateOnCompressedAttribute rewrites each on the codes).
class TreeCompiler {
 public:
  TreeCompiler(const CatalogRelation &relation, std::function<bool(attribute_id)> has_nulls, std::function<bool(attribute_id)> expand_in,
               TreeProgram *out)
      : relation_(relation), has_nulls_(std::move(has_nulls)), expand_in_(std::move(expand_in)), out_(out) {}
  void compile(const PredicateNode &root) {
    walk(root);
    // what qsx_bitmap_eval takes in one program
    int depth = 0, deepest = 0;
    for (std::int32_t code : out_->program) {
      depth += code >= 0 ? 1 : (code == QSX_BOOL_NOT ? 0 : -1);
      deepest = std::max(deepest, depth);
    }
    if (out_->leaves.size() > QSX_MAX_BOOL_LEAVES || out_->program.size() > QSX_MAX_BOOL_INSTRS || deepest > QSX_MAX_BOOL_DEPTH) {
      throw ExecutionError("predicate tree: more than QSX_MAX_BOOL_LEAVES leaves, QSX_MAX_BOOL_INSTRS instructions or QSX_MAX_BOOL_DEPTH levels",
                           QSX_ERR_UNSUPPORTED);
    }
  }

 private:
  void push(std::int32_t code) { out_->program.push_back(code); }
  // Identical leaves are evaluated once; the same attribute's null bitmap is one leaf.
  int termLeaf(const ComparisonPredicate &term) {
    for (std::size_t k = 0; k < out_->leaves.size(); ++k) {
      const TreeLeaf &l = out_->leaves[k];
      if (l.null_of == kInvalidAttributeID && l.in == nullptr && l.term.attribute == term.attribute && l.term.comparison == term.comparison &&
          SameLiteral(l.term.literal, term.literal) && SameOperand(l.term.operand, term.operand)) {
        return static_cast<int>(k);
      }
    }
    TreeLeaf leaf;
    leaf.term = term;
    out_->leaves.push_back(leaf);
    return static_cast<int>(out_->leaves.size() - 1);
  }
  int inLeaf(const PredicateNode &node, const Type &operand_type, std::size_t begin, std::size_t end) {
    for (std::size_t k = 0; k < out_->leaves.size(); ++k) {
      const TreeLeaf &l = out_->leaves[k];
      // the same operand against the same literals in the same order, wherever in the tree the list was written
      if (l.in == nullptr || l.term.attribute != node.comparison.attribute || !SameOperand(l.term.operand, node.comparison.operand) ||
          l.in_end - l.in_begin != end - begin) {
        continue;
      }
      bool same = true;
      for (std::size_t i = 0; i < end - begin && same; ++i) same = SameLiteral((*l.in_source)[l.in_begin + i], node.in_literals[begin + i]);
      if (same) return static_cast<int>(k);
    }
    TreeLeaf leaf;
    leaf.term = node.comparison;
    leaf.in = std::make_shared<InListLiterals>(MakeInList(operand_type, node.in_literals, begin, end));
    leaf.in_source = &node.in_literals;
    leaf.in_begin = begin;
    leaf.in_end = end;
    out_->leaves.push_back(leaf);
    return static_cast<int>(out_->leaves.size() - 1);
  }
  // `value AND NOT null(a)`: a comparison with a NULL operand is not true (LiteralComparators-inl.hpp:330-370), whatever
  // stands above it — so under a NOT the row IS selected (NegationPredicate.cpp:70-90)
  void clearNulls(attribute_id a) {
    if (!has_nulls_(a)) return;
    int at = -1;
    for (std::size_t k = 0; k < out_->leaves.size(); ++k) if (out_->leaves[k].null_of == a) at = static_cast<int>(k);
    if (at < 0) {
      TreeLeaf leaf;
      leaf.null_of = a;
      out_->leaves.push_back(leaf);
      at = static_cast<int>(out_->leaves.size() - 1);
    }
    push(at);
    push(QSX_BOOL_NOT);
    push(QSX_BOOL_AND);
  }
  void walk(const PredicateNode &node) {
    switch (node.kind) {
      case PredicateNode::kComparison: {
        if (node.comparison.operand != nullptr) CheckUnaryLiteral(CheckUnaryTerm(node.comparison, relation_), node.comparison.literal);
        if (node.comparison.rhs_attribute != kInvalidAttributeID) {
          throw ExecutionError("predicate tree: a comparison of two attributes as a leaf", QSX_ERR_UNSUPPORTED);
        }
        push(termLeaf(node.comparison));
        clearNulls(node.comparison.attribute);
        return;
      }
      case PredicateNode::kInList: {
        // InValueList::concretize (InValueList.cpp:40-65): a disjunction of equalities
        const bool unary = node.comparison.operand != nullptr;
        // the operand's type: the attribute's, or the unary operation's result (an INT, a CHAR(m))
        const Type t = unary ? CheckUnaryTerm(node.comparison, relation_) : relation_.getAttributeType(node.comparison.attribute);
        const attribute_id a = node.comparison.attribute;
        if (node.in_literals.empty()) throw ExecutionError("IN list without a literal", QSX_ERR_INVALID_ARGUMENT);
        if (t.id == kVarChar) throw ExecutionError("IN list on a VARCHAR attribute", QSX_ERR_UNSUPPORTED);
        if (unary) {
          for (const TypedLiteral &l : node.in_literals) CheckUnaryLiteral(t, l);
        }
        if (expand_in_(a)) {
          for (std::size_t k = 0; k < node.in_literals.size(); ++k) {
            if (node.in_literals[k].type != t.id) throw ExecutionError("IN list: a literal whose type differs from the operand's", QSX_ERR_UNSUPPORTED);
            ComparisonPredicate equality(a, ComparisonID::kEqual, node.in_literals[k]);
            equality.operand = node.comparison.operand;
            push(termLeaf(equality));
            if (k > 0) push(QSX_BOOL_OR);
          }
        } else {   // more than QSX_MAX_IN_LIST literals: several IN leaves under an OR
          for (std::size_t begin = 0; begin < node.in_literals.size(); begin += QSX_MAX_IN_LIST) {
            push(inLeaf(node, t, begin, std::min(node.in_literals.size(), begin + QSX_MAX_IN_LIST)));
            if (begin > 0) push(QSX_BOOL_OR);
          }
        }
        clearNulls(a);
        return;
      }
      case PredicateNode::kNegation: {
        if (node.children.size() != 1 || node.children[0] == nullptr) throw ExecutionError("predicate tree: NOT takes one child", QSX_ERR_INVALID_ARGUMENT);
        walk(*node.children[0]);
        push(QSX_BOOL_NOT);
        return;
      }
      default: {
        if (node.children.empty()) throw ExecutionError("predicate tree: AND / OR without a child", QSX_ERR_INVALID_ARGUMENT);
        for (std::size_t k = 0; k < node.children.size(); ++k) {
          if (node.children[k] == nullptr) throw ExecutionError("predicate tree: a null child", QSX_ERR_INVALID_ARGUMENT);
          walk(*node.children[k]);
          if (k > 0) push(node.kind == PredicateNode::kConjunction ? QSX_BOOL_AND : QSX_BOOL_OR);
        }
        return;
      }
    }
  }
  const CatalogRelation &relation_;
  std::function<bool(attribute_id)> has_nulls_, expand_in_;
  TreeProgram *out_;
};

void CollectLeafTerms(const PredicateNode &node, std::vector<const ComparisonPredicate *> *terms) {
  if (node.kind == PredicateNode::kComparison || node.kind == PredicateNode::kInList) {
    terms->push_back(&node.comparison);
    return;
  }
  for (const PredicateNodePtr &child : node.children) if (child != nullptr) CollectLeafTerms(*child, terms);
}

typedef std::vector<std::unique_ptr<DeviceBuffer>> TermScratch;   // what queued kernels of a term still read

// The blocks a term is evaluated over.  `run` false: ONE block (nb == 1), the single-stripe entry points; `run` true: a run of
// blocks, the _blocks entry points — also when the run happens to hold one block.  `ref`: the block a term is classified
// against — the block itself, or the first non-empty block of a run (RunPredicateCovers made the others agree with it).
struct BlockSpan {
  const StorageBlock *const *blocks;
  std::size_t nb;
  const std::int64_t *rows;
  const StorageBlock *ref;
  bool run;
};

// ONE term over a span of blocks into block b's bitmap outs[b] behind filters[b] (filters, or an entry of it, may be null) —
// the one place that turns a term into bitmaps: the conjunction chains and the leaves of a tree, per block and over a run, go
// through it.  One launch (two for a code set); in != nullptr: `term.attribute IN (..)`.  NULLs are the caller's.  The term is
// classified once, against span.ref; the two callers differ only where an entry point is called: a block takes qsx_select_*
// with cols[0], rows[0], its filter and outs[0], a run takes qsx_select_*_blocks.
void SelectTerm(const BlockSpan &span, const ComparisonPredicate &term, const InListLiterals *in, const std::uint64_t *const *filters,
                std::uint64_t *const *outs, std::int64_t *counts, TermScratch *scratch) {
  const std::size_t nb = span.nb;
  const std::int64_t num_blocks = static_cast<std::int64_t>(nb);
  const bool run = span.run;
  const StorageBlock &ref = *span.ref;
  const qsx_stream_t stream = CurrentStream();
  if (in == nullptr && term.operand == nullptr && term.rhs_attribute != kInvalidAttributeID) {
    // attribute OP attribute (ComparisonPredicate.cpp:243-333): one launch, every block's two operands as that block holds them
    SelectAttributeComparison(span.blocks, nb, span.rows, term, filters, outs, counts);
    ++(run ? attribute_comparison_run_evaluations : attribute_comparison_block_evaluations);
    return;
  }
  const bool unary = term.operand != nullptr;
  // (a unary term is checked before anything asks for its attribute: an operand CheckUnaryTerm refuses names none)
  const Type unary_type = unary ? CheckUnaryTerm(term, ref.getRelation()) : Type::Int();
  if (unary && in == nullptr) CheckUnaryLiteral(unary_type, term.literal);
  const Type &t = ref.getRelation().getAttributeType(term.attribute);
  const Type &operand_type = unary ? unary_type : t;   // of a unary term: the operation's result
  const bool like = !unary && in == nullptr && IsLikeComparison(term.comparison);
  if (like) CheckLikeTerm(term, t);
  const int comparison = static_cast<int>(term.comparison), negate = term.comparison == ComparisonID::kNotLike ? 1 : 0;
  const int literal_length = static_cast<int>(term.literal.text.size());
  const std::uint64_t *const filter0 = filters != nullptr ? filters[0] : nullptr;   // (of a block)

  // The term against nb stripes of values — the column stripes, or the dictionaries: then the bitmaps are the blocks' code
  // sets.  A unary operation of the attribute (ComparisonPredicate.cpp:209-240 over ScalarUnaryExpression::getAllValues), an
  // IN list, LIKE (PatternMatchingUncheckedComparator, PatternMatchingComparators-inl.hpp:190-268) or CHAR(n) OP string
  // literal (AsciiStringUncheckedComparator, AsciiStringComparators.hpp:218-251).
  const auto select_values = [&](int width, const std::int64_t *n, const void *const *cols, const std::uint64_t *const *f,
                                 std::uint64_t *const *bitmaps, std::int64_t *bitmap_counts) {
    const std::uint64_t *const f0 = f != nullptr ? f[0] : nullptr;
    if (unary) {
      const qsx_unary_operand_t operand = UnaryOperandOf(*term.operand);
      const bool text = operand_type.id == kChar;
      if (in != nullptr) {
        const void *literals = text ? static_cast<const void *>(in->slots.data()) : in->values.data();
        const std::int32_t *lengths = text ? in->lengths.data() : nullptr;
        CheckStatus(run ? qsx_select_in_unary_blocks(&operand, width, num_blocks, n, cols, literals, lengths, in->count, 0, f, bitmaps, bitmap_counts, stream)
                        : qsx_select_in_unary(&operand, cols[0], width, n[0], literals, lengths, in->count, 0, f0, bitmaps[0], bitmap_counts, stream),
                    run ? "qsx_select_in_unary_blocks" : "qsx_select_in_unary");
      } else {
        const void *literal = text ? static_cast<const void *>(term.literal.text.data()) : &term.literal.v.i32;
        const int length = text ? literal_length : 0;
        CheckStatus(run ? qsx_select_cmp_unary_blocks(&operand, width, num_blocks, n, cols, comparison, literal, length, f, bitmaps, bitmap_counts, stream)
                        : qsx_select_cmp_unary(&operand, cols[0], width, n[0], comparison, literal, length, f0, bitmaps[0], bitmap_counts, stream),
                    run ? "qsx_select_cmp_unary_blocks" : "qsx_select_cmp_unary");
      }
    } else if (in != nullptr && t.id == kChar) {
      CheckStatus(run ? qsx_select_in_char_blocks(width, num_blocks, n, cols, in->slots.data(), in->lengths.data(), in->count, 0, f, bitmaps, bitmap_counts, stream)
                      : qsx_select_in_char(cols[0], width, n[0], in->slots.data(), in->lengths.data(), in->count, 0, f0, bitmaps[0], bitmap_counts, stream),
                  run ? "qsx_select_in_char_blocks" : "qsx_select_in_char");
    } else if (in != nullptr) {
      CheckStatus(run ? qsx_select_in_blocks(t.id, num_blocks, n, cols, in->values.data(), in->count, 0, f, bitmaps, bitmap_counts, stream)
                      : qsx_select_in(t.id, cols[0], n[0], in->values.data(), in->count, 0, f0, bitmaps[0], bitmap_counts, stream),
                  run ? "qsx_select_in_blocks" : "qsx_select_in");
    } else if (!run) {
      SelectCharTerm(term, cols[0], width, n[0], f0, bitmaps[0], bitmap_counts);   // (qsx_select_like / qsx_select_cmp_char)
    } else if (like) {
      CheckStatus(qsx_select_like_blocks(width, num_blocks, n, cols, term.literal.text.data(), literal_length, negate, f, bitmaps, bitmap_counts, stream),
                  "qsx_select_like_blocks");
    } else {
      CheckStatus(qsx_select_cmp_char_blocks(width, num_blocks, n, cols, comparison, term.literal.text.data(), literal_length, f, bitmaps, bitmap_counts,
                                             stream), "qsx_select_cmp_char_blocks");
    }
  };

  const CompressedAttribute *c = ref.compressedAttribute(term.attribute);   // (an empty single block has none: the plain entries with n = 0)
  // A term whose matches are a set of the dictionary's codes: LIKE, an IN list on a dictionary, a unary term on a dictionary it can
  // be evaluated over (UnaryOnDictionary: fixed-width, and 8-byte aligned if of dates) — on the sort column too, a set is no range.
  const bool code_set = unary ? UnaryOnDictionary(ref, term.attribute, t)
                              : c != nullptr && (like || (in != nullptr && c->kind == CompressedAttribute::kDictionary));
  if (code_set) {
    // The pattern, the list or the term against every block's dictionary once — block b's code set —, then the code stripes
    // tested for membership in their block's set.  The reference runs the matcher on every decompressed value
    // (PatternMatchingComparators-inl.hpp:190-268); the values are not materialized here.
    const bool variable = c->variable_length;   // a VARCHAR attribute: the variable-length dictionaries where the images hold them
    if (variable && !like) throw ExecutionError("IN list on a VARCHAR attribute", QSX_ERR_UNSUPPORTED);
    std::vector<std::int64_t> num_codes(nb, 0), value_bytes(nb, 0);
    std::vector<const void *> codes(nb, nullptr), dictionaries(nb, nullptr);
    std::vector<const std::uint32_t *> offsets(nb, nullptr);
    std::vector<std::uint64_t *> sets(nb, nullptr);
    std::size_t set_words = 0;
    int value_width = t.width;
    for (std::size_t b = 0; b < nb; ++b) {
      const CompressedAttribute *cb = span.blocks[b]->compressedAttribute(term.attribute);
      if (cb == nullptr) continue;   // (an empty block of a run)
      codes[b] = cb->codes;
      num_codes[b] = cb->num_codes;
      if (!variable) {
        dictionaries[b] = cb->dictionary;
        value_width = cb->value_width;
      } else if (cb->num_codes != 0) {
        dictionaries[b] = cb->variable_values;
        offsets[b] = cb->variable_offsets;
        value_bytes[b] = static_cast<std::int64_t>(cb->variable_value_bytes);
      }
      set_words += static_cast<std::size_t>((cb->num_codes + 63) / 64) + 1;
    }
    // (num_codes + 63) / 64 words and one more per set; a run's buffer ends in one more word
    scratch->emplace_back(new DeviceBuffer(set_words * 8 + (run ? 8 : 0)));
    std::size_t set_at = 0;
    for (std::size_t b = 0; b < nb; ++b) {
      sets[b] = static_cast<std::uint64_t *>(scratch->back()->ptr) + set_at;
      set_at += static_cast<std::size_t>((num_codes[b] + 63) / 64) + (num_codes[b] != 0 ? 1 : 0);
    }
    if (variable) {   // (a block passes its dictionary as it is, a run NULLs for a dictionary without entries)
      CheckStatus(run ? qsx_select_like_var_blocks(t.width, num_blocks, num_codes.data(), offsets.data(), dictionaries.data(), value_bytes.data(),
                                                   term.literal.text.data(), literal_length, negate, nullptr, sets.data(), nullptr, stream)
                      : qsx_select_like_var(c->variable_offsets, c->variable_values, c->num_codes, static_cast<std::int64_t>(c->variable_value_bytes),
                                            t.width, term.literal.text.data(), literal_length, negate, nullptr, sets[0], nullptr, stream),
                  run ? "qsx_select_like_var_blocks" : "qsx_select_like_var");
    } else {
      select_values(unary && t.id == kDate ? 8 : value_width, num_codes.data(), dictionaries.data(), nullptr, sets.data(), nullptr);
    }
    CheckStatus(run ? qsx_select_codes_in_set_blocks(c->code_width, num_blocks, span.rows, codes.data(), sets.data(), num_codes.data(), filters, outs,
                                                     counts, stream)
                    : qsx_select_codes_in_set(c->code_width, codes[0], span.rows[0], sets[0], num_codes[0], filter0, outs[0], counts, stream),
                run ? "qsx_select_codes_in_set_blocks" : "qsx_select_codes_in_set");
  } else if (c != nullptr && !unary) {
    // CompressedTupleStorageSubBlock::getMatchesForPredicate (storage/CompressedTupleStorageSubBlock.cpp:160-250): the
    // comparison rewritten on every block's own codes, then the code stripes scanned — or, on the sort column of a compressed
    // store, searched: the codes ascend, the matches are one range (CompressedColumnStoreTupleStorageSubBlock.cpp:420-760).
    // (An IN list over truncated codes is K equalities in the tree's program: TreeCompiler, expand_in.)
    if (in != nullptr) throw ExecutionError("IN list over a truncated attribute reached the leaf evaluator", QSX_ERR_INVALID_ARGUMENT);
    std::vector<const void *> codes(nb, nullptr);
    std::vector<std::int32_t> ops(nb, QSX_CODE_LT);   // (an empty block of a run: no code)
    std::vector<std::uint32_t> firsts(nb, 0), seconds(nb, 0);
    bool all_or_none = false;   // (of the last block)
    for (std::size_t b = 0; b < nb; ++b) {
      const CompressedAttribute *cb = span.blocks[b]->compressedAttribute(term.attribute);
      if (cb == nullptr) continue;
      const PredicateTransformResult r = TransformPredicateOnCompressedAttribute(*cb, t.id, term.comparison, term.literal);
      codes[b] = cb->codes;
      all_or_none = r.type == PredicateTransformResult::kAll || r.type == PredicateTransformResult::kNone;
      if (all_or_none) {
        ops[b] = r.type == PredicateTransformResult::kAll ? QSX_CODE_GE : QSX_CODE_LT;   // every code / no code: code >= 0 resp. code < 0
      } else {
        ops[b] = r.comp;
        firsts[b] = r.first_literal;
        seconds[b] = r.second_literal;
      }
    }
    // A single block whose rewrite is every code / no code is scanned on its sort column too; a run searches every block.
    if (term.attribute == ref.sortColumn() && (run || !all_or_none)) {
      CheckStatus(run ? qsx_select_codes_sorted_blocks(c->code_width, num_blocks, span.rows, codes.data(), ops.data(), firsts.data(), seconds.data(),
                                                       filters, outs, counts, stream)
                      : qsx_select_codes_sorted(c->code_width, codes[0], span.rows[0], ops[0], firsts[0], seconds[0], filter0, outs[0], counts, stream),
                  run ? "qsx_select_codes_sorted_blocks" : "qsx_select_codes_sorted");
    } else {
      CheckStatus(run ? qsx_select_codes_blocks(c->code_width, num_blocks, span.rows, codes.data(), ops.data(), firsts.data(), seconds.data(), filters,
                                                outs, counts, stream)
                      : qsx_select_codes(c->code_width, codes[0], span.rows[0], ops[0], firsts[0], seconds[0], filter0, outs[0], counts, stream),
                  run ? "qsx_select_codes_blocks" : "qsx_select_codes");
    }
  } else {
    // Stripes of values.  For a unary term on a compressed attribute without a dictionary it can be evaluated over (truncated
    // values, a variable-length dictionary, a date dictionary that is not 8-byte aligned) stripe() is the decoded stripe: a
    // single block reads it, RunPredicateCovers keeps that shape off the run path.
    std::vector<const void *> stripes(nb);
    for (std::size_t b = 0; b < nb; ++b) stripes[b] = span.blocks[b]->stripe(term.attribute);
    if (unary || in != nullptr || IsTextType(t.id)) {   // (a plain VARCHAR(n) stripe holds CHAR(n) fields)
      select_values(unary ? UnaryStripeWidth(t) : t.width, span.rows, stripes.data(), filters, outs, counts);
    } else if (term.attribute == ref.sortColumn()) {
      // the blocks are sorted on this attribute: SortColumnPredicateEvaluator (storage/ColumnStoreUtil.cpp:40-280), one search per block
      CheckStatus(run ? qsx_select_cmp_sorted_blocks(t.id, num_blocks, span.rows, stripes.data(), comparison, &term.literal.v, filters, outs, counts, stream)
                      : qsx_select_cmp_sorted(t.id, stripes[0], span.rows[0], comparison, &term.literal.v, filter0, outs[0], counts, stream),
                  run ? "qsx_select_cmp_sorted_blocks" : "qsx_select_cmp_sorted");
    } else {
      CheckStatus(run ? qsx_select_cmp_blocks(t.id, num_blocks, span.rows, stripes.data(), comparison, &term.literal.v, filters, outs, counts, stream)
                      : qsx_select_cmp(t.id, stripes[0], span.rows[0], comparison, &term.literal.v, filter0, outs[0], counts, stream),
                  run ? "qsx_select_cmp_blocks" : "qsx_select_cmp");
    }
  }
  if (unary) ++(run ? unary_run_evaluations : unary_block_evaluations);
}

// The tree over a span of blocks: every leaf without a filter into bitmaps of its own (SelectTerm), a nullable attribute's null
// bitmap as one more leaf, then ONE qsx_bitmap_eval(_blocks) behind `filters` into outs / counts.  What the queued kernels read
// goes to `scratch`.
void EvaluateTree(const BlockSpan &span, const PredicateNode &tree, const std::uint64_t *const *filters, std::uint64_t *const *outs,
                  std::int64_t *counts, TermScratch *scratch) {
  const std::size_t nb = span.nb;
  TreeProgram compiled;
  TreeCompiler(span.ref->getRelation(),
               [&](attribute_id a) {
                 for (std::size_t b = 0; b < nb; ++b) if (span.blocks[b]->nullBitmap(a) != nullptr) return true;
                 return false;
               },
               [&](attribute_id a) {   // one program for the span: equalities as soon as one block's codes are truncated values
                 for (std::size_t b = 0; b < nb; ++b) {
                   // (a run passes over its empty blocks; a single block is asked whatever it holds)
                   const CompressedAttribute *c = span.run && span.blocks[b]->numTuples() == 0 ? nullptr : span.blocks[b]->compressedAttribute(a);
                   if (c != nullptr && c->kind != CompressedAttribute::kDictionary) return true;
                 }
                 return false;
               }, &compiled).compile(tree);
  std::size_t bitmap_words = 0;
  for (std::size_t b = 0; b < nb; ++b) bitmap_words += static_cast<std::size_t>((span.rows[b] + 63) / 64) + 1;
  const std::size_t num_leaves = compiled.leaves.size();
  scratch->emplace_back(new DeviceBuffer(num_leaves * bitmap_words * 8 + 8));
  std::uint64_t *leaf_storage = static_cast<std::uint64_t *>(scratch->back()->ptr);
  std::vector<const std::uint64_t *> block_leaves(nb * num_leaves, nullptr);   // block b's leaf k at [b * num_leaves + k]
  std::vector<std::uint64_t *> leaf_outs(nb);
  for (std::size_t k = 0; k < num_leaves; ++k) {
    const TreeLeaf &leaf = compiled.leaves[k];
    std::size_t leaf_at = k * bitmap_words;
    for (std::size_t b = 0; b < nb; ++b) {
      leaf_outs[b] = leaf_storage + leaf_at;
      leaf_at += static_cast<std::size_t>((span.rows[b] + 63) / 64) + 1;
      // NULL is the all-zero leaf: for a block without a null bitmap, and for every leaf of a run's empty block
      if (span.run && span.rows[b] == 0) continue;
      block_leaves[b * num_leaves + k] = leaf.null_of != kInvalidAttributeID ? span.blocks[b]->nullBitmap(leaf.null_of) : leaf_outs[b];
    }
    if (leaf.null_of == kInvalidAttributeID) SelectTerm(span, leaf.term, leaf.in.get(), nullptr, leaf_outs.data(), nullptr, scratch);
  }
  if (span.run) {
    CheckStatus(qsx_bitmap_eval_blocks(static_cast<int>(num_leaves), static_cast<int>(compiled.program.size()), compiled.program.data(),
                                       static_cast<std::int64_t>(nb), span.rows, block_leaves.data(), filters, outs, counts, CurrentStream()),
                "qsx_bitmap_eval_blocks");
    ++tree_run_evaluations;
  } else {
    CheckStatus(qsx_bitmap_eval(static_cast<int>(num_leaves), block_leaves.data(), static_cast<int>(compiled.program.size()), compiled.program.data(),
                                span.rows[0], filters != nullptr ? filters[0] : nullptr, outs[0], counts, CurrentStream()), "qsx_bitmap_eval");
    ++tree_block_evaluations;
  }
}
}  // namespace

std::int64_t NumPredicateTreeBlockEvaluations() { return tree_block_evaluations.load(); }
std::int64_t NumPredicateTreeRunEvaluations() { return tree_run_evaluations.load(); }
std::int64_t NumAttributeComparisonBlockEvaluations() { return attribute_comparison_block_evaluations.load(); }
std::int64_t NumAttributeComparisonRunEvaluations() { return attribute_comparison_run_evaluations.load(); }
std::int64_t NumUnaryPredicateBlockEvaluations() { return unary_block_evaluations.load(); }
std::int64_t NumUnaryPredicateRunEvaluations() { return unary_run_evaluations.load(); }

void LowerPredicateToAggConfig(const Predicate &predicate, const CatalogRelation &relation, const std::function<int(attribute_id)> &column_of,
                               qsx_agg_config_t *config, Predicate *external) {
  const auto keep_out = [&](const char *what) {
    if (external == nullptr) throw ExecutionError(std::string("qsx_agg_config_t.pred cannot hold ") + what, QSX_ERR_UNSUPPORTED);
  };
  int in_state = 0;
  for (const ComparisonPredicate &term : predicate.conjuncts) {
    if (term.operand != nullptr) {
      // qsx_agg_config_t.pred names a column: a term over a unary operation is the external predicate's
      CheckUnaryLiteral(CheckUnaryTerm(term, relation), term.literal);
      keep_out("a term over a unary operation (EXTRACT / SUBSTRING)");
      external->conjuncts.push_back(term);
      continue;
    }
    const Type &t = relation.getAttributeType(term.attribute);
    if (IsLikeComparison(term.comparison)) CheckLikeTerm(term, t);   // (a CHAR(n) term: evaluated by Predicate)
    if (IsTextType(t.id) || term.rhs_attribute != kInvalidAttributeID || in_state == QSX_MAX_PRED_TERMS) {
      keep_out("a CHAR(n) term, a comparison of two attributes or more than QSX_MAX_PRED_TERMS terms");
      external->conjuncts.push_back(term);   // string comparisons, attribute-vs-attribute, overflow
      continue;
    }
    config->pred[in_state].column = column_of(term.attribute);
    config->pred[in_state].op = static_cast<int>(term.comparison);
    std::memcpy(&config->pred[in_state].literal, &term.literal.v, sizeof(term.literal.v));
    ++in_state;
  }
  config->num_pred_terms = in_state;
  if (predicate.tree != nullptr) {
    // a tree (OR / NOT / IN) is no list of terms: it goes to the state's external predicate, evaluated block by block into the
    // update's filter like CHAR(n) terms
    keep_out("a predicate tree (OR / NOT / IN)");
    external->tree = predicate.tree;
  }
}

void *Predicate::getMatchesForBlock(const StorageBlock &block, std::int64_t *num_matches, const std::uint64_t *filter) const {
  const std::int64_t n = block.numTuples();
  const std::size_t words = static_cast<std::size_t>((n + 63) / 64);
  void *current = nullptr, *next = nullptr, *count = nullptr;
  CheckStatus(qsx_device_alloc(words * 8 + 8, &current), "qsx_device_alloc(bitmap)");
  CheckStatus(qsx_device_alloc(words * 8 + 8, &next), "qsx_device_alloc(bitmap)");
  CheckStatus(qsx_device_alloc(8, &count), "qsx_device_alloc(count)");
  bool first = true;
  bool recount = false;
  TermScratch scratch;   // code sets, leaf bitmaps (read by queued kernels: kept until the count has been read)
  const StorageBlock *const one = &block;
  const BlockSpan span{&one, 1, &n, one, false};   // (a block, not a run of one: the single-stripe entry points)
  try {
    for (const ComparisonPredicate &term : conjuncts) {
      const std::uint64_t *in = first ? filter : static_cast<const std::uint64_t *>(current);
      std::uint64_t *const out = static_cast<std::uint64_t *>(next);
      // conjunctions chain the filter through their children (short-circuit)
      SelectTerm(span, term, nullptr, in != nullptr ? &in : nullptr, &out, static_cast<std::int64_t *>(count), &scratch);
      // a comparison with NULL is not true (LiteralComparators-inl.hpp:330-370: the nullable variants test the value
      // pointer first): the stripe holds an arbitrary value under a NULL, so its match is taken back — for either operand of a
      // comparison of two attributes
      for (const attribute_id a : {term.attribute, term.rhs_attribute}) {
        if (a == kInvalidAttributeID || block.nullBitmap(a) == nullptr || n == 0) continue;
        CheckStatus(qsx_bitmap_combine(2, static_cast<const std::uint64_t *>(next), block.nullBitmap(a), n,
                                       static_cast<std::uint64_t *>(next), CurrentStream()), "qsx_bitmap_combine");
        recount = true;
      }
      std::swap(current, next);
      first = false;
    }
    if (tree != nullptr) {
      // AND(conjuncts) AND tree: the chain's result (or the incoming filter) is the evaluator's filter, applied once at the root —
      // leaves are pure functions of the row, so this equals the reference's short-circuit filtering
      const std::uint64_t *in = first ? filter : static_cast<const std::uint64_t *>(current);
      std::uint64_t *const out = static_cast<std::uint64_t *>(next);
      EvaluateTree(span, *tree, in != nullptr ? &in : nullptr, &out, static_cast<std::int64_t *>(count), &scratch);
      std::swap(current, next);
      first = false;
      recount = false;   // (the evaluator counted)
    }
    if (recount) {
      CheckStatus(qsx_bitmap_count(static_cast<const std::uint64_t *>(current), n, static_cast<std::int64_t *>(count), CurrentStream()),
                  "qsx_bitmap_count");
    }
    if (first) {  // empty conjunction: every tuple (of the filter) matches
      CheckStatus(qsx_memset_device(next, 0xFF, words * 8, CurrentStream()), "qsx_memset_device");
      CheckStatus(qsx_bitmap_combine(0, static_cast<const std::uint64_t *>(next),
                                     filter != nullptr ? filter : static_cast<const std::uint64_t *>(next), n,
                                     static_cast<std::uint64_t *>(current), CurrentStream()), "qsx_bitmap_combine");
      CheckStatus(qsx_bitmap_count(static_cast<const std::uint64_t *>(current), n, static_cast<std::int64_t *>(count),
                                   CurrentStream()), "qsx_bitmap_count");
    }
    *num_matches = ReadCount(count);
  } catch (...) {
    qsx_stream_synchronize(CurrentStream());
    qsx_device_free(current);
    qsx_device_free(next);
    qsx_device_free(count);
    throw;
  }
  qsx_device_free(next);
  qsx_device_free(count);
  return current;
}

// ---------------------------------------------------------------------------
// A predicate over a RUN of blocks (the SelectOperator's work orders over runs; the aggregation over runs of compressed blocks)
// ---------------------------------------------------------------------------
// Can the run forms evaluate `predicate` over these blocks in one launch per term?  Terms against a literal, every block coding
// and ordering a term's attribute like the first non-empty one; a term of the conjunction chain on attributes without NULLs.
// The leaves of a tree keep a nullable attribute on the run path: its null bitmap is one more leaf of the program, absent
// (NULL) for the blocks that hold none.
bool RunPredicateCovers(const Predicate &predicate, const std::vector<BlockReference> &blocks) {
  const StorageBlock *reference_block = nullptr;   // the first non-empty block: what the others have to agree with
  std::vector<const ComparisonPredicate *> leaf_terms;
  if (predicate.tree != nullptr) CollectLeafTerms(*predicate.tree, &leaf_terms);
  for (const BlockReference &block : blocks) {
    const StorageBlock &b = *block;
    const auto term_agrees = [&](const ComparisonPredicate &term, bool nulls_allowed, bool like) {
      if (term.operand != nullptr) {
        // a unary operation of the attribute: plain stripes in every block, or a dictionary the term can be evaluated over in
        // every block (the other compressed forms take the per-block path and its decoded stripe); no order is used
        CheckUnaryTerm(term, b.getRelation());
        if (!nulls_allowed && b.nullBitmap(term.attribute) != nullptr) return false;
        if (b.numTuples() == 0) return true;
        const CompressedAttribute *cb = b.compressedAttribute(term.attribute);
        if (cb != nullptr && !UnaryOnDictionary(b, term.attribute, b.getRelation().getAttributeType(term.attribute))) return false;
        if (reference_block == nullptr) reference_block = &b;
        const CompressedAttribute *cf = reference_block->compressedAttribute(term.attribute);
        return (cb != nullptr) == (cf != nullptr) && (cb == nullptr || cb->code_width == cf->code_width);
      }
      const Type &t = b.getRelation().getAttributeType(term.attribute);
      if (like) CheckLikeTerm(term, t);
      if (term.rhs_attribute != kInvalidAttributeID) {
        // attribute OP attribute: as a leaf it is refused (the per-block path says so); as a conjunct it stays on the run path —
        // coding is per block and per side in qsx_select_cmp_columns_blocks, so the blocks need not agree on anything; a
        // nullable operand sends the run to the per-block path like the other conjuncts
        if (nulls_allowed) return false;
        CheckAttributeComparison(term, b.getRelation());
        return b.nullBitmap(term.attribute) == nullptr && b.nullBitmap(term.rhs_attribute) == nullptr;
      }
      if (!nulls_allowed && b.nullBitmap(term.attribute) != nullptr) return false;
      if (b.numTuples() == 0) return true;              // (an empty block has neither codes nor an order to agree on)
      // a term on the blocks' sort column is a per-block binary search (also on the code stripe of a compressed sort column), a
      // term on a compressed attribute a scan of the code stripes with the comparison rewritten per block
      if (IsTextType(t.id) && b.compressedAttribute(term.attribute) == nullptr && term.attribute == b.sortColumn()) return false;
      if (reference_block == nullptr) reference_block = &b;
      const StorageBlock &f = *reference_block;
      if ((term.attribute == b.sortColumn()) != (term.attribute == f.sortColumn())) return false;
      const CompressedAttribute *cb = b.compressedAttribute(term.attribute), *cf = f.compressedAttribute(term.attribute);
      if ((cb != nullptr) != (cf != nullptr) || (cb != nullptr && cb->code_width != cf->code_width)) return false;
      return true;
    };
    for (const ComparisonPredicate &term : predicate.conjuncts) {
      if (!term_agrees(term, false, IsLikeComparison(term.comparison))) return false;
    }
    for (const ComparisonPredicate *term : leaf_terms) {   // (an IN leaf's comparison is kEqual)
      if (!term_agrees(*term, true, IsLikeComparison(term->comparison))) return false;
    }
  }
  return true;
}

// The TupleIdSequences of the run's blocks under `predicate` (RunPredicateCovers said yes), every term one launch over the run,
// chained like a conjunction behind `in_filters` (per block, entries may be null; or nullptr); then the tree: every leaf one
// launch over the run into bitmaps of its own, and ONE qsx_bitmap_eval_blocks behind the chain's result.  out->bitmaps[b] is
// block b's bitmap, out->counts the per-block match counts of the last launch (device memory).
void RunPredicateMatches(const Predicate &predicate, const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows,
                         const std::uint64_t *const *in_filters, RunMatches *out) {
  const std::size_t nb = blocks.size();
  std::size_t bitmap_words = 0;
  const StorageBlock *reference_block = blocks.empty() ? nullptr : blocks.front().get();
  std::vector<const StorageBlock *> plain(nb);
  for (std::size_t b = 0; b < nb; ++b) {
    plain[b] = blocks[b].get();
    bitmap_words += static_cast<std::size_t>((rows[b] + 63) / 64) + 1;
    if (reference_block != nullptr && reference_block->numTuples() == 0 && blocks[b]->numTuples() != 0) reference_block = blocks[b].get();
  }
  const BlockSpan span{plain.data(), nb, rows.data(), reference_block, true};   // (a run, also when nb == 1: the _blocks entry points)
  // two sets of per-block bitmaps in two allocations, the terms ping-pong between them
  out->set_a.reset(new DeviceBuffer(bitmap_words * 8 + 8));
  out->set_b.reset(new DeviceBuffer(bitmap_words * 8 + 8));
  out->counts.reset(new DeviceBuffer(nb * 8 + 8));
  std::vector<std::uint64_t *> cur(nb), nxt(nb);
  std::size_t at = 0;
  for (std::size_t b = 0; b < nb; ++b) {
    cur[b] = static_cast<std::uint64_t *>(out->set_a->ptr) + at;
    nxt[b] = static_cast<std::uint64_t *>(out->set_b->ptr) + at;
    at += static_cast<std::size_t>((rows[b] + 63) / 64) + 1;
  }
  bool first = true;
  for (const ComparisonPredicate &term : predicate.conjuncts) {
    const std::uint64_t *const *in = first ? in_filters : reinterpret_cast<const std::uint64_t *const *>(cur.data());
    SelectTerm(span, term, nullptr, in, nxt.data(), static_cast<std::int64_t *>(out->counts->ptr), &out->scratch);
    std::swap(cur, nxt);
    first = false;
  }
  if (predicate.tree != nullptr && nb > 0) {
    // AND(conjuncts) AND tree, as in getMatchesForBlock: the chain's result (or the incoming filters) is the evaluator's filter
    EvaluateTree(span, *predicate.tree, first ? in_filters : reinterpret_cast<const std::uint64_t *const *>(cur.data()), nxt.data(),
                 static_cast<std::int64_t *>(out->counts->ptr), &out->scratch);
    std::swap(cur, nxt);
  }
  out->bitmaps = cur;
}

// ---------------------------------------------------------------------------
// InsertDestination
// ---------------------------------------------------------------------------
BlockReference InsertDestination::getBlockForInsertion(std::int64_t capacity, block_id *id) {
  *id = storage_manager_->createBlock(relation_, capacity);
  return storage_manager_->getBlock(*id);
}
void InsertDestination::returnBlock(block_id id, std::int64_t num_tuples, partition_id input_partition) {
  if (isPartitionAware()) {
    repartitionBlock(id, num_tuples);
    return;
  }
  BlockReference block = storage_manager_->getBlock(id);
  block->setNumTuples(num_tuples);
  block->setFirstRow(storage_manager_->reserveRows(relation_->getID(), num_tuples));
  {
    std::lock_guard<std::mutex> lock(mutex_);
    touched_.push_back(TouchedBlock{id, input_partition});
    if (relation_->hasPartitionScheme()) {
      relation_->addBlockToPartition(id, input_partition);   // the output keeps the input's partitioning (no repartition)
    } else {
      relation_->addBlock(id);
    }
  }
  if (block_returned_) block_returned_();
}

// bulkInsertTuples of a PartitionAwareInsertDestination over every tuple of a run of input blocks: one K9 pass that finds the
// blocks' stripes through a table — against a copy of the run into one block (two more trips through HBM) and K9 over that.
bool InsertDestination::insertRunRepartitioned(const std::vector<BlockReference> &blocks, const std::vector<attribute_id> &attributes) {
  if (!isPartitionAware() || blocks.empty() || attributes.size() != relation_->size() || attributes.size() > QSX_MAX_COLUMNS) return false;
  const std::size_t P = num_partitions_;
  const Type &key_type = relation_->getAttributeType(partition_attribute_);
  if ((key_type.id != kInt && key_type.id != kLong) || P > 64) return false;   // (repartitionBlock reports these)
  for (std::size_t a = 0; a < relation_->size(); ++a) {
    const Type &t = relation_->getAttributeType(static_cast<attribute_id>(a));
    if (t.nullable || (t.width != 1 && t.width != 2 && t.width != 4 && t.width != 8)) return false;
  }
  std::vector<std::int64_t> rows;
  std::vector<const void *> keys, cols;
  std::vector<std::int32_t> widths;
  std::int64_t total = 0;
  for (const BlockReference &b : blocks) {
    for (attribute_id a : attributes) {
      if (b->nullBitmap(a) != nullptr) return false;
    }
    rows.push_back(b->numTuples());
    total += b->numTuples();
    keys.push_back(b->numTuples() > 0 ? b->stripe(attributes[partition_attribute_]) : nullptr);
    for (attribute_id a : attributes) cols.push_back(b->numTuples() > 0 ? b->stripe(a) : nullptr);
  }
  if (total == 0) return true;
  for (std::size_t a = 0; a < relation_->size(); ++a) widths.push_back(relation_->getAttributeType(static_cast<attribute_id>(a)).width);
  block_id scattered_id;
  BlockReference scattered = getBlockForInsertion(total, &scattered_id);
  scattered->setNumTuples(total);
  std::vector<void *> outs;
  for (std::size_t a = 0; a < relation_->size(); ++a) outs.push_back(scattered->stripe(static_cast<attribute_id>(a)));
  const std::size_t ws_bytes = qsx_partition_blocks_workspace_bytes(total, static_cast<std::int64_t>(blocks.size()), static_cast<int>(P));
  DeviceBuffer ws(ws_bytes + 8), offsets_dev((P + 1) * 8);
  CheckStatus(qsx_partition_scatter_blocks(key_type.id, static_cast<std::int64_t>(blocks.size()), rows.data(), keys.data(), static_cast<int>(P),
                                           static_cast<int>(widths.size()), cols.data(), widths.data(), outs.data(),
                                           static_cast<std::int64_t *>(offsets_dev.ptr), ws.ptr, ws_bytes, CurrentStream()),
              "qsx_partition_scatter_blocks");
  std::vector<std::int64_t> offsets(P + 1);
  CheckStatus(qsx_copy_to_host(offsets.data(), offsets_dev.ptr, (P + 1) * 8, CurrentStream()), "qsx_copy_to_host");
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // (the work order's wait; ws goes out of scope)
  std::vector<std::pair<block_id, partition_id>> made;
  for (std::size_t p = 0; p < P; ++p) {
    const std::int64_t first = offsets[p], rows_p = offsets[p + 1] - offsets[p];
    if (rows_p == 0) continue;
    const block_id view_id = storage_manager_->createViewBlock(scattered_id, first, rows_p);
    storage_manager_->getBlock(view_id)->setFirstRow(storage_manager_->reserveRows(relation_->getID(), rows_p));
    made.emplace_back(view_id, p);
  }
  storage_manager_->deleteBlockOrBlobFile(scattered_id);      // (the views keep the scattered block alive)
  {
    std::lock_guard<std::mutex> lock(mutex_);
    for (const auto &m : made) {
      touched_.push_back(TouchedBlock{m.first, m.second});
      relation_->addBlockToPartition(m.first, m.second);
    }
  }
  if (block_returned_ && !made.empty()) block_returned_();
  return true;
}

// bulkInsertTuples of a PartitionAwareInsertDestination (storage/InsertDestination.hpp:560-660), on a whole block at once:
// K9 scatters the columns of 1 / 2 / 4 / 8 bytes and a row-number column by the partition of the partition attribute; wider
// columns (CHAR(n)) and the null bits follow through the scattered row numbers; the scattered block is then cut into one
// block per partition (views: no copy).
void InsertDestination::repartitionBlock(block_id id, std::int64_t num_tuples) {
  BlockReference src = storage_manager_->getBlock(id);
  src->setNumTuples(num_tuples);
  const std::size_t P = num_partitions_;
  const Type &key_type = relation_->getAttributeType(partition_attribute_);
  if (key_type.id != kInt && key_type.id != kLong) {
    throw ExecutionError("PartitionAwareInsertDestination: the partition attribute must be INT or LONG", QSX_ERR_UNSUPPORTED);
  }
  if (P > 64) throw ExecutionError("PartitionAwareInsertDestination: more than 64 partitions", QSX_ERR_UNSUPPORTED);
  if (num_tuples == 0) {
    storage_manager_->deleteBlockOrBlobFile(id);
    return;
  }
  block_id scattered_id;
  BlockReference scattered = getBlockForInsertion(num_tuples, &scattered_id);
  scattered->setNumTuples(num_tuples);
  bool need_rows = false;
  std::vector<const void *> cols;
  std::vector<void *> outs;
  std::vector<std::int32_t> widths;
  for (std::size_t a = 0; a < relation_->size(); ++a) {
    const Type &t = relation_->getAttributeType(static_cast<attribute_id>(a));
    if (t.nullable) need_rows = true;
    if (t.width == 1 || t.width == 2 || t.width == 4 || t.width == 8) {
      cols.push_back(src->stripe(static_cast<attribute_id>(a)));
      outs.push_back(scattered->stripe(static_cast<attribute_id>(a)));
      widths.push_back(t.width);
    } else {
      need_rows = true;
    }
  }
  std::unique_ptr<DeviceBuffer> rows, rows_scattered;
  if (need_rows) {
    // row numbers 0 .. n-1: the tuple ids of an all-ones TupleIdSequence (NOT of a zeroed one: trailing bits stay zero)
    const std::size_t words = static_cast<std::size_t>((num_tuples + 63) / 64) + 1;
    DeviceBuffer zero(words * 8), ones(words * 8), count(8);
    CheckStatus(qsx_memset_device(zero.ptr, 0, words * 8, CurrentStream()), "qsx_memset_device");
    CheckStatus(qsx_bitmap_combine(3, static_cast<const std::uint64_t *>(zero.ptr), nullptr, num_tuples, static_cast<std::uint64_t *>(ones.ptr),
                                   CurrentStream()), "qsx_bitmap_combine");
    rows.reset(new DeviceBuffer(static_cast<std::size_t>(num_tuples) * 4 + 8));
    rows_scattered.reset(new DeviceBuffer(static_cast<std::size_t>(num_tuples) * 4 + 8));
    const std::size_t tws = qsx_compact_workspace_bytes(num_tuples);
    DeviceBuffer tw(tws + 8);
    CheckStatus(qsx_bitmap_to_tids(static_cast<const std::uint64_t *>(ones.ptr), num_tuples, 0, static_cast<std::int32_t *>(rows->ptr),
                                   static_cast<std::int64_t *>(count.ptr), tw.ptr, tws, CurrentStream()), "qsx_bitmap_to_tids");
    cols.push_back(rows->ptr);
    outs.push_back(rows_scattered->ptr);
    widths.push_back(4);
    CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // (zero / ones / tw go out of scope)
  }
  const std::size_t ws_bytes = qsx_partition_workspace_bytes(num_tuples, static_cast<int>(P));
  DeviceBuffer ws(ws_bytes + 8), offsets_dev((P + 1) * 8);
  CheckStatus(qsx_partition_scatter(key_type.id, src->stripe(partition_attribute_), num_tuples, static_cast<int>(P), static_cast<int>(cols.size()),
                                    cols.data(), widths.data(), outs.data(), static_cast<std::int64_t *>(offsets_dev.ptr), ws.ptr, ws_bytes,
                                    CurrentStream()), "qsx_partition_scatter");
  std::vector<std::int64_t> offsets(P + 1);
  CheckStatus(qsx_copy_to_host(offsets.data(), offsets_dev.ptr, (P + 1) * 8, CurrentStream()), "qsx_copy_to_host");
  for (std::size_t a = 0; a < relation_->size(); ++a) {
    const Type &t = relation_->getAttributeType(static_cast<attribute_id>(a));
    if (t.width == 1 || t.width == 2 || t.width == 4 || t.width == 8) continue;
    CheckStatus(qsx_gather(t.width, src->stripe(static_cast<attribute_id>(a)), static_cast<const std::int32_t *>(rows_scattered->ptr), num_tuples,
                           scattered->stripe(static_cast<attribute_id>(a)), CurrentStream()), "qsx_gather");
  }
  std::vector<std::pair<block_id, partition_id>> made;
  for (std::size_t p = 0; p < P; ++p) {
    const std::int64_t first = offsets[p], rows_p = offsets[p + 1] - offsets[p];
    if (rows_p == 0) continue;
    const block_id view_id = storage_manager_->createViewBlock(scattered_id, first, rows_p);
    BlockReference view = storage_manager_->getBlock(view_id);
    for (std::size_t a = 0; a < relation_->size(); ++a) {
      std::uint64_t *dst = view->nullBitmap(static_cast<attribute_id>(a));
      if (dst == nullptr) continue;
      const std::uint64_t *bits = src->nullBitmap(static_cast<attribute_id>(a));
      const std::int64_t zero_row = 0;
      CheckStatus(qsx_bitmap_gather_segmented(1, &bits, &zero_row, static_cast<const std::int32_t *>(rows_scattered->ptr) + first, rows_p, dst,
                                              CurrentStream()), "qsx_bitmap_gather_segmented");
    }
    view->setFirstRow(storage_manager_->reserveRows(relation_->getID(), rows_p));
    made.emplace_back(view_id, p);
  }
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // before the source block goes
  storage_manager_->deleteBlockOrBlobFile(id);
  storage_manager_->deleteBlockOrBlobFile(scattered_id);      // (the views keep the scattered block alive)
  {
    std::lock_guard<std::mutex> lock(mutex_);
    for (const auto &m : made) {
      touched_.push_back(TouchedBlock{m.first, m.second});
      relation_->addBlockToPartition(m.first, m.second);
    }
  }
  if (block_returned_ && !made.empty()) block_returned_();
}
std::vector<block_id> InsertDestination::getTouchedBlocks() const {
  std::lock_guard<std::mutex> lock(mutex_);
  std::vector<block_id> ids;
  for (const TouchedBlock &t : touched_) ids.push_back(t.id);
  return ids;
}
std::vector<InsertDestination::TouchedBlock> InsertDestination::getTouchedBlocksWithPartitions() const {
  std::lock_guard<std::mutex> lock(mutex_);
  return touched_;
}
std::vector<InsertDestination::TouchedBlock> InsertDestination::getTouchedBlocksSince(std::size_t from) const {
  std::lock_guard<std::mutex> lock(mutex_);
  if (from >= touched_.size()) return {};
  return std::vector<TouchedBlock>(touched_.begin() + static_cast<std::ptrdiff_t>(from), touched_.end());
}
std::size_t InsertDestination::numTouchedBlocks() const {
  std::lock_guard<std::mutex> lock(mutex_);
  return touched_.size();
}

// ---------------------------------------------------------------------------
// AggregationOperationState
// ---------------------------------------------------------------------------
struct AggregationOperationState::Distinctify {
  std::size_t agg_index = 0;            // position in spec.aggregates
  std::vector<attribute_id> attrs;      // group-by..., argument (kInvalidAttributeID: the argument is `expression`)
  std::vector<Type> types;
  ScalarPtr expression;                 // DISTINCT over an arithmetic expression: evaluated per block into a DOUBLE column
  std::mutex mutex;                     // many AggregationWorkOrders append concurrently
  struct Chunk {
    std::vector<std::unique_ptr<DeviceBuffer>> cols;
    std::int64_t rows = 0;
  };
  std::vector<Chunk> chunks;
};

namespace {
qsx_agg_fn_t AggFn(AggregationID id) {
  switch (id) {
    case AggregationID::kCount: return QSX_AGG_COUNT_STAR;
    case AggregationID::kSum: return QSX_AGG_SUM;
    case AggregationID::kAvg: return QSX_AGG_AVG;
    case AggregationID::kMin: return QSX_AGG_MIN;
    default: return QSX_AGG_MAX;
  }
}
// Result type of an aggregate (AggregationHandle{Count,Sum,Avg,Min,Max}::getResultType).
Type AggResultType(AggregationID id, const Type &argument) {
  switch (id) {
    case AggregationID::kCount: return Type::Long();
    case AggregationID::kSum: return (argument.id == kInt || argument.id == kLong) ? Type::Long() : Type::Double();
    case AggregationID::kAvg: return Type::Double();
    default: return argument;
  }
}
}  // namespace

TypeID ScalarResultType(const ScalarPtr &scalar, const CatalogRelation &relation) {
  if (scalar == nullptr) throw ExecutionError("ScalarResultType: null scalar", QSX_ERR_INVALID_ARGUMENT);
  switch (scalar->kind) {
    case Scalar::kAttribute: {
      const TypeID t = relation.getAttributeType(scalar->attribute).id;
      if (t != kInt && t != kLong && t != kFloat && t != kDouble) {
        throw ExecutionError("arithmetic over a non-numeric attribute", QSX_ERR_UNSUPPORTED);
      }
      return t == kFloat ? kDouble : t;   // (FLOAT operands are evaluated in double)
    }
    case Scalar::kLiteral:
      return scalar->literal_type;
    case Scalar::kCaseExpression: {
      // the unifying type of the branches (Resolver.cpp:2819-2829); a NULL branch has no say
      TypeID unified = kInt;
      bool any = false;
      const auto take = [&](const ScalarPtr &branch) {
        if (branch == nullptr) return;
        const TypeID t = ScalarResultType(branch, relation);
        any = true;
        if (t == kDouble || unified == kDouble) unified = kDouble;
        else if (t == kLong) unified = kLong;
      };
      for (const auto &when : scalar->whens) take(when.second);
      take(scalar->else_result);
      if (!any) throw ExecutionError("CASE: every branch is NULL", QSX_ERR_UNSUPPORTED);
      return unified;
    }
    case Scalar::kUnaryExpression:
      return UnaryResultType(scalar, relation).id;
    default: {
      const TypeID l = ScalarResultType(scalar->left, relation), r = ScalarResultType(scalar->right, relation);
      if (l == kChar || r == kChar) throw ExecutionError("arithmetic over a SUBSTRING", QSX_ERR_UNSUPPORTED);
      if (l == kDouble || r == kDouble) return kDouble;
      return l == kLong || r == kLong ? kLong : kInt;
    }
  }
}

// DateExtractOperation::resultTypeForArgumentType (an INT, nullable as the argument) and SubstringOperation.hpp:174-182.
Type UnaryResultType(const ScalarPtr &scalar, const CatalogRelation &relation) {
  if (scalar == nullptr || scalar->kind != Scalar::kUnaryExpression) throw ExecutionError("UnaryResultType: not a unary expression", QSX_ERR_INVALID_ARGUMENT);
  if (scalar->operand == nullptr || scalar->operand->kind != Scalar::kAttribute) {
    throw ExecutionError("EXTRACT / SUBSTRING: the operand must be an attribute (not a literal, an expression, a CASE or another unary)",
                         QSX_ERR_UNSUPPORTED);
  }
  const Type &t = relation.getAttributeType(scalar->operand->attribute);
  Type result = Type::Int();
  if (scalar->unary_operation == UnaryOperationID::kDateExtract) {
    if (t.id != kDate) throw ExecutionError("EXTRACT: the operand must be a DATE attribute", QSX_ERR_UNSUPPORTED);
    if (scalar->date_extract_unit != QSX_DATE_YEAR && scalar->date_extract_unit != QSX_DATE_MONTH) {
      throw ExecutionError("EXTRACT: a Date has a YEAR and a MONTH (DAY / HOUR / MINUTE / SECOND belong to Datetime)", QSX_ERR_UNSUPPORTED);
    }
  } else {
    if (t.id != kChar) throw ExecutionError("SUBSTRING: the operand must be a CHAR(n) attribute", QSX_ERR_UNSUPPORTED);
    if (scalar->substring_start < 0 || scalar->substring_start >= t.width || scalar->substring_length < 1 || t.width < 1 || t.width > 255) {
      throw ExecutionError("SUBSTRING: 0 <= start < width, length >= 1, width 1..255", QSX_ERR_INVALID_ARGUMENT);
    }
    result = Type::Char(t.width - scalar->substring_start < scalar->substring_length ? t.width - scalar->substring_start : scalar->substring_length);
  }
  result.nullable = t.nullable;
  return result;
}

qsx_operand_t ExpressionFlattener::add(const ScalarPtr &scalar) {
  if (scalar == nullptr) throw ExecutionError("ExpressionFlattener: null scalar", QSX_ERR_INVALID_ARGUMENT);
  switch (scalar->kind) {
    case Scalar::kAttribute:
      return qsx_operand_t{QSX_OPD_COLUMN, column_of_(scalar->attribute)};
    case Scalar::kLiteral: {
      for (std::size_t i = 0; i < consts_.size(); ++i) {
        if (std::memcmp(&consts_[i], &scalar->literal, sizeof(double)) == 0) return qsx_operand_t{QSX_OPD_CONST, static_cast<std::int32_t>(i)};
      }
      if (consts_.size() >= QSX_MAX_CONSTS) throw ExecutionError("expression: too many distinct literals", QSX_ERR_UNSUPPORTED);
      consts_.push_back(scalar->literal);
      return qsx_operand_t{QSX_OPD_CONST, static_cast<std::int32_t>(consts_.size() - 1)};
    }
    case Scalar::kCaseExpression:
      throw ExecutionError("CASE inside an arithmetic expression or inside another CASE's branch: a CASE is the root of a Select "
                           "scalar or of an aggregate's argument", QSX_ERR_UNSUPPORTED);
    case Scalar::kUnaryExpression:
      if (scalar->unary_operation != UnaryOperationID::kDateExtract) throw ExecutionError("SUBSTRING inside an arithmetic expression", QSX_ERR_UNSUPPORTED);
      if (!column_of_unary_) {
        throw ExecutionError("EXTRACT inside a CASE or an aggregate's argument: a unary expression is a Select scalar (or a leaf of its "
                             "arithmetic) or a group-by key", QSX_ERR_UNSUPPORTED);
      }
      return qsx_operand_t{QSX_OPD_COLUMN, column_of_unary_(scalar)};
    default: {
      const qsx_operand_t a = add(scalar->left), b = add(scalar->right);
      std::int32_t op = static_cast<std::int32_t>(scalar->operation);   // kAdd .. kDivide = QSX_EX_ADD .. QSX_EX_DIV
      if (integer_relation_ != nullptr && ScalarResultType(scalar, *integer_relation_) != kDouble) op += QSX_EX_IADD;   // .. IDIV
      for (const qsx_expr_instr_t &in : instrs_) {   // the same node again (shared subexpression): its temp
        if (in.op == op && in.a.kind == a.kind && in.a.index == a.index && in.b.kind == b.kind && in.b.index == b.index) {
          return qsx_operand_t{QSX_OPD_TEMP, in.dst};
        }
      }
      if (instrs_.size() >= QSX_MAX_INSTRS || instrs_.size() >= QSX_MAX_TEMPS) {
        throw ExecutionError("expression: more nodes than the kernel's program holds", QSX_ERR_UNSUPPORTED);
      }
      qsx_expr_instr_t in;
      in.op = op;
      in.dst = static_cast<std::int32_t>(instrs_.size());   // one temp per node
      in.a = a;
      in.b = b;
      instrs_.push_back(in);
      return qsx_operand_t{QSX_OPD_TEMP, in.dst};
    }
  }
}

// ---------------------------------------------------------------------------
// searched CASE (ScalarCaseExpression::getAllValues, expressions/scalar/ScalarCaseExpression.cpp:273-350)
// ---------------------------------------------------------------------------
CaseEvaluator::CaseEvaluator(const ScalarPtr &s, const CatalogRelation &relation, bool integer_arithmetic) : scalar(s) {
  if (s == nullptr || s->kind != Scalar::kCaseExpression) throw ExecutionError("CaseEvaluator: not a CASE", QSX_ERR_INVALID_ARGUMENT);
  if (s->whens.empty() || s->whens.size() > QSX_MAX_CASE_WHENS) {
    throw ExecutionError("CASE: 1 .. QSX_MAX_CASE_WHENS WHEN clauses", QSX_ERR_UNSUPPORTED);
  }
  std::memset(&desc, 0, sizeof(desc));
  ExpressionFlattener flattener([&](attribute_id a) {
    for (std::size_t c = 0; c < attrs.size(); ++c) if (attrs[c] == a) return static_cast<int>(c);
    attrs.push_back(a);
    return static_cast<int>(attrs.size() - 1);
  }, integer_arithmetic ? &relation : nullptr);
  const TypeID unified = ScalarResultType(s, relation);   // (throws QSX_ERR_UNSUPPORTED on a CHAR / DATE branch)
  out_type = integer_arithmetic ? unified : kDouble;
  desc.num_whens = static_cast<std::int32_t>(s->whens.size());
  desc.out_type = out_type;
  const auto branch = [&](const ScalarPtr &value) {
    if (value == nullptr) {
      has_null_branch = true;
      return qsx_operand_t{QSX_OPD_NULL, 0};
    }
    if (value->kind == Scalar::kCaseExpression) throw ExecutionError("CASE nested in a branch of a CASE", QSX_ERR_UNSUPPORTED);
    return flattener.add(value);
  };
  for (std::size_t k = 0; k < s->whens.size(); ++k) {
    std::vector<const ComparisonPredicate *> when_terms;
    for (const ComparisonPredicate &term : s->whens[k].first.conjuncts) when_terms.push_back(&term);
    if (s->whens[k].first.tree != nullptr) CollectLeafTerms(*s->whens[k].first.tree, &when_terms);
    for (const ComparisonPredicate *term : when_terms) {
      if (term->operand != nullptr) {
        CheckUnaryTerm(*term, relation);   // (the literals' types are checked where the WHEN is evaluated)
        continue;
      }
      if (IsLikeComparison(term->comparison)) CheckLikeTerm(*term, relation.getAttributeType(term->attribute));
      if (term->rhs_attribute != kInvalidAttributeID) CheckAttributeComparison(*term, relation);
    }
    desc.value[k] = branch(s->whens[k].second);
  }
  desc.value[s->whens.size()] = branch(s->else_result);
  if (attrs.size() > QSX_MAX_COLUMNS) throw ExecutionError("CASE over too many attributes", QSX_ERR_UNSUPPORTED);
  instrs = flattener.instrs();
  for (std::size_t c = 0; c < flattener.consts().size(); ++c) consts[c] = flattener.consts()[c];
  nullable = has_null_branch;
  for (attribute_id a : attrs) {
    types.push_back(relation.getAttributeType(a).id);
    nullable = nullable || relation.getAttributeType(a).nullable;
  }
}

void CaseEvaluator::evalBlock(const StorageBlock &block, void *out_dev, std::uint64_t *out_nulls_dev) const {
  const std::int64_t n = block.numTuples();
  if (n == 0) return;
  struct Owned {
    std::vector<void *> ptrs;
    ~Owned() { for (void *p : ptrs) qsx_device_free(p); }
  } when_bitmaps;
  const std::uint64_t *whens[QSX_MAX_CASE_WHENS] = {};
  for (std::size_t k = 0; k < scalar->whens.size(); ++k) {
    std::int64_t matches = 0;   // the predicate over the WHOLE block: the kernel gives the first match the row
    when_bitmaps.ptrs.push_back(scalar->whens[k].first.getMatchesForBlock(block, &matches, nullptr));
    whens[k] = static_cast<const std::uint64_t *>(when_bitmaps.ptrs.back());
  }
  const void *cols[QSX_MAX_COLUMNS] = {};
  const std::uint64_t *col_nulls[QSX_MAX_COLUMNS] = {};
  for (std::size_t c = 0; c < attrs.size(); ++c) {
    cols[c] = block.stripe(attrs[c]);
    col_nulls[c] = block.nullBitmap(attrs[c]);
  }
  if (nullable && out_nulls_dev == nullptr) throw ExecutionError("CASE that can yield NULL needs a null bitmap", QSX_ERR_INVALID_ARGUMENT);
  CheckStatus(qsx_eval_case(static_cast<int>(attrs.size()), cols, types.data(), nullable ? col_nulls : nullptr, static_cast<int>(instrs.size()),
                            instrs.data(), consts, &desc, whens, n, out_dev, nullable ? out_nulls_dev : nullptr, CurrentStream()),
              "qsx_eval_case");
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // (the WHEN bitmaps go back)
}

bool CaseEvaluator::evalBlocks(const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows, void *const *outs,
                               std::vector<std::unique_ptr<RunMatches>> *keep) const {
  if (nullable || blocks.empty()) return false;
  for (const auto &when : scalar->whens) {
    if (when.first.empty() || !RunPredicateCovers(when.first, blocks)) return false;
  }
  for (const BlockReference &b : blocks) {
    for (attribute_id a : attrs) if (b->nullBitmap(a) != nullptr) return false;
  }
  const std::size_t nb = blocks.size(), nw = scalar->whens.size();
  std::vector<const std::uint64_t *> when_bitmaps(nb * nw);
  for (std::size_t k = 0; k < nw; ++k) {
    keep->emplace_back(new RunMatches);
    RunPredicateMatches(scalar->whens[k].first, blocks, rows, nullptr, keep->back().get());
    for (std::size_t b = 0; b < nb; ++b) when_bitmaps[b * nw + k] = keep->back()->bitmaps[b];
  }
  std::vector<const void *> cols(nb * attrs.size());
  for (std::size_t b = 0; b < nb; ++b) {
    for (std::size_t c = 0; c < attrs.size(); ++c) cols[b * attrs.size() + c] = blocks[b]->stripe(attrs[c]);
  }
  CheckStatus(qsx_eval_case_blocks(static_cast<int>(attrs.size()), types.data(), static_cast<int>(instrs.size()), instrs.data(), consts, &desc,
                                   static_cast<std::int64_t>(nb), rows.data(), cols.data(), nullptr, when_bitmaps.data(), outs, nullptr,
                                   CurrentStream()), "qsx_eval_case_blocks");
  return true;
}

// ---------------------------------------------------------------------------
// unary operations (types/operations/unary_operations/DateExtractOperation.cpp, SubstringOperation.cpp)
// ---------------------------------------------------------------------------
UnaryEvaluator::UnaryEvaluator(const ScalarPtr &s, const CatalogRelation &relation) : scalar(s) {
  result = UnaryResultType(s, relation);   // (checks the operand and the window)
  operand = s->operand->attribute;
  operand_type = relation.getAttributeType(operand);
}

bool UnaryEvaluator::extractsOnCodes(const StorageBlock &block) const {
  if (scalar->unary_operation != UnaryOperationID::kDateExtract) return false;
  const CompressedAttribute *ca = block.compressedAttribute(operand);
  return ca != nullptr && ca->kind == CompressedAttribute::kDictionary && !block.valuesMaterialized(operand) && ca->num_codes > 0 &&
         (reinterpret_cast<std::uintptr_t>(ca->dictionary) & 7) == 0;   // (a dictionary inside an adopted image may lie anywhere)
}

bool UnaryEvaluator::evalBlock(const StorageBlock &block, void *out_dev, Scratch *keep) const {
  const std::int64_t n = block.numTuples();
  if (n == 0) return false;
  if (scalar->unary_operation == UnaryOperationID::kSubstring) {
    CheckStatus(qsx_eval_substring(block.stripe(operand), operand_type.width, n, scalar->substring_start, scalar->substring_length, out_dev,
                                   CurrentStream()), "qsx_eval_substring");
    return false;
  }
  if (!extractsOnCodes(block)) {
    CheckStatus(qsx_eval_date_extract(scalar->date_extract_unit, block.stripe(operand), n, static_cast<std::int32_t *>(out_dev), CurrentStream()),
                "qsx_eval_date_extract");
    return false;
  }
  const CompressedAttribute *ca = block.compressedAttribute(operand);
  const std::size_t codes = static_cast<std::size_t>(ca->num_codes);
  keep->emplace_back(new DeviceBuffer((codes + 1) * 4 + 16));
  std::int32_t *fields = static_cast<std::int32_t *>(keep->back()->ptr);
  CheckStatus(qsx_eval_date_extract(scalar->date_extract_unit, ca->dictionary, ca->num_codes, fields, CurrentStream()), "qsx_eval_date_extract(dictionary)");
  CheckStatus(qsx_memset_device(fields + codes, 0, 4, CurrentStream()), "qsx_memset_device");   // the NULL code's entry
  CheckStatus(qsx_decode_codes(ca->code_width, ca->codes, n, fields, 4, out_dev, CurrentStream()), "qsx_decode_codes(extract)");
  return true;
}

std::int64_t UnaryEvaluator::evalBlocks(const std::vector<BlockReference> &blocks, const std::vector<std::int64_t> &rows, void *const *outs,
                                        Scratch *keep) const {
  std::int64_t on_codes = 0;
  std::vector<std::int64_t> run_rows;
  std::vector<const void *> run_cols;
  std::vector<void *> run_outs;
  for (std::size_t b = 0; b < blocks.size(); ++b) {
    if (rows[b] == 0) continue;
    if (extractsOnCodes(*blocks[b])) {
      on_codes += evalBlock(*blocks[b], outs[b], keep) ? 1 : 0;
      continue;
    }
    run_rows.push_back(rows[b]);
    run_cols.push_back(blocks[b]->stripe(operand));
    run_outs.push_back(outs[b]);
  }
  if (run_rows.empty()) return on_codes;
  if (scalar->unary_operation == UnaryOperationID::kSubstring) {
    CheckStatus(qsx_eval_substring_blocks(operand_type.width, static_cast<std::int64_t>(run_rows.size()), run_rows.data(), run_cols.data(),
                                          scalar->substring_start, scalar->substring_length, run_outs.data(), CurrentStream()),
                "qsx_eval_substring_blocks");
  } else {
    CheckStatus(qsx_eval_date_extract_blocks(scalar->date_extract_unit, static_cast<std::int64_t>(run_rows.size()), run_rows.data(), run_cols.data(),
                                             reinterpret_cast<std::int32_t *const *>(run_outs.data()), CurrentStream()),
                "qsx_eval_date_extract_blocks");
  }
  return on_codes;
}

struct AggregationOperationState::UnaryColumn {
  int column;
  UnaryEvaluator evaluator;
  UnaryColumn(int c, const ScalarPtr &s, const CatalogRelation &rel) : column(c), evaluator(s, rel) {}
};

struct AggregationOperationState::CaseColumn {
  int column;
  CaseEvaluator evaluator;
  CaseColumn(int c, const ScalarPtr &s, const CatalogRelation &rel, bool integer) : column(c), evaluator(s, rel, integer) {}
};

AggregationOperationState::AggregationOperationState(const AggregationStateSpec &given) : spec_(given) {
  // group_by_scalars replaces group_by; a list of attributes only is the plain form
  if (!spec_.group_by_scalars.empty()) {
    bool attributes_only = true;
    for (const ScalarPtr &key : spec_.group_by_scalars) {
      if (key == nullptr || (key->kind != Scalar::kAttribute && key->kind != Scalar::kUnaryExpression)) {
        throw ExecutionError("AggregationOperationState: a group-by key is an attribute or a unary expression over one", QSX_ERR_UNSUPPORTED);
      }
      attributes_only = attributes_only && key->kind == Scalar::kAttribute;
    }
    spec_.group_by.clear();
    if (attributes_only) {
      for (const ScalarPtr &key : spec_.group_by_scalars) spec_.group_by.push_back(key->attribute);
      spec_.group_by_scalars.clear();
    }
  }
  const AggregationStateSpec &spec = spec_;
  // the library must have been built from the header this file was compiled against
  if (qsx_abi_version() != QSX_ABI_VERSION || qsx_abi_sizeof_agg_config() != sizeof(qsx_agg_config_t)) {
    throw ExecutionError("libqsx.so and include/qsx.h disagree on the ABI version / qsx_agg_config_t", QSX_ERR_INVALID_ARGUMENT);
  }
  std::memset(&config_, 0, sizeof(config_));
  const CatalogRelation &rel = *spec.input_relation;
  auto column_of = [&](attribute_id attr) -> int {
    for (std::size_t i = 0; i < column_attr_.size(); ++i) {
      if (column_attr_[i] == attr) return static_cast<int>(i);
    }
    if (column_attr_.size() >= QSX_MAX_COLUMNS) throw ExecutionError("AggregationOperationState: too many columns", QSX_ERR_UNSUPPORTED);
    const Type &t = rel.getAttributeType(attr);
    config_.column_type[column_attr_.size()] = t.id;
    config_.column_width[column_attr_.size()] = t.width;
    config_.column_nullable[column_attr_.size()] = t.nullable ? 1 : 0;
    column_attr_.push_back(attr);
    return static_cast<int>(column_attr_.size() - 1);
  };
  // the group-by keys: attributes, or (group_by_scalars) attributes and unary expressions, each of the latter a derived column
  const std::size_t num_keys = spec.group_by_scalars.empty() ? spec.group_by.size() : spec.group_by_scalars.size();
  if (num_keys > QSX_MAX_KEYS) throw ExecutionError("AggregationOperationState: too many group-by keys", QSX_ERR_UNSUPPORTED);
  std::vector<Type> key_types;               // a unary key: its result type
  std::vector<attribute_id> key_attributes;  // ... and its operand attribute
  config_.strategy = num_keys == 0 ? QSX_AGG_SINGLE_STATE : spec.strategy;
  config_.num_keys = static_cast<int>(num_keys);
  for (std::size_t k = 0; k < num_keys; ++k) {
    const ScalarPtr unary = !spec.group_by_scalars.empty() && spec.group_by_scalars[k]->kind == Scalar::kUnaryExpression ? spec.group_by_scalars[k] : nullptr;
    if (unary == nullptr) {
      const attribute_id attr = spec.group_by_scalars.empty() ? spec.group_by[k] : spec.group_by_scalars[k]->attribute;
      config_.key_column[k] = column_of(attr);
      key_types.push_back(rel.getAttributeType(attr));
      key_attributes.push_back(attr);
      continue;
    }
    if (column_attr_.size() >= QSX_MAX_COLUMNS) throw ExecutionError("AggregationOperationState: too many columns", QSX_ERR_UNSUPPORTED);
    const int column = static_cast<int>(column_attr_.size());
    unary_columns_.emplace_back(new UnaryColumn(column, unary, rel));
    const UnaryEvaluator &ev = unary_columns_.back()->evaluator;
    config_.column_type[column] = ev.result.id;
    config_.column_width[column] = ev.result.width;
    config_.column_nullable[column] = ev.result.nullable ? 1 : 0;
    column_attr_.push_back(kInvalidAttributeID);
    config_.key_column[k] = column;
    key_types.push_back(ev.result);
    key_attributes.push_back(ev.operand);
  }
  // GROUP BY CHAR(n): the widths the state packs itself (1, 2, 4, 8 bytes under COMPACT_KEY) keep their path; every other
  // CHAR group-by attribute is presented as an INT column of ids out of a device dictionary of its values
  for (std::size_t k = 0; k < num_keys; ++k) {
    const Type &t = key_types[k];
    // (a VARCHAR(n) key is always interned: its stripe — decoded from the block's variable-length dictionary — holds CHAR(n) fields)
    const bool packs = t.id == kChar && (t.width == 1 || t.width == 2 || t.width == 4 || t.width == 8);
    if (!IsTextType(t.id) || (packs && config_.strategy != QSX_AGG_GENERIC) || internedKeyOf(config_.key_column[k]) >= 0) continue;
    if (t.id == kVarChar && (t.width < 1 || t.width > QSX_MAX_CHAR_DICT_WIDTH)) {
      throw ExecutionError("GROUP BY VARCHAR(n): n outside 1..QSX_MAX_CHAR_DICT_WIDTH", QSX_ERR_UNSUPPORTED);
    }
    InternedKey key;
    key.column = config_.key_column[k];
    key.attribute = key_attributes[k];
    key.derived = column_attr_[static_cast<std::size_t>(key.column)] == kInvalidAttributeID;
    key.width = t.width;
    key.capacity = spec.estimated_num_groups > 16 ? spec.estimated_num_groups : 16;
    if (key.capacity > (std::int64_t(1) << 30)) key.capacity = std::int64_t(1) << 30;
    interned_.push_back(key);
    config_.column_type[key.column] = kInt;
    config_.column_width[key.column] = 4;
  }
  int num_main = 0;
  ExpressionFlattener flattener(column_of, spec.integer_argument_arithmetic ? &rel : nullptr);
  for (std::size_t a = 0; a < spec_.aggregates.size(); ++a) {
    if (spec_.aggregates[a].argument_expression != nullptr && spec_.aggregates[a].argument_expression->kind == Scalar::kAttribute) {
      spec_.aggregates[a].argument = spec_.aggregates[a].argument_expression->attribute;   // ScalarAttribute: the plain form
      spec_.aggregates[a].argument_expression = nullptr;
    }
    const AggregateSpec &ag = spec_.aggregates[a];
    if (ag.argument_expression == nullptr && ag.argument != kInvalidAttributeID && rel.getAttributeType(ag.argument).id == kVarChar) {
      throw ExecutionError("a VARCHAR attribute as an aggregate's argument", QSX_ERR_UNSUPPORTED);
    }
    if (ag.is_distinct && !unary_columns_.empty()) {   // (the distinctify tables are keyed by group-by ATTRIBUTES)
      throw ExecutionError("DISTINCT aggregate beside a unary group-by key", QSX_ERR_UNSUPPORTED);
    }
    if (ag.argument_expression != nullptr && ag.argument_expression->kind == Scalar::kUnaryExpression) {
      throw ExecutionError("a unary expression as an aggregate's argument: project it with a Select first", QSX_ERR_UNSUPPORTED);
    }
    if (ag.is_distinct && !interned_.empty()) {   // (finalizeWithDistinct lines its result sets up by sorting on key VALUES)
      throw ExecutionError("DISTINCT aggregate beside a CHAR(n) group-by key that is interned into ids", QSX_ERR_UNSUPPORTED);
    }
    if (ag.argument_expression != nullptr && ag.argument_expression->kind == Scalar::kCaseExpression) {
      // a CASE argument: a derived column of the state (quickstep_gpu.hpp case_columns_)
      if (ag.is_distinct) throw ExecutionError("DISTINCT aggregate over a CASE", QSX_ERR_UNSUPPORTED);
      if (column_attr_.size() >= QSX_MAX_COLUMNS) throw ExecutionError("AggregationOperationState: too many columns", QSX_ERR_UNSUPPORTED);
      const int column = static_cast<int>(column_attr_.size());
      case_columns_.emplace_back(new CaseColumn(column, ag.argument_expression, rel, spec.integer_argument_arithmetic));
      const CaseEvaluator &ev = case_columns_.back()->evaluator;
      config_.column_type[column] = ev.out_type;
      config_.column_width[column] = ev.width();
      config_.column_nullable[column] = ev.nullable ? 1 : 0;
      column_attr_.push_back(kInvalidAttributeID);
      // COUNT(CASE ..) counts the rows whose value is not NULL; over a CASE that cannot be NULL it is COUNT(*)
      config_.aggs[num_main].fn = ag.function == AggregationID::kCount ? (ev.nullable ? QSX_AGG_COUNT : QSX_AGG_COUNT_STAR) : AggFn(ag.function);
      config_.aggs[num_main].arg.kind = QSX_OPD_COLUMN;
      config_.aggs[num_main].arg.index = column;
      main_agg_.push_back(num_main++);
      continue;
    }
    if (ag.argument_expression != nullptr && ag.is_distinct) {
      // DISTINCT over an arithmetic expression (Distinct.test:58-72 COUNT(DISTINCT x % y) is such a query): the distinctify
      // key is (group-by..., value of the expression); the value column is computed per block (qsx_eval_expression)
      if (spec.group_by.size() + 1 > QSX_MAX_KEYS) throw ExecutionError("DISTINCT aggregate: too many group-by attributes", QSX_ERR_UNSUPPORTED);
      std::unique_ptr<Distinctify> d(new Distinctify);
      d->agg_index = a;
      d->attrs = spec.group_by;
      d->attrs.push_back(kInvalidAttributeID);
      for (attribute_id attr : spec.group_by) d->types.push_back(rel.getAttributeType(attr));
      d->types.push_back(Type::Double());
      d->expression = ag.argument_expression;
      distinctify_.push_back(std::move(d));
      main_agg_.push_back(-1);
      continue;
    }
    if (ag.argument_expression != nullptr) {
      // an arithmetic expression as the aggregate's argument: part of the state's expression program
      if (ag.function == AggregationID::kCount) throw ExecutionError("COUNT over an expression: pass COUNT(*)", QSX_ERR_UNSUPPORTED);
      const qsx_operand_t value = flattener.add(ag.argument_expression);
      if (value.kind == QSX_OPD_CONST) throw ExecutionError("aggregate over a literal", QSX_ERR_UNSUPPORTED);
      config_.aggs[num_main].fn = AggFn(ag.function);
      config_.aggs[num_main].arg = value;
      main_agg_.push_back(num_main++);
      continue;
    }
    if (ag.is_distinct) {
      // "Initialize the corresponding distinctify hash table if this is a DISTINCT aggregation" (:172-207):
      // key types = group-by types + argument types
      if (ag.argument == kInvalidAttributeID) throw ExecutionError("DISTINCT aggregate without an argument", QSX_ERR_INVALID_ARGUMENT);
      if (spec.group_by.size() + 1 > QSX_MAX_KEYS) throw ExecutionError("DISTINCT aggregate: too many group-by attributes", QSX_ERR_UNSUPPORTED);
      std::unique_ptr<Distinctify> d(new Distinctify);
      d->agg_index = a;
      d->attrs = spec.group_by;
      d->attrs.push_back(ag.argument);
      for (attribute_id attr : d->attrs) d->types.push_back(rel.getAttributeType(attr));
      distinctify_.push_back(std::move(d));
      main_agg_.push_back(-1);
      continue;
    }
    config_.aggs[num_main].fn = AggFn(ag.function);
    if (ag.function != AggregationID::kCount) {
      config_.aggs[num_main].arg.kind = QSX_OPD_COLUMN;
      config_.aggs[num_main].arg.index = column_of(ag.argument);
    } else if (ag.argument != kInvalidAttributeID && rel.getAttributeType(ag.argument).nullable) {
      // COUNT(x) over a nullable x counts the non-NULL values (AggregationHandleCount<false, true>); over a
      // non-nullable x it is COUNT(*)
      config_.aggs[num_main].fn = QSX_AGG_COUNT;
      config_.aggs[num_main].arg.kind = QSX_OPD_COLUMN;
      config_.aggs[num_main].arg.index = column_of(ag.argument);
    }
    main_agg_.push_back(num_main++);
  }
  config_.num_aggs = num_main;
  config_.num_instrs = static_cast<int>(flattener.instrs().size());
  for (std::size_t k = 0; k < flattener.instrs().size(); ++k) config_.instrs[k] = flattener.instrs()[k];
  for (std::size_t k = 0; k < flattener.consts().size(); ++k) config_.consts[k] = flattener.consts()[k];
  if (spec.predicate != nullptr) {
    // (what the struct cannot hold — CHAR(n) terms, a tree — goes to external_predicate_: evaluated block by block by Predicate)
    LowerPredicateToAggConfig(*spec.predicate, rel, [&](attribute_id a) { return column_of(a); }, &config_, &external_predicate_);
  }
  config_.num_columns = static_cast<int>(column_attr_.size());
  config_.est_groups = spec.estimated_num_groups;
  config_.num_entries = spec.collision_free_num_entries;
  // all_distinct_ (:126-127, 620-628): no upsert into the final table per block, it is filled from the distinctify tables
  if (num_main > 0 || distinctify_.empty()) CheckStatus(qsx_agg_state_create(&config_, &state_), "qsx_agg_state_create");
  try {
    for (InternedKey &key : interned_) CheckStatus(qsx_char_dict_create(key.width, key.capacity, &key.dictionary), "qsx_char_dict_create");
  } catch (...) {
    for (InternedKey &key : interned_) if (key.dictionary != nullptr) qsx_char_dict_destroy(key.dictionary);
    if (state_ != nullptr) qsx_agg_state_destroy(state_);
    throw;
  }
}

AggregationOperationState::~AggregationOperationState() {
  if (state_ != nullptr) qsx_agg_state_destroy(state_);
  if (coded_state_ != nullptr) qsx_agg_state_destroy(coded_state_);
  for (InternedKey &key : interned_) if (key.dictionary != nullptr) qsx_char_dict_destroy(key.dictionary);
}

int AggregationOperationState::internedKeyOf(std::size_t column) const {
  for (std::size_t i = 0; i < interned_.size(); ++i) {
    if (static_cast<std::size_t>(interned_[i].column) == column) return static_cast<int>(i);
  }
  return -1;
}

struct AggregationOperationState::InternScratch {
  std::vector<std::unique_ptr<DeviceBuffer>> buffers;
  void *take(std::size_t bytes) {
    buffers.emplace_back(new DeviceBuffer(bytes + 16));
    return buffers.back()->ptr;
  }
};

// The id stripes of the interned keys for the rows of `requests` (a block, or the blocks of a run), ready when this returns.
//   a plain stripe             qsx_char_dict_intern / _intern_blocks under the request's filter, NULL rows kept out of it
//                              (PackedPayloadHashTable.hpp:861-867 skips a tuple with a NULL key; their id is -1 and the
//                              attribute's null bitmap, which travels with the id column, keeps them out of the state)
//   a dictionary-coded stripe  the block's DICTIONARY is interned (num_codes values) and the code stripe mapped through the
//                              resulting id array (qsx_decode_codes): the values are never decoded, as with LIKE on codes
// An intern is stream-ordered and cannot fail for lack of room: it drops rows instead.  So the dictionary's counters are read
// behind it (one synchronisation); on a drop the dictionary is enlarged at least fourfold and the interns are repeated — ids
// that were handed out stay — before any of them reaches the state.  One block or run at a time per state: `dropped` belongs
// to the dictionary, not to a call.
void AggregationOperationState::internBlocks(std::vector<InternRequest> *requests, InternScratch *scratch) {
  if (interned_.empty() || requests->empty()) return;
  std::vector<std::unique_ptr<DeviceBuffer>> not_null;   // the intern filters of nullable keys
  for (InternRequest &r : *requests) r.ids.assign(interned_.size(), nullptr);
  std::lock_guard<std::mutex> lock(intern_mutex_);
  for (std::size_t k = 0; k < interned_.size(); ++k) {
    InternedKey &key = interned_[k];
    std::vector<std::int64_t> rows;
    std::vector<const void *> cols;
    std::vector<const std::uint64_t *> filters;
    std::vector<std::int32_t *> outs;
    struct Coded { const CompressedAttribute *attribute; std::int64_t n; std::int32_t *code_ids, *out; };
    std::vector<Coded> coded;
    for (InternRequest &r : *requests) {
      const std::int64_t n = r.block->numTuples();
      std::int32_t *ids = static_cast<std::int32_t *>(scratch->take(static_cast<std::size_t>(n) * 4));
      r.ids[k] = ids;
      if (n == 0) continue;
      const CompressedAttribute *ca = key.derived ? nullptr : r.block->compressedAttribute(key.attribute);
      // (a variable-length dictionary — a VARCHAR key — is no stripe of fixed fields: its block presents the decoded stripe)
      if (!key.derived && ca != nullptr && ca->kind == CompressedAttribute::kDictionary && !ca->variable_length &&
          !r.block->valuesMaterialized(key.attribute)) {
        // (one more entry than codes: the dictionary's NULL code, num_codes, maps to -1)
        coded.push_back(Coded{ca, n, static_cast<std::int32_t *>(scratch->take((static_cast<std::size_t>(ca->num_codes) + 1) * 4)), ids});
        continue;
      }
      const std::uint64_t *filter = r.filter;
      if (r.block->nullBitmap(key.attribute) != nullptr) {
        std::unique_ptr<DeviceBuffer> keep = NotNullFilter(*r.block, {key.attribute}, r.filter);
        if (keep != nullptr) {
          filter = static_cast<const std::uint64_t *>(keep->ptr);
          not_null.push_back(std::move(keep));
        }
      }
      rows.push_back(n);
      cols.push_back(key.derived ? r.derived.at(static_cast<std::size_t>(key.column)) : r.block->stripe(key.attribute));
      filters.push_back(filter);
      outs.push_back(ids);
    }
    for (;;) {
      if (rows.size() == 1) {
        CheckStatus(qsx_char_dict_intern(key.dictionary, cols[0], rows[0], filters[0], outs[0], CurrentStream()), "qsx_char_dict_intern");
      } else if (!rows.empty()) {
        CheckStatus(qsx_char_dict_intern_blocks(key.dictionary, static_cast<std::int64_t>(rows.size()), rows.data(), cols.data(), filters.data(),
                                                outs.data(), CurrentStream()), "qsx_char_dict_intern_blocks");
      }
      for (const Coded &c : coded) {
        CheckStatus(qsx_char_dict_intern(key.dictionary, c.attribute->dictionary, c.attribute->num_codes, nullptr, c.code_ids, CurrentStream()),
                    "qsx_char_dict_intern(dictionary)");
        CheckStatus(qsx_memset_device(c.code_ids + c.attribute->num_codes, 0xFF, 4, CurrentStream()), "qsx_memset_device");
      }
      std::int64_t values = 0, dropped = 0;
      CheckStatus(qsx_char_dict_size(key.dictionary, &values, &dropped, CurrentStream()), "qsx_char_dict_size");
      if (dropped == 0) break;
      if (key.capacity >= (std::int64_t(1) << 30)) throw ExecutionError("GROUP BY CHAR(n): more than 2^30 distinct values", QSX_ERR_TOO_MANY_GROUPS);
      key.capacity = key.capacity * 4 < (std::int64_t(1) << 30) ? key.capacity * 4 : (std::int64_t(1) << 30);
      CheckStatus(qsx_char_dict_reserve(key.dictionary, key.capacity, CurrentStream()), "qsx_char_dict_reserve");
    }
    for (const Coded &c : coded) {
      CheckStatus(qsx_decode_codes(c.attribute->code_width, c.attribute->codes, c.n, c.code_ids, 4, c.out, CurrentStream()), "qsx_decode_codes(ids)");
    }
  }
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // (the filters in not_null go back to the pool)
}

void AggregationOperationState::initialize(std::size_t state_partition_id) {
  if (config_.strategy != QSX_AGG_COLLISION_FREE) {
    throw ExecutionError("AggregationOperationState::initialize() is not supported by this aggregation", QSX_ERR_UNSUPPORTED);
  }
  if (state_partition_id != 0) return;   // (the fill of slice 0 covers the whole allocation)
  if (state_ != nullptr) CheckStatus(qsx_agg_state_clear(state_, CurrentStream()), "qsx_agg_state_clear");
  if (coded_state_ != nullptr) CheckStatus(qsx_agg_state_clear(coded_state_, CurrentStream()), "qsx_agg_state_clear");
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // the aggregation runs on other streams
}

void AggregationOperationState::aggregateBlock(const StorageBlock &block, const std::uint64_t *lip_filter) {
  const std::int64_t n = block.numTuples();
  if (!distinctify_.empty() && n > 0) {
    // insertValueAccessorIntoDistinctifyHashTable per DISTINCT aggregate (:522-528, 600-628), on the tuples that pass
    // the state's predicate and the LIP filters: the block's distinct (group-by..., argument) tuples are appended
    std::int64_t matches = n;
    void *selected = nullptr;
    if (spec_.predicate != nullptr) selected = spec_.predicate->getMatchesForBlock(block, &matches, lip_filter);
    const std::uint64_t *filter = selected != nullptr ? static_cast<const std::uint64_t *>(selected) : lip_filter;
    const std::size_t ws_bytes = qsx_sort_workspace_bytes(n);
    DeviceBuffer ws(ws_bytes), tids(static_cast<std::size_t>(n) * 4 + 16), count(8);
    for (auto &d : distinctify_) {
      const void *cols[QSX_MAX_KEYS];
      std::int32_t types[QSX_MAX_KEYS];
      std::unique_ptr<DeviceBuffer> expression_values;
      std::vector<attribute_id> nullable_sources;   // attributes whose NULLs keep a tuple out of the table
      for (std::size_t c = 0; c < d->attrs.size(); ++c) {
        types[c] = d->types[c].id;
        if (d->attrs[c] != kInvalidAttributeID) {
          cols[c] = block.stripe(d->attrs[c]);
          nullable_sources.push_back(d->attrs[c]);
          continue;
        }
        std::vector<attribute_id> attrs;
        ExpressionFlattener flattener([&](attribute_id a) {
          for (std::size_t k = 0; k < attrs.size(); ++k) if (attrs[k] == a) return static_cast<int>(k);
          attrs.push_back(a);
          return static_cast<int>(attrs.size() - 1);
        });
        const qsx_operand_t result = flattener.add(d->expression);
        const void *in_cols[QSX_MAX_COLUMNS];
        std::int32_t in_types[QSX_MAX_COLUMNS];
        if (attrs.size() > QSX_MAX_COLUMNS) throw ExecutionError("DISTINCT: expression over too many attributes", QSX_ERR_UNSUPPORTED);
        for (std::size_t k = 0; k < attrs.size(); ++k) {
          in_cols[k] = block.stripe(attrs[k]);
          in_types[k] = block.getRelation().getAttributeType(attrs[k]).id;
          nullable_sources.push_back(attrs[k]);   // a NULL operand makes the value NULL
        }
        double consts[QSX_MAX_CONSTS] = {};
        for (std::size_t k = 0; k < flattener.consts().size(); ++k) consts[k] = flattener.consts()[k];
        expression_values.reset(new DeviceBuffer(static_cast<std::size_t>(n) * 8 + 8));
        CheckStatus(qsx_eval_expression(static_cast<int>(attrs.size()), in_cols, in_types, static_cast<int>(flattener.instrs().size()),
                                        flattener.instrs().data(), consts, result, n, static_cast<double *>(expression_values->ptr),
                                        CurrentStream()), "qsx_eval_expression");
        cols[c] = expression_values->ptr;
      }
      // the distinctify table is keyed by (group-by..., argument): a tuple with a NULL in any of them is not inserted
      // (PackedPayloadHashTable.hpp:861-867)
      const std::unique_ptr<DeviceBuffer> not_null = NotNullFilter(block, nullable_sources, filter);
      const std::uint64_t *distinct_filter = not_null != nullptr ? static_cast<const std::uint64_t *>(not_null->ptr) : filter;
      CheckStatus(qsx_distinct_rows(static_cast<int>(d->attrs.size()), cols, types, n, distinct_filter, static_cast<std::int32_t *>(tids.ptr),
                                    static_cast<std::int64_t *>(count.ptr), ws.ptr, ws_bytes, CurrentStream()), "qsx_distinct_rows");
      Distinctify::Chunk chunk;
      chunk.rows = ReadCount(count.ptr);
      if (chunk.rows == 0) continue;
      for (std::size_t c = 0; c < d->attrs.size(); ++c) {
        chunk.cols.emplace_back(new DeviceBuffer(static_cast<std::size_t>(chunk.rows) * d->types[c].width + 16));
        CheckStatus(qsx_gather(d->types[c].width, cols[c], static_cast<const std::int32_t *>(tids.ptr), chunk.rows,
                               chunk.cols.back()->ptr, CurrentStream()), "qsx_gather");
      }
      CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
      std::lock_guard<std::mutex> lock(d->mutex);
      d->chunks.push_back(std::move(chunk));
    }
    qsx_device_free(selected);
  }
  if (state_ == nullptr) return;
  // the conjuncts the kernel does not evaluate: a TupleIdSequence like the one a SelectOperator computes, used as the filter
  struct OwnedBitmap {
    void *ptr = nullptr;
    ~OwnedBitmap() { if (ptr != nullptr) qsx_device_free(ptr); }
  } external_matches;
  if (!external_predicate_.empty() && n > 0) {
    std::int64_t matches = 0;
    external_matches.ptr = external_predicate_.getMatchesForBlock(block, &matches, lip_filter);
    lip_filter = static_cast<const std::uint64_t *>(external_matches.ptr);
  }
  // A block with compressed operand attributes whose values have not been materialised: aggregate on the codes.
  // (Key and predicate columns of the state take the value path here: stripe() decodes them once per block.)
  // null bitmaps of the nullable operand attributes (a block may hold none: loadBlock without bitmaps)
  const std::uint64_t *nulls[QSX_MAX_COLUMNS] = {};
  bool any_nulls = false;
  for (std::size_t i = 0; i < column_attr_.size(); ++i) {
    if (column_attr_[i] == kInvalidAttributeID) continue;   // a derived column: below
    nulls[i] = config_.column_nullable[i] != 0 ? block.nullBitmap(column_attr_[i]) : nullptr;
    any_nulls = any_nulls || nulls[i] != nullptr;
  }
  // the CASE arguments of the block: their values (and null bitmaps) stand where an attribute's would; they live until the
  // wait behind the update
  std::vector<std::unique_ptr<DeviceBuffer>> case_scratch;
  const void *derived[QSX_MAX_COLUMNS] = {};
  for (const auto &cc : case_columns_) {
    case_scratch.emplace_back(new DeviceBuffer(static_cast<std::size_t>(n) * 8 + 16));
    derived[cc->column] = case_scratch.back()->ptr;
    std::uint64_t *bits = nullptr;
    if (cc->evaluator.nullable) {
      case_scratch.emplace_back(new DeviceBuffer(static_cast<std::size_t>((n + 63) / 64) * 8 + 16));
      bits = static_cast<std::uint64_t *>(case_scratch.back()->ptr);
      if (n > 0) {
        nulls[cc->column] = bits;
        any_nulls = true;
      }
    }
    cc->evaluator.evalBlock(block, const_cast<void *>(derived[cc->column]), bits);
  }
  // the unary group-by keys of the block likewise; a key is NULL where its operand is
  for (const auto &uc : unary_columns_) {
    const UnaryEvaluator &ev = uc->evaluator;
    case_scratch.emplace_back(new DeviceBuffer(static_cast<std::size_t>(n) * static_cast<std::size_t>(ev.result.width) + 16));
    derived[uc->column] = case_scratch.back()->ptr;
    if (ev.evalBlock(block, case_scratch.back()->ptr, &case_scratch)) ++unary_coded_blocks_;
    nulls[uc->column] = ev.result.nullable && n > 0 ? block.nullBitmap(ev.operand) : nullptr;
    any_nulls = any_nulls || nulls[uc->column] != nullptr;
  }
  int code_width[QSX_MAX_COLUMNS] = {};
  bool any_coded = false;
  for (std::size_t i = 0; i < column_attr_.size() && !any_nulls && case_columns_.empty() && unary_columns_.empty(); ++i) {
    const CompressedAttribute *ca = block.compressedAttribute(column_attr_[i]);
    const int type = config_.column_type[i];
    if (ca != nullptr && type != kChar && !ca->variable_length && internedKeyOf(i) < 0 && !block.valuesMaterialized(column_attr_[i])) {
      code_width[i] = ca->code_width;
      any_coded = true;
    }
  }
  // the id stripes of the interned CHAR(n) keys stand where the attribute's stripe would (under the filter the update gets)
  InternScratch intern_scratch;
  std::vector<InternRequest> intern(1, InternRequest{&block, lip_filter, {}, {}});
  if (!unary_columns_.empty()) intern[0].derived.assign(derived, derived + QSX_MAX_COLUMNS);
  if (n > 0) internBlocks(&intern, &intern_scratch);
  const auto stripe_of = [&](std::size_t i) -> const void * {
    const int key = internedKeyOf(i);
    if (key >= 0 && n > 0) return intern[0].ids[key];
    return column_attr_[i] == kInvalidAttributeID ? derived[i] : block.stripe(column_attr_[i]);
  };
  if (any_coded && n > 0) {
    bool use_coded = false;
    {
      std::lock_guard<std::mutex> lock(coded_mutex_);
      if (coded_state_ == nullptr && !coded_merged_) {
        coded_config_ = config_;
        for (std::size_t i = 0; i < column_attr_.size(); ++i) coded_config_.column_code_width[i] = code_width[i];
        externalizeCodedPredicate();
        CheckStatus(qsx_agg_state_create(&coded_config_, &coded_state_), "qsx_agg_state_create");
      }
      if (coded_state_ != nullptr && !coded_merged_) {
        use_coded = true;
        for (std::size_t i = 0; i < column_attr_.size(); ++i) use_coded = use_coded && coded_config_.column_code_width[i] == code_width[i];
      }
    }
    if (use_coded) {
      const void *cols[QSX_MAX_COLUMNS];
      const void *dicts[QSX_MAX_COLUMNS];
      std::int32_t dict_entries[QSX_MAX_COLUMNS] = {};
      for (std::size_t i = 0; i < column_attr_.size(); ++i) {
        const CompressedAttribute *ca = code_width[i] != 0 ? block.compressedAttribute(column_attr_[i]) : nullptr;
        cols[i] = ca != nullptr ? ca->codes : stripe_of(i);
        dicts[i] = ca != nullptr && ca->kind == CompressedAttribute::kDictionary ? ca->dictionary : nullptr;
        dict_entries[i] = dicts[i] != nullptr ? static_cast<std::int32_t>(ca->num_codes) : 0;
      }
      OwnedBitmap predicate_matches;
      const std::uint64_t *coded_filter = lip_filter;
      if (coded_predicate_external_) {   // the state over code stripes leaves its predicate to the scans on codes (externalizeCodedPredicate)
        std::int64_t matches = 0;
        predicate_matches.ptr = spec_.predicate->getMatchesForBlock(block, &matches, lip_filter);
        coded_filter = static_cast<const std::uint64_t *>(predicate_matches.ptr);
      }
      CheckStatus(qsx_agg_update_coded_sized(coded_state_, cols, dicts, dict_entries, n, coded_filter, CurrentStream()),
                  "qsx_agg_update_coded_sized");
      ++coded_blocks_;
      CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
      return;
    }
  }
  const void *cols[QSX_MAX_COLUMNS];
  for (std::size_t i = 0; i < column_attr_.size(); ++i) cols[i] = stripe_of(i);
  if (any_nulls) {
    CheckStatus(qsx_agg_update_nullable(state_, cols, nulls, n, lip_filter, CurrentStream()), "qsx_agg_update_nullable");
  } else {
    CheckStatus(qsx_agg_update(state_, cols, n, lip_filter, CurrentStream()), "qsx_agg_update");
  }
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
}

// The state over code stripes leaves a predicate that the kernel would have evaluated on DECODED values to the scans on codes
// instead (Predicate::getMatchesForBlock / RunPredicateMatches: the comparison rewritten on every block's own dictionary,
// storage/CompressedStoreUtil.cpp:51-140 — a code stripe is an eighth of the column) and takes the resulting TupleIdSequence as
// its filter.  The state then has no predicate of its own, which also lets its aggregates factor through the dictionary codes
// (csrc/agg_factored.hpp): TPC-H Q1's l_shipdate <= DATE over lineitem's compressed blocks.  Called with coded_mutex_ held.
void AggregationOperationState::externalizeCodedPredicate() {
  if (coded_config_.num_pred_terms > 0 && spec_.predicate != nullptr && external_predicate_.empty()) {
    coded_config_.num_pred_terms = 0;
    coded_predicate_external_ = true;
  }
}

// A run of blocks through a state with derived columns — CASE arguments and unary group-by keys.  The unary keys by one
// _blocks launch each (UnaryEvaluator::evalBlocks), and then, as for the CASE arguments: the WHEN predicates over the run (RunPredicateMatches), the derived
// columns by one qsx_eval_case_blocks each, one qsx_agg_update_blocks — when no derived column can be NULL (the TPC-H shape:
// ELSE 0 over non-nullable attributes) and the run forms cover the blocks; otherwise block by block, like nullable attributes.
void AggregationOperationState::aggregateBlocksWithDerivedColumns(const std::vector<BlockReference> &blocks,
                                                        const std::vector<const std::uint64_t *> &lip_filters) {
  bool in_run = state_ != nullptr && distinctify_.empty() && external_predicate_.empty();
  for (const auto &cc : case_columns_) in_run = in_run && !cc->evaluator.nullable;
  std::vector<BlockReference> run;
  std::vector<std::int64_t> rows;
  std::vector<const std::uint64_t *> filters;
  bool any_filter = false;
  for (std::size_t i = 0; i < blocks.size() && in_run; ++i) {
    if (blocks[i]->numTuples() == 0) continue;
    for (attribute_id a : column_attr_) {
      if (a != kInvalidAttributeID && blocks[i]->nullBitmap(a) != nullptr) in_run = false;
    }
    run.push_back(blocks[i]);
    rows.push_back(blocks[i]->numTuples());
    filters.push_back(i < lip_filters.size() ? lip_filters[i] : nullptr);
    any_filter = any_filter || filters.back() != nullptr;
  }
  std::vector<std::unique_ptr<DeviceBuffer>> case_scratch;
  std::vector<std::unique_ptr<RunMatches>> keep;
  // the unary keys of the run: a key over a nullable operand carries null bitmaps, which travel with single-block calls
  for (const auto &uc : unary_columns_) {
    for (const BlockReference &b : run) in_run = in_run && b->nullBitmap(uc->evaluator.operand) == nullptr;
  }
  std::vector<std::vector<void *>> unary_derived(unary_columns_.size());
  std::int64_t on_codes = 0;
  for (std::size_t k = 0; k < unary_columns_.size() && in_run && !run.empty(); ++k) {
    const UnaryEvaluator &ev = unary_columns_[k]->evaluator;
    for (std::int64_t n : rows) {
      case_scratch.emplace_back(new DeviceBuffer(static_cast<std::size_t>(n) * static_cast<std::size_t>(ev.result.width) + 16));
      unary_derived[k].push_back(case_scratch.back()->ptr);
    }
    on_codes += ev.evalBlocks(run, rows, unary_derived[k].data(), &case_scratch);
  }
  std::vector<std::vector<void *>> derived(case_columns_.size());
  for (std::size_t k = 0; k < case_columns_.size() && in_run && !run.empty(); ++k) {
    for (std::int64_t n : rows) {
      case_scratch.emplace_back(new DeviceBuffer(static_cast<std::size_t>(n) * 8 + 16));
      derived[k].push_back(case_scratch.back()->ptr);
    }
    in_run = case_columns_[k]->evaluator.evalBlocks(run, rows, derived[k].data(), &keep);
  }
  if (!in_run) {
    CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // (derived columns already queued are dropped)
    for (std::size_t i = 0; i < blocks.size(); ++i) aggregateBlock(*blocks[i], i < lip_filters.size() ? lip_filters[i] : nullptr);
    return;
  }
  if (run.empty()) return;
  InternScratch intern_scratch;
  std::vector<InternRequest> intern;
  if (!interned_.empty()) {
    for (std::size_t b = 0; b < run.size(); ++b) {
      intern.push_back(InternRequest{run[b].get(), filters[b], {}, {}});
      if (unary_columns_.empty()) continue;
      intern.back().derived.assign(QSX_MAX_COLUMNS, nullptr);
      for (std::size_t k = 0; k < unary_columns_.size(); ++k) intern.back().derived[static_cast<std::size_t>(unary_columns_[k]->column)] = unary_derived[k][b];
    }
    internBlocks(&intern, &intern_scratch);
  }
  std::vector<const void *> cols;
  for (std::size_t b = 0; b < run.size(); ++b) {
    for (std::size_t c = 0; c < column_attr_.size(); ++c) {
      const int key = internedKeyOf(c);
      if (key >= 0) {
        cols.push_back(intern[b].ids[static_cast<std::size_t>(key)]);
      } else if (column_attr_[c] == kInvalidAttributeID) {
        for (std::size_t k = 0; k < case_columns_.size(); ++k) if (static_cast<std::size_t>(case_columns_[k]->column) == c) cols.push_back(derived[k][b]);
        for (std::size_t k = 0; k < unary_columns_.size(); ++k) if (static_cast<std::size_t>(unary_columns_[k]->column) == c) cols.push_back(unary_derived[k][b]);
      } else {
        cols.push_back(run[b]->stripe(column_attr_[c]));
      }
    }
  }
  CheckStatus(qsx_agg_update_blocks(state_, static_cast<int>(rows.size()), rows.data(), cols.data(), any_filter ? filters.data() : nullptr,
                                    CurrentStream()), "qsx_agg_update_blocks");
  if (!case_columns_.empty()) case_run_blocks_ += static_cast<std::int64_t>(rows.size());
  if (!unary_columns_.empty()) unary_run_blocks_ += static_cast<std::int64_t>(rows.size());
  unary_coded_blocks_ += on_codes;
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");   // the scratch behind the derived columns and bitmaps goes back
}

void AggregationOperationState::aggregateBlocks(const std::vector<BlockReference> &blocks,
                                                const std::vector<const std::uint64_t *> &lip_filters) {
  if (!case_columns_.empty() || !unary_columns_.empty()) {   // states with derived columns
    aggregateBlocksWithDerivedColumns(blocks, lip_filters);
    return;
  }
  std::vector<std::int64_t> rows;
  std::vector<const void *> cols;
  std::vector<const std::uint64_t *> filters;
  bool any_filter = false;
  std::vector<std::int64_t> coded_rows;
  std::vector<const void *> coded_cols, coded_dicts;
  std::vector<std::int32_t> coded_entries;   // every block's dictionary sizes (the reference builds a dictionary per block)
  std::vector<const std::uint64_t *> coded_filters;
  std::vector<BlockReference> coded_refs;
  bool any_coded_filter = false;
  const bool state_allows = state_ != nullptr && distinctify_.empty() && external_predicate_.empty();
  // interned CHAR(n) keys: their id stripes are made for the whole run at once (internBlocks) and then stand where the
  // attribute's stripe would; until then the column's entry is a placeholder
  InternScratch intern_scratch;
  std::vector<InternRequest> intern;
  struct Placeholder { bool coded; std::size_t at; std::size_t request; int key; };
  std::vector<Placeholder> placeholders;
  const auto stripe_or_placeholder = [&](const StorageBlock &block, std::size_t c, bool coded, std::size_t at) -> const void * {
    const int key = internedKeyOf(c);
    if (key < 0) return block.stripe(column_attr_[c]);
    placeholders.push_back(Placeholder{coded, at, intern.size() - 1, key});
    return nullptr;
  };
  for (std::size_t i = 0; i < blocks.size(); ++i) {
    const StorageBlock &block = *blocks[i];
    const std::uint64_t *filter = i < lip_filters.size() ? lip_filters[i] : nullptr;
    bool in_run = state_allows && block.numTuples() > 0;
    int code_width[QSX_MAX_COLUMNS] = {};
    bool any_coded = false;
    for (std::size_t c = 0; c < column_attr_.size() && in_run; ++c) {
      // null bitmaps travel with single-block calls (qsx_agg_update_nullable)
      if (block.nullBitmap(column_attr_[c]) != nullptr) in_run = false;
      const CompressedAttribute *ca = block.compressedAttribute(column_attr_[c]);
      if (ca != nullptr && config_.column_type[c] != kChar && !ca->variable_length && internedKeyOf(c) < 0 &&
          !block.valuesMaterialized(column_attr_[c])) {
        code_width[c] = ca->code_width;          // aggregated on its codes, like aggregateBlock does
        any_coded = true;
      }
    }
    if (in_run && any_coded) {
      // compressed blocks: one run through the state over code stripes (created by the first such block, which fixes the code
      // widths; blocks that compressed differently go with the run of plain stripes)
      bool use_coded = false;
      {
        std::lock_guard<std::mutex> lock(coded_mutex_);
        if (coded_state_ == nullptr && !coded_merged_) {
          coded_config_ = config_;
          for (std::size_t c = 0; c < column_attr_.size(); ++c) coded_config_.column_code_width[c] = code_width[c];
          externalizeCodedPredicate();
          CheckStatus(qsx_agg_state_create(&coded_config_, &coded_state_), "qsx_agg_state_create");
        }
        if (coded_state_ != nullptr && !coded_merged_) {
          use_coded = true;
          for (std::size_t c = 0; c < column_attr_.size(); ++c) use_coded = use_coded && coded_config_.column_code_width[c] == code_width[c];
        }
      }
      if (!use_coded) {
        // a block that compressed an operand differently than the block the coded state was created for (another code width, or
        // not at all): its values — stripe() decodes them once — join the run of plain stripes instead of a call of their own
        rows.push_back(block.numTuples());
        if (!interned_.empty()) intern.push_back(InternRequest{&block, filter, {}, {}});
        for (std::size_t c = 0; c < column_attr_.size(); ++c) cols.push_back(stripe_or_placeholder(block, c, false, cols.size()));
        filters.push_back(filter);
        any_filter = any_filter || filter != nullptr;
        continue;
      }
      if (!interned_.empty()) intern.push_back(InternRequest{&block, filter, {}, {}});
      coded_rows.push_back(block.numTuples());
      coded_refs.push_back(blocks[i]);
      for (std::size_t c = 0; c < column_attr_.size(); ++c) {
        const CompressedAttribute *ca = code_width[c] != 0 ? block.compressedAttribute(column_attr_[c]) : nullptr;
        coded_cols.push_back(ca != nullptr ? ca->codes : stripe_or_placeholder(block, c, true, coded_cols.size()));
        coded_dicts.push_back(ca != nullptr && ca->kind == CompressedAttribute::kDictionary ? ca->dictionary : nullptr);
        coded_entries.push_back(coded_dicts.back() != nullptr ? static_cast<std::int32_t>(ca->num_codes) : 0);
      }
      coded_filters.push_back(filter);
      any_coded_filter = any_coded_filter || filter != nullptr;
      continue;
    }
    if (!in_run) {
      aggregateBlock(block, filter);
      continue;
    }
    rows.push_back(block.numTuples());
    if (!interned_.empty()) intern.push_back(InternRequest{&block, filter, {}, {}});
    for (std::size_t c = 0; c < column_attr_.size(); ++c) cols.push_back(stripe_or_placeholder(block, c, false, cols.size()));
    filters.push_back(filter);
    any_filter = any_filter || filter != nullptr;
  }
  internBlocks(&intern, &intern_scratch);
  for (const Placeholder &p : placeholders) (p.coded ? coded_cols : cols)[p.at] = intern[p.request].ids[p.key];
  RunMatches coded_matches;
  if (!coded_rows.empty() && coded_predicate_external_) {
    // the predicate over the run's code stripes: every term one launch, rewritten on every block's own codes
    // (RunPredicateMatches); a run the run forms do not cover goes block by block
    if (!RunPredicateCovers(*spec_.predicate, coded_refs)) {
      for (std::size_t b = 0; b < coded_refs.size(); ++b) aggregateBlock(*coded_refs[b], coded_filters[b]);
      coded_rows.clear();
    } else {
      RunPredicateMatches(*spec_.predicate, coded_refs, coded_rows, any_coded_filter ? coded_filters.data() : nullptr, &coded_matches);
      for (std::size_t b = 0; b < coded_refs.size(); ++b) coded_filters[b] = coded_matches.bitmaps[b];
      any_coded_filter = true;
    }
  }
  if (!coded_rows.empty()) {
    CheckStatus(qsx_agg_update_coded_blocks_sized(coded_state_, static_cast<int>(coded_rows.size()), coded_rows.data(), coded_cols.data(),
                                                  coded_dicts.data(), coded_entries.data(), any_coded_filter ? coded_filters.data() : nullptr,
                                                  CurrentStream()),
                "qsx_agg_update_coded_blocks_sized");
    coded_blocks_ += static_cast<int>(coded_rows.size());
    CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
  }
  if (rows.empty()) return;
  CheckStatus(qsx_agg_update_blocks(state_, static_cast<int>(rows.size()), rows.data(), cols.data(), any_filter ? filters.data() : nullptr,
                                    CurrentStream()), "qsx_agg_update_blocks");
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
}

// finalizeAggregate with DISTINCT aggregates: every distinctify table is reduced to its distinct tuples, which are
// aggregated once each into a table keyed like the final one (aggregateOnDistinctifyHashTableFor{Single,GroupBy},
// AggregationOperationState.cpp:652-670, 720-760); the per-aggregate results are then lined up on the group key.
void AggregationOperationState::finalizeWithDistinct(InsertDestination *dest) {
  const CatalogRelation &rel = *spec_.input_relation;
  const int nk = config_.num_keys;
  struct ResultSet {
    std::vector<std::unique_ptr<DeviceBuffer>> keys, vals;
    std::int64_t rows = 0;
    std::unique_ptr<DeviceBuffer> order;      // row numbers in ascending key order
  };
  auto finalize_into = [&](qsx_agg_state_t *state, const qsx_agg_config_t &cfg, const std::vector<Type> &val_types, ResultSet *out) {
    std::int64_t groups = 0;
    CheckStatus(qsx_agg_num_groups(state, &groups, CurrentStream()), "qsx_agg_num_groups");
    const std::int64_t cap = groups > 0 ? groups : 1;
    void *key_cols[QSX_MAX_KEYS];
    void *val_cols[QSX_MAX_AGGS];
    for (int k = 0; k < cfg.num_keys; ++k) {
      out->keys.emplace_back(new DeviceBuffer(static_cast<std::size_t>(cap) * cfg.column_width[cfg.key_column[k]] + 16));
      key_cols[k] = out->keys.back()->ptr;
    }
    for (int a = 0; a < cfg.num_aggs; ++a) {
      out->vals.emplace_back(new DeviceBuffer(static_cast<std::size_t>(cap) * val_types[a].width + 16));
      val_cols[a] = out->vals.back()->ptr;
    }
    DeviceBuffer rows(8);
    CheckStatus(qsx_agg_finalize(state, 0, 1, key_cols, val_cols, nullptr, cap, static_cast<std::int64_t *>(rows.ptr), CurrentStream()),
                "qsx_agg_finalize");
    out->rows = ReadCount(rows.ptr);
    if (out->rows == QSX_GROUPS_HASH_COLLISION) throw ExecutionError("qsx_agg_finalize: wide group-by key", QSX_ERR_HASH_COLLISION);
    if (cfg.num_keys > 0 && out->rows > 0) {   // ascending key order: the common order of all result sets
      const void *cols[QSX_MAX_KEYS];
      std::int32_t types[QSX_MAX_KEYS];
      for (int k = 0; k < cfg.num_keys; ++k) {
        cols[k] = out->keys[k]->ptr;
        types[k] = cfg.column_type[cfg.key_column[k]];
        if (types[k] == kChar && cfg.column_width[cfg.key_column[k]] != 1) {
          throw ExecutionError("DISTINCT aggregate: CHAR group-by keys wider than one byte", QSX_ERR_UNSUPPORTED);
        }
      }
      const std::size_t ws_bytes = qsx_sort_workspace_bytes(out->rows);
      DeviceBuffer ws(ws_bytes);
      out->order.reset(new DeviceBuffer(static_cast<std::size_t>(out->rows) * 4 + 16));
      CheckStatus(qsx_sort_permutation(cfg.num_keys, cols, types, nullptr, out->rows, static_cast<std::int32_t *>(out->order->ptr), ws.ptr,
                                       ws_bytes, CurrentStream()), "qsx_sort_permutation");
    }
  };

  // the non-DISTINCT aggregates
  ResultSet main;
  std::vector<Type> main_types;
  if (state_ != nullptr) {
    for (std::size_t a = 0; a < spec_.aggregates.size(); ++a) {
      if (main_agg_[a] < 0) continue;
      const AggregateSpec &ag = spec_.aggregates[a];
      Type expression_type = Type::Double();   // expressions evaluate in DOUBLE, but for integer-typed ones under the spec's flag
      if (ag.argument_expression != nullptr && spec_.integer_argument_arithmetic) {
        const TypeID id = ScalarResultType(ag.argument_expression, rel);
        if (id == kInt) expression_type = Type::Int();
        if (id == kLong) expression_type = Type::Long();
      }
      main_types.push_back(AggResultType(ag.function, ag.argument_expression != nullptr ? expression_type
                                                      : ag.argument == kInvalidAttributeID ? Type::Long() : rel.getAttributeType(ag.argument)));
    }
    finalize_into(state_, config_, main_types, &main);
  }
  // one result set per DISTINCT aggregate
  std::vector<ResultSet> distinct(distinctify_.size());
  for (std::size_t i = 0; i < distinctify_.size(); ++i) {
    Distinctify &d = *distinctify_[i];
    const AggregateSpec &ag = spec_.aggregates[d.agg_index];
    const std::size_t ncols = d.attrs.size();
    std::int64_t total = 0;
    for (const auto &chunk : d.chunks) total += chunk.rows;
    // all block-level tuples side by side, then distinct over the whole input
    std::vector<std::unique_ptr<DeviceBuffer>> all, tuples;
    for (std::size_t c = 0; c < ncols; ++c) {
      all.emplace_back(new DeviceBuffer(static_cast<std::size_t>(total) * d.types[c].width + 16));
      char *at = static_cast<char *>(all.back()->ptr);
      for (const auto &chunk : d.chunks) {
        const std::size_t bytes = static_cast<std::size_t>(chunk.rows) * d.types[c].width;
        CheckStatus(qsx_copy_on_device(at, chunk.cols[c]->ptr, bytes, CurrentStream()), "qsx_copy_on_device");
        at += bytes;
      }
    }
    std::int64_t rows = 0;
    if (total > 0) {
      const void *cols[QSX_MAX_KEYS];
      std::int32_t types[QSX_MAX_KEYS];
      for (std::size_t c = 0; c < ncols; ++c) { cols[c] = all[c]->ptr; types[c] = d.types[c].id; }
      const std::size_t ws_bytes = qsx_sort_workspace_bytes(total);
      DeviceBuffer ws(ws_bytes), tids(static_cast<std::size_t>(total) * 4 + 16), count(8);
      CheckStatus(qsx_distinct_rows(static_cast<int>(ncols), cols, types, total, nullptr, static_cast<std::int32_t *>(tids.ptr),
                                    static_cast<std::int64_t *>(count.ptr), ws.ptr, ws_bytes, CurrentStream()), "qsx_distinct_rows");
      rows = ReadCount(count.ptr);
      for (std::size_t c = 0; c < ncols; ++c) {
        tuples.emplace_back(new DeviceBuffer(static_cast<std::size_t>(rows) * d.types[c].width + 16));
        CheckStatus(qsx_gather(d.types[c].width, cols[c], static_cast<const std::int32_t *>(tids.ptr), rows, tuples.back()->ptr,
                               CurrentStream()), "qsx_gather");
      }
    }
    // the aggregate over the distinct tuples, keyed like the final table
    qsx_agg_config_t cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.strategy = config_.strategy;
    cfg.num_columns = static_cast<int>(ncols);
    for (std::size_t c = 0; c < ncols; ++c) {
      cfg.column_type[c] = d.types[c].id;
      cfg.column_width[c] = d.types[c].width;
    }
    cfg.num_keys = nk;
    for (int k = 0; k < nk; ++k) cfg.key_column[k] = k;
    cfg.num_aggs = 1;
    cfg.aggs[0].fn = AggFn(ag.function);             // COUNT(DISTINCT x) = COUNT(*) over the distinct tuples (no NULLs)
    if (ag.function != AggregationID::kCount) {
      cfg.aggs[0].arg.kind = QSX_OPD_COLUMN;
      cfg.aggs[0].arg.index = nk;
    }
    cfg.est_groups = config_.est_groups;
    cfg.num_entries = config_.num_entries;
    qsx_agg_state_t *state = nullptr;
    CheckStatus(qsx_agg_state_create(&cfg, &state), "qsx_agg_state_create");
    try {
      if (rows > 0) {
        const void *cols[QSX_MAX_KEYS];
        for (std::size_t c = 0; c < ncols; ++c) cols[c] = tuples[c]->ptr;
        CheckStatus(qsx_agg_update(state, cols, rows, nullptr, CurrentStream()), "qsx_agg_update");
      }
      finalize_into(state, cfg, {AggResultType(ag.function, d.types.back())}, &distinct[i]);
    } catch (...) {
      qsx_agg_state_destroy(state);
      throw;
    }
    CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
    qsx_agg_state_destroy(state);
  }
  // every result set holds the same groups (each group has at least one tuple in every table)
  const ResultSet &first = state_ != nullptr ? main : distinct.front();
  for (const ResultSet &r : distinct) {
    if (r.rows != first.rows) throw ExecutionError("DISTINCT aggregate: group sets differ", QSX_ERR_INVALID_ARGUMENT);
  }
  block_id id;
  BlockReference out = dest->getBlockForInsertion(first.rows > 0 ? first.rows : 1, &id);
  auto emit = [&](const ResultSet &r, const void *src, int width, attribute_id out_attr) {
    if (r.rows == 0) return;
    if (r.order != nullptr) {
      CheckStatus(qsx_gather(width, src, static_cast<const std::int32_t *>(r.order->ptr), r.rows, out->stripe(out_attr), CurrentStream()),
                  "qsx_gather");
    } else {
      CheckStatus(qsx_copy_on_device(out->stripe(out_attr), src, static_cast<std::size_t>(r.rows) * width, CurrentStream()),
                  "qsx_copy_on_device");
    }
  };
  for (int k = 0; k < nk; ++k) emit(first, first.keys[k]->ptr, config_.column_width[config_.key_column[k]], k);
  std::size_t next_distinct = 0;
  for (std::size_t a = 0; a < spec_.aggregates.size(); ++a) {
    const attribute_id out_attr = static_cast<attribute_id>(nk + a);
    if (main_agg_[a] >= 0) {
      emit(main, main.vals[main_agg_[a]]->ptr, main_types[main_agg_[a]].width, out_attr);
    } else {
      const ResultSet &r = distinct[next_distinct];
      emit(r, r.vals[0]->ptr, AggResultType(spec_.aggregates[a].function, distinctify_[next_distinct]->types.back()).width, out_attr);
      ++next_distinct;
    }
  }
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
  dest->returnBlock(id, first.rows);
}

void AggregationOperationState::buildExistenceMap(const StorageBlock &block, attribute_id build_attribute, const Type &type) {
  if (type.id != kInt && type.id != kLong) {   // LOG(FATAL) "Build attribute type not supported" (:203-206)
    throw ExecutionError("BuildAggregationExistenceMapOperator: build attribute must be INT or LONG", QSX_ERR_UNSUPPORTED);
  }
  CheckStatus(qsx_agg_mark_existence(state_, type.id, block.stripe(build_attribute), block.numTuples(), nullptr, CurrentStream()),
              "qsx_agg_mark_existence");
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
}

void AggregationOperationState::finalizeAggregate(std::size_t partition, std::size_t num_partitions, InsertDestination *dest) {
  {   // the state fed by compressed blocks joins the other one (same image layout: mergeFrom semantics)
    std::lock_guard<std::mutex> lock(coded_mutex_);
    if (coded_state_ != nullptr && !coded_merged_) {
      CheckStatus(qsx_agg_merge(state_, coded_state_, CurrentStream()), "qsx_agg_merge");
      CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
    }
    coded_merged_ = true;
  }
  if (!distinctify_.empty()) {
    // the distinctify tables are drained by one work order; the others of a partitioned finalize have nothing to emit
    if (partition == 0) finalizeWithDistinct(dest);
    return;
  }
  std::int64_t groups = 0;
  CheckStatus(qsx_agg_num_groups(state_, &groups, CurrentStream()), "qsx_agg_num_groups");
  block_id id;
  BlockReference out = dest->getBlockForInsertion(groups > 0 ? groups : 1, &id);
  void *key_cols[QSX_MAX_KEYS];
  void *val_cols[QSX_MAX_AGGS];
  std::uint8_t *null_cols[QSX_MAX_AGGS] = {};
  std::vector<std::unique_ptr<DeviceBuffer>> null_flags;
  // an interned CHAR(n) key is finalized as the ids the state grouped by, into scratch; its bytes follow below
  std::vector<std::unique_ptr<DeviceBuffer>> key_ids(static_cast<std::size_t>(config_.num_keys));
  for (int k = 0; k < config_.num_keys; ++k) {
    key_cols[k] = out->stripe(k);
    if (internedKeyOf(static_cast<std::size_t>(config_.key_column[k])) < 0) continue;
    key_ids[k].reset(new DeviceBuffer(static_cast<std::size_t>(out->capacity()) * 4 + 16));
    key_cols[k] = key_ids[k]->ptr;
  }
  for (int a = 0; a < config_.num_aggs; ++a) {
    val_cols[a] = out->stripe(config_.num_keys + a);
    // result types of SUM / AVG / MIN / MAX are nullable (AggregationHandleSum::getResultType ...->getNullableVersion()):
    // an output attribute declared nullable receives the NULL flags as its null bitmap
    if (out->nullBitmap(static_cast<attribute_id>(config_.num_keys + a)) != nullptr) {
      null_flags.emplace_back(new DeviceBuffer(static_cast<std::size_t>(out->capacity()) + 16));
      null_cols[a] = static_cast<std::uint8_t *>(null_flags.back()->ptr);
    }
  }
  DeviceBuffer rows(8);
  CheckStatus(qsx_agg_finalize(state_, static_cast<int>(partition), static_cast<int>(num_partitions), key_cols, val_cols,
                               null_flags.empty() ? nullptr : null_cols, out->capacity(), static_cast<std::int64_t *>(rows.ptr),
                               CurrentStream()),
              "qsx_agg_finalize");
  const std::int64_t written = ReadCount(rows.ptr);
  // a key wider than 8 bytes is grouped by its 64-bit hash and verified: two keys under one hash void the result
  if (written == QSX_GROUPS_HASH_COLLISION) throw ExecutionError("qsx_agg_finalize: wide group-by key", QSX_ERR_HASH_COLLISION);
  if (written > out->capacity()) throw ExecutionError("qsx_agg_finalize: more groups than the output block holds", QSX_ERR_CAPACITY);
  for (int k = 0; k < config_.num_keys && written > 0; ++k) {
    if (key_ids[k] == nullptr) continue;
    const InternedKey &key = interned_[static_cast<std::size_t>(internedKeyOf(static_cast<std::size_t>(config_.key_column[k])))];
    CheckStatus(qsx_char_dict_values(key.dictionary, static_cast<const std::int32_t *>(key_ids[k]->ptr), written, out->stripe(k), CurrentStream()),
                "qsx_char_dict_values");
  }
  for (int a = 0; a < config_.num_aggs && written > 0; ++a) {
    if (null_cols[a] == nullptr) continue;
    // byte flags -> TupleIdSequence-ordered bitmap: a scan of 1-byte "codes" for flag >= 1
    CheckStatus(qsx_select_codes(1, null_cols[a], written, QSX_CODE_GE, 1, 0, nullptr,
                                 out->nullBitmap(static_cast<attribute_id>(config_.num_keys + a)), static_cast<std::int64_t *>(rows.ptr),
                                 CurrentStream()), "qsx_select_codes(null flags)");
  }
  CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
  dest->returnBlock(id, written);
}

// ---------------------------------------------------------------------------
// QueryContext
// ---------------------------------------------------------------------------
QueryContext::~QueryContext() {
  for (auto &parts : join_tables_) {
    for (qsx_join_table_t *t : parts) qsx_join_table_destroy(t);
  }
  for (qsx_lip_filter_t *f : lip_filters_) qsx_lip_filter_destroy(f);
}
QueryContext::lip_filter_id QueryContext::addLIPFilter(qsx_lip_kind_t kind, std::int64_t cardinality, std::int64_t min_value,
                                                       bool is_anti) {
  qsx_lip_filter_t *f = nullptr;
  CheckStatus(qsx_lip_filter_create(kind, cardinality, min_value, is_anti ? 1 : 0, &f), "qsx_lip_filter_create");
  lip_filters_.push_back(f);
  return static_cast<lip_filter_id>(lip_filters_.size() - 1);
}
void QueryContext::destroyLIPFilter(lip_filter_id id) {
  qsx_lip_filter_destroy(lip_filters_.at(id));
  lip_filters_.at(id) = nullptr;
}
QueryContext::lip_deployment_id QueryContext::addLIPDeployment(LIPFilterDeployment deployment) {
  lip_deployments_.push_back(std::move(deployment));
  return static_cast<lip_deployment_id>(lip_deployments_.size() - 1);
}

// ---------------------------------------------------------------------------
// LIP filter builder / prober
// ---------------------------------------------------------------------------
LIPFilterBuilder::LIPFilterBuilder(const QueryContext::LIPFilterDeployment &deployment, const QueryContext &query_context) {
  for (const auto &e : deployment.build_entries) entries_.emplace_back(query_context.getLIPFilterMutable(e.lip_filter), e.attribute);
}
void LIPFilterBuilder::insertValueAccessor(const StorageBlock &block, const std::uint64_t *filter) const {
  for (const auto &e : entries_) {
    // a NULL is never inserted (SingleIdentityHashFilter.hpp:115-126, BitVectorExactFilter.hpp:115-128)
    std::unique_ptr<DeviceBuffer> not_null = NotNullFilter(block, {e.second}, filter);
    CheckStatus(qsx_lip_build(e.first, block.getRelation().getAttributeType(e.second).id, block.stripe(e.second),
                              block.numTuples(), not_null != nullptr ? static_cast<const std::uint64_t *>(not_null->ptr) : filter,
                              CurrentStream()), "qsx_lip_build");
    if (not_null != nullptr) CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
  }
}
bool LIPFilterBuilder::coversBlocks(const std::vector<BlockReference> &blocks) const {
  for (const auto &e : entries_) {
    for (const BlockReference &b : blocks) {
      if (b->nullBitmap(e.second) != nullptr) return false;   // (a compressed attribute is read as it lies: RunJoinKeys)
    }
  }
  return true;
}
bool LIPFilterBuilder::insertBlocks(const std::vector<BlockReference> &blocks, qsx_join_table_t *built_table, attribute_id table_key) const {
  if (!coversBlocks(blocks)) return false;
  std::vector<std::int64_t> rows;
  std::int64_t total_rows = 0;
  for (const BlockReference &b : blocks) {
    rows.push_back(b->numTuples());
    total_rows += b->numTuples();
  }
  for (const auto &e : entries_) {
    if (built_table != nullptr && e.second == table_key) {
      // the table holds these keys already: its head words are the filter's bits (QSX_ERR_UNSUPPORTED: not that kind of table
      // or filter, or the run is too short for a pass over the key range to pay — the keys one by one then)
      const int rc = qsx_lip_build_from_join_table(e.first, built_table, total_rows, CurrentStream());
      if (rc == QSX_OK) continue;
      if (rc != QSX_ERR_UNSUPPORTED) CheckStatus(rc, "qsx_lip_build_from_join_table");
    }
    // (INT / LONG attributes — the key types of a LIP filter — that a block holds compressed are read as they lie)
    const RunJoinKeys keys(blocks, {e.second}, rows);
    CheckStatus(qsx_lip_build_blocks_coded(e.first, blocks.front()->getRelation().getAttributeType(e.second).id,
                                           static_cast<std::int64_t>(blocks.size()), rows.data(), keys.ptr.data(), keys.coding(), nullptr,
                                           CurrentStream()),
                "qsx_lip_build_blocks");
  }
  return true;
}
LIPFilterAdaptiveProber::LIPFilterAdaptiveProber(const QueryContext::LIPFilterDeployment &deployment,
                                                 const QueryContext &query_context) {
  for (const auto &e : deployment.probe_entries) entries_.emplace_back(query_context.getLIPFilterMutable(e.lip_filter), e.attribute);
}
void *LIPFilterAdaptiveProber::filterValueAccessor(const StorageBlock &block, const std::uint64_t *filter,
                                                   std::int64_t *num_hits) const {
  const std::int64_t n = block.numTuples();
  const std::size_t bytes = static_cast<std::size_t>((n + 63) / 64) * 8 + 8;
  void *current = nullptr, *next = nullptr;
  CheckStatus(qsx_device_alloc(bytes, &current), "qsx_device_alloc(bitmap)");
  CheckStatus(qsx_device_alloc(bytes, &next), "qsx_device_alloc(bitmap)");
  DeviceBuffer count(8);
  const std::uint64_t *in = filter;
  for (const auto &e : entries_) {
    // a NULL never passes a filter (SingleIdentityHashFilter.hpp:133-152)
    std::unique_ptr<DeviceBuffer> not_null = NotNullFilter(block, {e.second}, in);
    if (not_null != nullptr) in = static_cast<const std::uint64_t *>(not_null->ptr);
    CheckStatus(qsx_lip_probe(e.first, block.getRelation().getAttributeType(e.second).id, block.stripe(e.second), n, in,
                              static_cast<std::uint64_t *>(next), static_cast<std::int64_t *>(count.ptr), CurrentStream()),
                "qsx_lip_probe");
    if (not_null != nullptr) CheckStatus(qsx_stream_synchronize(CurrentStream()), "qsx_stream_synchronize");
    std::swap(current, next);
    in = static_cast<const std::uint64_t *>(current);
  }
  if (num_hits != nullptr) *num_hits = ReadCount(count.ptr);
  qsx_device_free(next);
  return current;
}
bool LIPFilterAdaptiveProber::filterBlocks(const std::vector<BlockReference> &blocks, void **storage,
                                           std::vector<const std::uint64_t *> *bitmaps, std::int64_t *num_hits,
                                           const std::uint64_t *const *in_bitmaps) const {
  *storage = nullptr;
  for (const auto &e : entries_) {
    for (const BlockReference &b : blocks) {
      if (b->nullBitmap(e.second) != nullptr) return false;   // (a compressed attribute is read as it lies: RunJoinKeys)
    }
  }
  const std::size_t nb = blocks.size();
  std::vector<std::int64_t> rows;
  std::size_t words = 0;
  for (const BlockReference &b : blocks) {
    rows.push_back(b->numTuples());
    words += static_cast<std::size_t>((b->numTuples() + 63) / 64) + 1;
  }
  // two sets of per-block bitmaps in one allocation; the filters ping-pong between them and the result ends in the first
  CheckStatus(qsx_device_alloc(2 * words * 8 + 8, storage), "qsx_device_alloc(bitmaps)");
  std::vector<std::uint64_t *> cur(nb), nxt(nb);
  std::size_t at = 0;
  for (std::size_t b = 0; b < nb; ++b) {
    cur[b] = static_cast<std::uint64_t *>(*storage) + at;
    nxt[b] = static_cast<std::uint64_t *>(*storage) + words + at;
    at += static_cast<std::size_t>((rows[b] + 63) / 64) + 1;
  }
  DeviceBuffer count(8);
  bool first = true;
  for (const auto &e : entries_) {
    const RunJoinKeys keys(blocks, {e.second}, rows);   // (a compressed INT / LONG attribute: its code stripes, as they lie)
    CheckStatus(qsx_lip_probe_blocks_coded(e.first, blocks.front()->getRelation().getAttributeType(e.second).id, static_cast<std::int64_t>(nb),
                                           rows.data(), keys.ptr.data(), keys.coding(),
                                           first ? in_bitmaps : reinterpret_cast<const std::uint64_t *const *>(cur.data()), nxt.data(),
                                           static_cast<std::int64_t *>(count.ptr), CurrentStream()), "qsx_lip_probe_blocks");
    std::swap(cur, nxt);
    first = false;
  }
  if (num_hits != nullptr) {
    *num_hits = 0;
    if (first) {
      for (std::int64_t r : rows) *num_hits += r;
    } else {
      *num_hits = ReadCount(count.ptr);
    }
  }
  if (first && in_bitmaps != nullptr) {   // no filter attached: what came in
    for (std::size_t b = 0; b < nb; ++b) {
      if (rows[b] > 0) CheckStatus(qsx_bitmap_combine(0, in_bitmaps[b], in_bitmaps[b], rows[b], cur[b], CurrentStream()), "qsx_bitmap_combine");
    }
  } else if (first) {   // no filter attached: every tuple
    for (std::size_t b = 0; b < nb; ++b) {
      CheckStatus(qsx_memset_device(nxt[b], 0xFF, static_cast<std::size_t>((rows[b] + 63) / 64) * 8, CurrentStream()), "qsx_memset_device");
      if (rows[b] > 0) {
        CheckStatus(qsx_bitmap_combine(0, nxt[b], nxt[b], rows[b], cur[b], CurrentStream()), "qsx_bitmap_combine");   // clears the tail bits
      }
    }
  }
  bitmaps->assign(cur.begin(), cur.end());
  return true;
}
LIPFilterBuilder *CreateLIPFilterBuilderHelper(QueryContext::lip_deployment_id id, const QueryContext *query_context) {
  const QueryContext::LIPFilterDeployment *d = query_context->getLIPDeployment(id);
  return d == nullptr || d->build_entries.empty() ? nullptr : new LIPFilterBuilder(*d, *query_context);
}
LIPFilterAdaptiveProber *CreateLIPFilterAdaptiveProberHelper(QueryContext::lip_deployment_id id, const QueryContext *query_context) {
  const QueryContext::LIPFilterDeployment *d = query_context->getLIPDeployment(id);
  return d == nullptr || d->probe_entries.empty() ? nullptr : new LIPFilterAdaptiveProber(*d, *query_context);
}
QueryContext::predicate_id QueryContext::addPredicate(Predicate p) {
  predicates_.push_back(std::move(p));
  return static_cast<predicate_id>(predicates_.size() - 1);
}
QueryContext::scalar_group_id QueryContext::addScalarGroup(std::vector<attribute_id> attrs) {
  scalar_groups_.push_back(std::move(attrs));
  return static_cast<scalar_group_id>(scalar_groups_.size() - 1);
}
QueryContext::join_hash_table_id QueryContext::addJoinHashTable(TypeID key_type, std::int64_t estimated_entries,
                                                                std::size_t num_partitions,
                                                                const ExactKeyRange *exact_key_range) {
  std::vector<qsx_join_table_t *> parts(num_partitions, nullptr);
  if (key_type == kVarChar) throw ExecutionError("a VARCHAR attribute as a join key", QSX_ERR_UNSUPPORTED);
  if (key_type == kChar) key_type = kLong;   // a CHAR(n <= 8) key travels as the LONG qsx_join_key_pack_char makes of it
  for (std::size_t p = 0; p < num_partitions; ++p) {
    if (exact_key_range != nullptr) {
      // every partition addresses the whole range: the single-node partition function is not a stride of the key
      CheckStatus(qsx_join_table_create_dense(key_type, exact_key_range->min_value, exact_key_range->max_value, 1,
                                              estimated_entries, &parts[p]),
                  "qsx_join_table_create_dense");
    } else {
      CheckStatus(qsx_join_table_create(key_type, estimated_entries, &parts[p]), "qsx_join_table_create");
    }
  }
  join_tables_.push_back(std::move(parts));
  return static_cast<join_hash_table_id>(join_tables_.size() - 1);
}
void QueryContext::destroyJoinHashTable(join_hash_table_id id, partition_id part) {
  // (DestroyHashOperator runs behind the last HashJoin work order, and every work order waits for its stream before it returns:
  // nothing queued uses the table — no wait for the other operators' kernels, qsx_join_table_release)
  qsx_join_table_release(join_tables_.at(id).at(part));
  join_tables_.at(id).at(part) = nullptr;
}
QueryContext::aggregation_state_id QueryContext::addAggregationState(const AggregationStateSpec &spec,
                                                                     std::size_t num_partitions) {
  std::vector<std::unique_ptr<AggregationOperationState>> parts;
  for (std::size_t p = 0; p < num_partitions; ++p) parts.emplace_back(new AggregationOperationState(spec));
  agg_states_.push_back(std::move(parts));
  return static_cast<aggregation_state_id>(agg_states_.size() - 1);
}
QueryContext::insert_destination_id QueryContext::addInsertDestination(CatalogRelation *relation,
                                                                       StorageManager *storage_manager) {
  destinations_.emplace_back(new InsertDestination(relation, storage_manager));
  return static_cast<insert_destination_id>(destinations_.size() - 1);
}
QueryContext::insert_destination_id QueryContext::addPartitionAwareInsertDestination(CatalogRelation *relation,
                                                                                     StorageManager *storage_manager) {
  if (!relation->hasPartitionScheme()) {
    throw ExecutionError("addPartitionAwareInsertDestination: the output relation has no partition scheme", QSX_ERR_INVALID_ARGUMENT);
  }
  destinations_.emplace_back(new InsertDestination(relation, storage_manager, relation->getNumPartitions(), relation->getPartitionAttribute()));
  return static_cast<insert_destination_id>(destinations_.size() - 1);
}

// has_repartition of an operator (RelationalOperator.hpp:311-320) and the kind of its InsertDestination must agree: a
// repartitioning operator whose destination would drop the partition scheme is a plan error, never silently accepted.
void CheckRepartition(const char *op, bool has_repartition, const InsertDestination *dest) {
  if (dest == nullptr || has_repartition == dest->isPartitionAware()) return;
  throw ExecutionError(std::string(op) + (has_repartition ? ": has_repartition needs a PartitionAwareInsertDestination (QueryContext::addPartitionAwareInsertDestination)"
                                                          : ": a PartitionAwareInsertDestination needs has_repartition = true"),
                       QSX_ERR_INVALID_ARGUMENT);
}

// ---------------------------------------------------------------------------
// WorkOrdersContainer
// ---------------------------------------------------------------------------
void WorkOrdersContainer::addNormalWorkOrder(WorkOrder *workorder, std::size_t operator_index) {
  std::lock_guard<std::mutex> lock(mutex_);
  queues_.at(operator_index).emplace_back(workorder);
}
bool WorkOrdersContainer::hasNormalWorkOrder(std::size_t operator_index) const {
  std::lock_guard<std::mutex> lock(mutex_);
  return !queues_.at(operator_index).empty();
}
WorkOrder *WorkOrdersContainer::getNormalWorkOrder(std::size_t operator_index) {
  std::lock_guard<std::mutex> lock(mutex_);
  auto &q = queues_.at(operator_index);
  if (q.empty()) return nullptr;
  WorkOrder *wo = q.front().release();
  q.pop_front();
  return wo;
}
std::size_t WorkOrdersContainer::getNumNormalWorkOrders(std::size_t operator_index) const {
  std::lock_guard<std::mutex> lock(mutex_);
  return queues_.at(operator_index).size();
}


}  // namespace quickstep
