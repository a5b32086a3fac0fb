// scan_column.hpp -- a column of a scan's bind result and what its Arrow field says about its values: the questions the
// filter binding, the dictionaries and the fused aggregates all ask of a column.  Host code over ipc_format.hpp alone.
#pragma once

#include <string>

#include "ipc_format.hpp"

namespace miarrow {

struct ScanColumn {
  std::string name;
  ArrowField field;           // arrow field of the first file that has it
  bool is_filename = false;   // `filename` option (README.md:104-107)
  bool is_hive = false;       // hive partition key
  std::string hive_key;
  //! one value per file, made on the host: never read from a file, decoded or filtered on the GPU
  bool is_constant() const { return is_filename || is_hive; }
};

//! a run-end encoded column is filtered on its flat vector: what matters is the field of its values
inline const ArrowField& ValueField(const ArrowField& f) { return f.type == MI_AT_RUN_END && f.children.size() == 2 ? f.children[1] : f; }
//! Columns a range comparison / the fused aggregate reads as integers: integers, DATE, TIME / TIMESTAMP, DECIMAL(<= 18)
//! -- and booleans where `allow_bool` -- by their transcode plan
inline bool IsIntegerLike(int32_t kind, int32_t width, const ArrowField& f, bool allow_bool) {
  return (kind == MI_K_COPY || kind == MI_K_DEC128 || kind == MI_K_DATE64 || kind == MI_K_MUL_I32 || kind == MI_K_MUL_I64 ||
          kind == MI_K_DIV_I64 || kind == MI_K_NARROW || (allow_bool && (kind == MI_K_BOOL || kind == MI_K_BOOL8))) &&
         (width == 1 || width == 2 || width == 4 || width == 8) && f.type != MI_AT_FLOAT;
}
inline bool IsStringKind(int32_t kind) { return kind == MI_K_STR32 || kind == MI_K_STR64 || kind == MI_K_FIXED_BINARY; }

//! what a column's values are compared as by a pushed-down filter
enum class FilterValueClass { kOther, kFloat32, kFloat64, kWide };
inline FilterValueClass FilterClassOf(const ArrowField& field) {
  const ArrowField& vf = ValueField(field);
  int32_t kind, w;
  int64_t param;
  if (!vf.Plan(&kind, &param, &w, /*value_only*/ true)) return FilterValueClass::kOther;
  if (vf.type == MI_AT_FLOAT && (w == 4 || w == 8)) return w == 4 ? FilterValueClass::kFloat32 : FilterValueClass::kFloat64;
  if (vf.type == MI_AT_DECIMAL && kind == MI_K_COPY && w == 16) return FilterValueClass::kWide;
  if (kind == MI_K_UUID) return FilterValueClass::kWide;   // hugeint_t whose signed order is the order of the text
  return FilterValueClass::kOther;
}

}  // namespace miarrow
