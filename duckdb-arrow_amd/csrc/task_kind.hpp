// task_kind.hpp -- the one table of what a task kind (enum mi_kind) is: which kernel sees it, in which launch of a plan, how
// wide its output rows are.  Plain C++ over the C header alone, shared by the host (plan_layout.cpp, engine.cpp, the scan) and
// the kernels: every function is constexpr and callable from both sides.
#pragma once

#include <cstdint>

#include "../../include/mi_arrow_ipc.h"

#if defined(__HIPCC__)
// always_inline: left to the inliner, transcode_misc_light called MiscGroupOfKind where it had inlined its own copy of the switch
#define MI_HD __host__ __device__ __attribute__((always_inline))
#else
#define MI_HD
#endif

namespace miarrow {
namespace device {

// rows per tile == DuckDB STANDARD_VECTOR_SIZE: one tile is one output vector.  The kernels know the number as kTileRows
// (kernels.hpp, beside kBlockThreads: the suite reads both from that file), which is held equal to this one there.
constexpr int kVectorRows = 2048;
#ifndef MI_COPY_TILE_ROWS
#define MI_COPY_TILE_ROWS 2048
#endif
#ifndef MI_DEC_TILE_ROWS
#define MI_DEC_TILE_ROWS 2048
#endif
constexpr int kCopyTileRows = MI_COPY_TILE_ROWS;  // copy / dec128 tiles may span several vectors (multiples of 2048)
constexpr int kDecTileRows = MI_DEC_TILE_ROWS;

// Kernel classes: a plan groups its tasks by class and launches one kernel per non-empty class.  Statistics (bytes, rows,
// tiles, milliseconds) are kept per class.
enum KernelClass { kClassCopy = 0, kClassDec128 = 1, kClassString = 2, kClassMisc = 3, kClassEncFixed = 4, kClassEncString = 5, kClassGather = 6,
                   kNumClasses = 7 };

MI_HD constexpr int TileRowsOfClass(int cls) { return cls == kClassCopy ? kCopyTileRows : cls == kClassDec128 ? kDecTileRows : kVectorRows; }

// the dominant kernel of every class, as rocprofv3 prints it
constexpr const char* KernelNameOfClass(int cls) {
  switch (cls) {
    case kClassCopy: return "transcode_copy";
    case kClassDec128: return "transcode_dec128";
    case kClassString: return "transcode_string";
    case kClassMisc: return "transcode_misc_light";
    case kClassEncFixed: return "encode_fixed";
    case kClassEncString: return "encode_string_1p";
    case kClassGather: return "transcode_gather";
    default: return "";
  }
}

// What a slice of a plan launches: one of the classes (same values as KernelClass), or one of the four kinds whose kernel
// lives outside the class kernels -- transcode_run_end (kernels_run_end.hip), encode_string_view (kernels_encode_view.hip),
// transcode_union / transcode_union_dense (kernels_union.hip).
enum LaunchSlot { kSlotRunEnd = kNumClasses, kSlotEncView, kSlotUnionTags, kSlotUnionDense, kNumSlots };

// A plan launches pass by pass, inside a pass depth by depth (shallow first: a child sees its parent's finished validity
// words), inside a depth by position.
//   pass 0: the classes, then the union tag passes -- their masks are the parent words of their members, one level deeper;
//   pass 1: run-end and dense-union expansions -- they read the decoded vectors of children deeper than they are;
//   pass 2: string-view encode -- it reads the look-back words encode_string_1p's slice left.
struct SlotInfo {
  int8_t pass, position;
  int8_t cls;          // the class this slot's bytes, rows, tiles and milliseconds are accounted under
  int32_t tile_rows;
};
constexpr SlotInfo kSlots[kNumSlots] = {
    {0, 0, kClassCopy, TileRowsOfClass(kClassCopy)},
    {0, 1, kClassDec128, TileRowsOfClass(kClassDec128)},
    {0, 2, kClassString, TileRowsOfClass(kClassString)},
    {0, 3, kClassMisc, TileRowsOfClass(kClassMisc)},
    {0, 4, kClassEncFixed, TileRowsOfClass(kClassEncFixed)},
    {0, 5, kClassEncString, TileRowsOfClass(kClassEncString)},
    {0, 6, kClassGather, TileRowsOfClass(kClassGather)},
    {1, 0, kClassMisc, kVectorRows},        // kSlotRunEnd
    {2, 0, kClassEncString, kVectorRows},   // kSlotEncView
    {0, 7, kClassMisc, kVectorRows},        // kSlotUnionTags
    {1, 1, kClassMisc, kVectorRows},        // kSlotUnionDense
};
constexpr int kNumPasses = 3;
//! the slot launched at `position` of `pass`, -1 past the last one
constexpr int SlotAt(int pass, int position) {
  for (int s = 0; s < kNumSlots; s++)
    if (kSlots[s].pass == pass && kSlots[s].position == position) return s;
  return -1;
}

//! -1 for an unknown kind
MI_HD constexpr int SlotOfKind(int32_t kind) {
  switch (kind) {
    case MI_K_COPY: return kClassCopy;
    case MI_K_DEC128: return kClassDec128;
    case MI_K_STR32: case MI_K_STR64: case MI_K_FIXED_BINARY: return kClassString;
    case MI_K_BOOL: case MI_K_DATE64: case MI_K_MUL_I32: case MI_K_MUL_I64: case MI_K_DIV_I64: case MI_K_DURATION:
    case MI_K_DICT: case MI_K_INTERVAL_MONTHS: case MI_K_INTERVAL_MDN: case MI_K_NARROW: case MI_K_HALF_FLOAT:
    case MI_K_NULL: case MI_K_STRVIEW: case MI_K_LIST32: case MI_K_LIST64: case MI_K_STRUCT: case MI_K_UUID: case MI_K_BOOL8: return kClassMisc;
    case MI_K_ENC_COPY: case MI_K_ENC_DEC128: case MI_K_ENC_BOOL: case MI_K_ENC_VALIDITY: case MI_K_ENC_UUID_TEXT:
    case MI_K_ENC_INTERVAL: case MI_K_ENC_UNION: return kClassEncFixed;
    case MI_K_ENC_STR32: case MI_K_ENC_LIST32: return kClassEncString;
    case MI_K_RUN_END: return kSlotRunEnd;
    case MI_K_ENC_STRVIEW: return kSlotEncView;
    case MI_K_UNION: return kSlotUnionTags;
    case MI_K_UNION_DENSE: return kSlotUnionDense;
    default: return -1;
  }
}
//! the class whose kernels take the kind; -1 for an unknown kind and for the kinds with a kernel of their own
MI_HD constexpr int ClassOfKind(int32_t kind) { return SlotOfKind(kind) < kNumClasses ? SlotOfKind(kind) : -1; }

// which transcode_misc kernel owns a kind of the misc class: 0 / 3 common flat kinds (one wave per tile; 3 = 8-byte inputs),
// 1 nested, 2 rare flat
MI_HD constexpr int MiscGroupOfKind(int32_t kind) {
  switch (kind) {
    case MI_K_BOOL: case MI_K_DICT: case MI_K_MUL_I32: return 0;
    case MI_K_DATE64: case MI_K_MUL_I64: case MI_K_DIV_I64: return 3;
    case MI_K_STRUCT: case MI_K_LIST32: case MI_K_LIST64: case MI_K_STRVIEW: return 1;
    default: return 2;
  }
}

//! kinds transcode_gather (kernels_gather.hip) decodes through a selection vector
MI_HD constexpr bool KindCanGather(int32_t kind) {
  switch (kind) {
    case MI_K_COPY: case MI_K_DEC128: case MI_K_STR32: case MI_K_STR64: case MI_K_FIXED_BINARY: case MI_K_BOOL: case MI_K_DATE64:
    case MI_K_MUL_I32: case MI_K_MUL_I64: case MI_K_DIV_I64: case MI_K_DICT: case MI_K_UUID: case MI_K_BOOL8:
      return true;
    default:
      return false;
  }
}

//! slot of a task: gather mode (mi_col_task.sel) has its own kernel; -1 when the kind is unknown or cannot be gathered
MI_HD constexpr int SlotOfTask(const mi_col_task& t) {
  return t.sel != nullptr ? (KindCanGather(t.kind) ? static_cast<int>(kClassGather) : -1) : SlotOfKind(t.kind);
}
MI_HD constexpr int ClassOfTask(const mi_col_task& t) { return SlotOfTask(t) < kNumClasses ? SlotOfTask(t) : -1; }

//! bytes per output row of a decode kind (what ArrowField::Plan reports as out_width); 0 for STRUCT, encode and unknown kinds
MI_HD constexpr int OutWidth(int32_t kind, int64_t param) {
  switch (kind) {
    case MI_K_COPY: case MI_K_DEC128: case MI_K_UNION_DENSE: return static_cast<int>(param);
    case MI_K_BOOL: case MI_K_BOOL8: case MI_K_NULL: case MI_K_UNION: return 1;
    case MI_K_DATE64: case MI_K_HALF_FLOAT: case MI_K_DICT: return 4;
    case MI_K_MUL_I32: case MI_K_MUL_I64: case MI_K_DIV_I64: return 8;
    case MI_K_STR32: case MI_K_STR64: case MI_K_FIXED_BINARY: case MI_K_STRVIEW: case MI_K_LIST32: case MI_K_LIST64:
    case MI_K_DURATION: case MI_K_INTERVAL_MONTHS: case MI_K_INTERVAL_MDN: case MI_K_UUID: return 16;
    case MI_K_NARROW: case MI_K_RUN_END: return static_cast<int>((param >> 8) & 0xFF);
    default: return 0;
  }
}

//! whether any row of the task can be NULL: it has a bitmap that counts, or a parent whose NULLs propagate
MI_HD constexpr bool TaskNeedsMask(const mi_col_task& t) {
  return (t.validity != nullptr && t.null_count != 0) || t.out_aux != nullptr;
}

// ClassSlice::kernel_mask is the OR of this over the slice's tasks: which of the kernels that serve the slot have tiles, so
// that the launcher starts only those.
//   misc:              1 << MiscGroupOfKind -- bit 0 transcode_misc_light<false>, bit 1 transcode_misc<1> (nested), bit 2
//                      transcode_misc<2> (rare flat), bit 3 transcode_misc_light<true> (8-byte inputs)
//   dec128, string:    bit 0 the instance for tiles without NULLs, bit 1 the one for tiles that need a mask (TaskNeedsMask)
//   enc_fixed:         bit 0 encode_fixed, bit 1 encode_uuid_text, bit 2 encode_union (launched first: its masks are the validity of
//                      its members' tasks, which are tasks of this slice or of a later one)
//   enc_string:        bit 1 the slice has lists (strings set nothing)
//   every other slot:  one kernel, 0
MI_HD constexpr uint32_t KernelMaskOfTask(int slot, const mi_col_task& t) {
  switch (slot) {
    case kClassMisc: return 1u << MiscGroupOfKind(t.kind);
    case kClassDec128: case kClassString: return TaskNeedsMask(t) ? 2u : 1u;
    case kClassEncFixed: return t.kind == MI_K_ENC_UUID_TEXT ? 2u : t.kind == MI_K_ENC_UNION ? 4u : 1u;
    case kClassEncString: return t.kind == MI_K_ENC_LIST32 ? 2u : 0u;
    default: return 0u;
  }
}

}  // namespace device
}  // namespace miarrow
