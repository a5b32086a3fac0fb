// plan_layout.cpp -- validation, grouping and tile tables of a transcode plan.  See plan_layout.hpp.  No HIP here.
#include "plan_layout.hpp"

#include <algorithm>
#include <string>

#include "ipc_format.hpp"

namespace miarrow {

static void ValidateTask(const mi_col_task& t, size_t i) {
  auto fail = [&](const std::string& what) {
    throw InvalidInputException("task " + std::to_string(i) + ": " + what);
  };
  if (device::SlotOfKind(t.kind) < 0) fail("unknown kind " + std::to_string(t.kind));
  if (t.sel != nullptr) {  // gather mode: decode only the rows a selection vector names, compacted per 2048-row window
    if (!device::KindCanGather(t.kind)) fail("kind " + std::to_string(t.kind) + " cannot be decoded through a selection vector");
    if (t.sel_count == nullptr) fail("gather tasks need sel_count (rows selected per 2048-row window)");
    if (t.out_aux != nullptr || t.depth != 0) fail("gather tasks are top-level columns");
    if (reinterpret_cast<uintptr_t>(t.sel) % 4 != 0 || reinterpret_cast<uintptr_t>(t.sel_count) % 4 != 0) fail("selection vector misaligned");
  }
  if (t.nrows < 0) fail("negative row count");
  if (t.row_offset < 0) fail("negative row offset");
  if (t.depth < 0 || t.depth > 64) fail("bad nesting depth");
  if (t.nrows == 0) return;
  if (t.kind == MI_K_STRUCT) {
    if (t.out_validity == nullptr) fail("STRUCT tasks produce validity only: out_validity is NULL");
    if (reinterpret_cast<uintptr_t>(t.out_validity) % 8 != 0) fail("out_validity must be 8-byte aligned");
    return;
  }
  if (t.out_data == nullptr) fail("out_data is NULL");
  if (reinterpret_cast<uintptr_t>(t.out_data) % 16 != 0) fail("out_data must be 16-byte aligned");
  // decode writes validity words; encode writes an Arrow bitmap, which is bytes (whole words where they happen to be aligned)
  if (t.out_validity && t.kind < MI_K_ENC_COPY && reinterpret_cast<uintptr_t>(t.out_validity) % 8 != 0) fail("out_validity must be 8-byte aligned");
  if (t.validity && reinterpret_cast<uintptr_t>(t.validity) % 8 != 0) fail("validity bitmap must be 8-byte aligned");
  if (t.buf1 == nullptr && t.kind != MI_K_NULL) fail("buf1 is NULL");
  switch (t.kind) {
    case MI_K_LIST32: case MI_K_LIST64:
      if (reinterpret_cast<uintptr_t>(t.buf1) % (t.kind == MI_K_LIST32 ? 4 : 8) != 0) fail("offsets buffer misaligned");
      if (t.param < 0) fail("LIST needs param = child length");
      if (t.buf2 && t.buf2_len <= 0) fail("window table is empty");
      break;
    case MI_K_STRVIEW:
      if (reinterpret_cast<uintptr_t>(t.buf1) % 4 != 0) fail("views buffer misaligned");
      if (t.buf2_len > 0 && t.buf2 == nullptr) fail("STRVIEW needs the variadic buffer table in buf2");
      break;
    case MI_K_NARROW: {
      const int sw = static_cast<int>(t.param & 0xFF), dw = static_cast<int>((t.param >> 8) & 0xFF);
      if (!((sw == 4 && dw == 2) || (sw == 8 && (dw == 2 || dw == 4)))) fail("NARROW needs src 4->2 or 8->2/4");
      break;
    }
    case MI_K_COPY:
      if (t.param != 1 && t.param != 2 && t.param != 4 && t.param != 8 && t.param != 16) fail("COPY width must be 1,2,4,8,16");
      break;
    case MI_K_DEC128:
      if (t.param != 2 && t.param != 4 && t.param != 8) fail("DEC128 out width must be 2,4,8");
      if (reinterpret_cast<uintptr_t>(t.buf1) % 8 != 0) fail("decimal buffer must be 8-byte aligned");
      break;
    case MI_K_STR32:
    case MI_K_STR64:
      if (t.buf2 == nullptr && t.buf2_len != 0) fail("string data buffer is NULL");
      if (reinterpret_cast<uintptr_t>(t.buf1) % (t.kind == MI_K_STR32 ? 4 : 8) != 0) fail("offsets buffer misaligned");
      if (t.buf2 && reinterpret_cast<uintptr_t>(t.buf2) % 4 != 0) fail("string data buffer must be 4-byte aligned");
      if (t.buf2_len < 0) fail("negative buf2_len");
      break;
    case MI_K_FIXED_BINARY:
      if (t.param <= 0) fail("fixed binary width must be positive");
      if (reinterpret_cast<uintptr_t>(t.buf1) % 4 != 0) fail("fixed binary buffer must be 4-byte aligned");
      break;
    case MI_K_DICT: {
      int iw = static_cast<int>(t.param & 0xFF);
      if (iw != 1 && iw != 2 && iw != 4 && iw != 8) fail("dictionary index width must be 1,2,4,8");
      break;
    }
    case MI_K_MUL_I32: case MI_K_MUL_I64:
      if (t.param <= 0) fail("multiplier must be positive");
      break;
    case MI_K_DIV_I64:
      if (t.param <= 0) fail("divisor must be positive");
      break;
    case MI_K_DURATION:
      if (t.param == 0) fail("duration factor must be non-zero");
      break;
    case MI_K_UUID:
      if (reinterpret_cast<uintptr_t>(t.buf1) % 4 != 0) fail("uuid buffer must be 4-byte aligned");
      break;
    case MI_K_RUN_END: {
      const int64_t rw = t.param & 0xFF, w = (t.param >> 8) & 0xFF;
      if (rw != 2 && rw != 4 && rw != 8) fail("RUN_END run-end width must be 2,4,8");
      if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16) fail("RUN_END out width must be 1,2,4,8,16");
      if (reinterpret_cast<uintptr_t>(t.buf1) % rw != 0) fail("run ends misaligned");
      if (t.param2 <= 0) fail("RUN_END needs param2 = number of runs > 0");
      if (t.buf2 == nullptr || reinterpret_cast<uintptr_t>(t.buf2) % 16 != 0) fail("RUN_END needs the decoded values (16-byte aligned) in buf2");
      if (t.flags > 1) fail("RUN_END parents are structs (flags 0 or 1)");
      break;
    }
    case MI_K_UNION: {
      const int64_t words = (t.nrows + 63) / 64;
      if (t.param < 1 || t.param > MI_MAX_UNION_MEMBERS) fail("UNION needs param = number of members, 1 .. " + std::to_string(MI_MAX_UNION_MEMBERS));
      if (t.buf2 == nullptr || reinterpret_cast<uintptr_t>(t.buf2) % 8 != 0) fail("UNION needs the union table (8-byte aligned) in buf2");
      if (t.ptr_base % 4 != 0) fail("UNION dense offsets misaligned");
      if (t.param2 <= 0 || t.param2 % 8 != 0 || t.param2 < t.nrows) fail("UNION needs param2 = distance from out_data to mask 0: a multiple of 8 behind the tags");
      if (t.buf2_len % 8 != 0 || t.buf2_len < 8 * words) fail("UNION needs buf2_len = distance between masks: a multiple of 8, at least 8 ceil(nrows / 64)");
      if (t.flags > 1) fail("UNION parents are structs (flags 0 or 1)");
      if (t.sel != nullptr) fail("UNION tasks cannot be decoded through a selection vector");
      break;
    }
    case MI_K_UNION_DENSE:
      if (t.param != 1 && t.param != 2 && t.param != 4 && t.param != 8 && t.param != 16) fail("UNION_DENSE width must be 1,2,4,8,16");
      if (reinterpret_cast<uintptr_t>(t.buf1) % 4 != 0) fail("UNION_DENSE offsets misaligned");
      if (t.buf2 == nullptr || reinterpret_cast<uintptr_t>(t.buf2) % 16 != 0) fail("UNION_DENSE needs the member's decoded vector (16-byte aligned) in buf2");
      if (t.buf2_len < 0) fail("UNION_DENSE needs buf2_len = rows of the member's vector");
      if (t.out_aux == nullptr || reinterpret_cast<uintptr_t>(t.out_aux) % 8 != 0) fail("UNION_DENSE needs the member's mask (8-byte aligned) in out_aux");
      if (t.flags > 1) fail("UNION_DENSE masks have the union's row numbering (flags 0 or 1)");
      if (t.sel != nullptr) fail("UNION_DENSE tasks cannot be decoded through a selection vector");
      break;
    case MI_K_ENC_COPY:
      if (t.param != 1 && t.param != 2 && t.param != 4 && t.param != 8 && t.param != 16) fail("ENC_COPY width must be 1,2,4,8,16");
      break;
    case MI_K_ENC_DEC128:
      if (t.param != 2 && t.param != 4 && t.param != 8) fail("ENC_DEC128 in width must be 2,4,8");
      break;
    case MI_K_ENC_STR32:
    case MI_K_ENC_STRVIEW:
      if (t.out_aux == nullptr) fail("out_aux (string data) is NULL");
      if (reinterpret_cast<uintptr_t>(t.buf1) % 16 != 0) fail("string_t vector must be 16-byte aligned");
      break;
    case MI_K_ENC_LIST32:
      if (reinterpret_cast<uintptr_t>(t.buf1) % 16 != 0) fail("list_entry_t vector must be 16-byte aligned");
      break;
    case MI_K_ENC_UUID_TEXT:
      if (t.out_aux == nullptr) fail("out_aux (string data) is NULL");
      if (reinterpret_cast<uintptr_t>(t.buf1) % 16 != 0) fail("UUID vector must be 16-byte aligned");
      if (reinterpret_cast<uintptr_t>(t.out_aux) % 16 != 0) fail("string data buffer must be 16-byte aligned");
      if (reinterpret_cast<uintptr_t>(t.out_data) % 8 != 0) fail("offsets buffer misaligned");
      if (t.nrows > 0x7FFFFFFFll) fail("more than INT32_MAX rows");
      break;
    case MI_K_ENC_INTERVAL:
      if (reinterpret_cast<uintptr_t>(t.buf1) % 16 != 0) fail("interval_t vector must be 16-byte aligned");
      break;
    case MI_K_ENC_UNION: {
      const int64_t words = (t.nrows + 63) / 64;
      if (t.param < 1 || t.param > MI_MAX_UNION_MEMBERS) fail("ENC_UNION needs param = number of members, 1 .. " + std::to_string(MI_MAX_UNION_MEMBERS));
      if (t.buf2 == nullptr || reinterpret_cast<uintptr_t>(t.buf2) % 8 != 0) fail("ENC_UNION needs the members' validity addresses (8-byte aligned) in buf2");
      if (t.out_aux == nullptr || reinterpret_cast<uintptr_t>(t.out_aux) % 8 != 0) fail("ENC_UNION needs the masks (8-byte aligned) in out_aux");
      if (t.buf2_len % 8 != 0 || t.buf2_len < 8 * words) fail("ENC_UNION needs buf2_len = distance between masks: a multiple of 8, at least 8 ceil(nrows / 64)");
      if (t.ptr_base % 8 != 0) fail("ENC_UNION parent words misaligned");
      break;
    }
    default: break;
  }
  if (t.kind >= MI_K_ENC_COPY && t.kind != MI_K_ENC_COPY && t.kind != MI_K_ENC_UNION && t.out_validity == nullptr)
    fail("encode tasks need out_validity (the bitmap is always emitted; only a bare ENC_COPY of list offsets has none)");
}

static int64_t TaskBytesRead(const mi_col_task& t) {
  const int64_t n = t.nrows;
  int64_t b = 0;
  if (t.kind == MI_K_RUN_END) {  // run ends + every run's value and validity bit once (+ the parent's words)
    b = t.param2 * ((t.param & 0xFF) + ((t.param >> 8) & 0xFF)) + (t.validity ? ((t.param2 + 63) / 64) * 8 : 0);
    return b + (t.out_aux ? ((n + 63) / 64) * 8 : 0);
  }
  if (t.kind == MI_K_UNION)   // type ids, dense offsets, the parent's words (member bitmaps: a bit per row at most, not counted)
    return n * (t.ptr_base ? 5 : 1) + (t.out_aux ? ((n + 63) / 64) * 8 : 0);
  if (t.kind == MI_K_UNION_DENSE)   // offsets, the mask, and every value of the member once at most
    return n * 4 + ((n + 63) / 64) * 8 + std::min(n, t.buf2_len) * t.param;
  if (t.kind < MI_K_ENC_COPY) {
    if (t.validity && t.null_count != 0) b += (n + 7) / 8;
    switch (t.kind) {
      case MI_K_COPY: case MI_K_FIXED_BINARY: b += n * t.param; break;
      case MI_K_BOOL: b += (n + 7) / 8; break;
      case MI_K_DEC128: b += n * 16; break;
      case MI_K_DATE64: case MI_K_MUL_I64: case MI_K_DIV_I64: case MI_K_DURATION: b += n * 8; break;
      case MI_K_MUL_I32: b += n * 4; break;
      case MI_K_STR32: b += (n ? (n + 1) * 4 : 0) + t.buf2_len; break;
      case MI_K_STR64: b += (n ? (n + 1) * 8 : 0) + t.buf2_len; break;
      case MI_K_DICT: b += n * (t.param & 0xFF); break;
      case MI_K_INTERVAL_MONTHS: b += n * 4; break;
      case MI_K_INTERVAL_MDN: case MI_K_UUID: b += n * 16; break;
      case MI_K_BOOL8: b += n; break;
      case MI_K_NARROW: b += n * (t.param & 0xFF); break;
      case MI_K_HALF_FLOAT: b += n * 2; break;
      case MI_K_LIST32: b += n ? (n + 1) * 4 : 0; break;
      case MI_K_LIST64: b += n ? (n + 1) * 8 : 0; break;
      case MI_K_STRVIEW: b += n * 16; break;
      default: break;
    }
    if (t.out_aux) b += ((n + 63) / 64) * 8;
  } else {
    if (t.validity) b += ((n + 63) / 64) * 8;
    switch (t.kind) {
      case MI_K_ENC_COPY: case MI_K_ENC_DEC128: b += n * t.param; break;
      case MI_K_ENC_BOOL: b += n; break;
      case MI_K_ENC_UNION: b += n + (t.param + (t.ptr_base ? 1 : 0)) * ((n + 63) / 64) * 8; break;   // tags; member (at most) and parent words
      case MI_K_ENC_STR32: case MI_K_ENC_LIST32: case MI_K_ENC_STRVIEW: case MI_K_ENC_UUID_TEXT: case MI_K_ENC_INTERVAL: b += n * 16; break;  // + payload, known only after the scan (reported via buf2_len if given)
      default: break;
    }
    if (t.kind == MI_K_ENC_STR32 || t.kind == MI_K_ENC_STRVIEW) b += t.buf2_len;   // (views: the long strings alone)
  }
  return b;
}

static int64_t TaskBytesWritten(const mi_col_task& t) {
  const int64_t n = t.nrows;
  if (t.kind < MI_K_ENC_COPY) {
    return n * device::OutWidth(t.kind, t.param) + ((t.out_validity ? 1 : 0) + (t.kind == MI_K_UNION ? t.param : 0)) * ((n + 63) / 64) * 8;
  }
  if (t.kind == MI_K_ENC_UNION) return n + t.param * ((n + 63) / 64) * 8;   // type ids and the masks; no bitmap
  int64_t b = t.out_validity ? (n + 7) / 8 : 0;  // bitmap
  switch (t.kind) {
    case MI_K_ENC_COPY: b += n * t.param; break;
    case MI_K_ENC_DEC128: case MI_K_ENC_INTERVAL: b += n * 16; break;
    case MI_K_ENC_BOOL: b += (n + 7) / 8; break;
    case MI_K_ENC_STR32: case MI_K_ENC_UUID_TEXT: b += (n + 1) * ((t.flags & 1) ? 8 : 4) + t.buf2_len; break;   // (buf2_len: the text bytes)
    case MI_K_ENC_LIST32: b += (n + 1) * ((t.flags & 1) ? 8 : 4); break;
    case MI_K_ENC_STRVIEW: b += n * 16 + t.buf2_len; break;
    default: break;
  }
  return b;
}

void LayOutPlan(const mi_col_task* in_tasks, int32_t n_tasks, PlanLayout* out) {
  PlanLayout& p = *out;
  p.tasks.clear();
  p.order.clear();
  p.tile_begin.clear();
  p.tile_task.clear();
  p.slices.clear();
  p.total_tiles = 0;
  p.bytes_read = p.bytes_written = p.rows = 0;
  for (int c = 0; c < device::kNumClasses; c++) p.class_tiles[c] = 0, p.class_bytes_read[c] = p.class_bytes_written[c] = p.class_rows[c] = 0;
  p.is_encode = false;
  p.n_null_counts = 0;
  int max_depth = 0;
  std::vector<mi_col_task> staged;
  std::vector<int> staged_slot;
  for (int32_t i = 0; i < n_tasks; i++) {
    ValidateTask(in_tasks[i], static_cast<size_t>(i));
    mi_col_task t = in_tasks[i];
    const int slot = device::SlotOfTask(t), cls = device::kSlots[slot].cls;
    if (t.kind >= MI_K_ENC_COPY) {
      p.is_encode = true;
      t.depth = 0;
      t.param2 = p.n_null_counts++;  // slot of this task's NULL counter
    }
    const int64_t r = TaskBytesRead(t), w = TaskBytesWritten(t);
    p.bytes_read += r;
    p.bytes_written += w;
    p.rows += t.nrows;
    p.class_bytes_read[cls] += r;
    p.class_bytes_written[cls] += w;
    p.class_rows[cls] += t.nrows;
    max_depth = std::max(max_depth, t.depth);
    staged.push_back(t);
    staged_slot.push_back(slot);
  }
  p.order.assign(static_cast<size_t>(n_tasks), {0, 0});
  // one slice per (pass, depth, position) that has tasks, in that order (device::kSlots says why); stable inside a slice
  for (int pass = 0; pass < device::kNumPasses; pass++)
  for (int depth = 0; depth <= max_depth; depth++)
  for (int pos = 0, slot; (slot = device::SlotAt(pass, pos)) >= 0; pos++) {
    ClassSlice sl;
    sl.slot = static_cast<device::LaunchSlot>(slot);
    sl.depth = depth;
    sl.first_task = static_cast<int32_t>(p.tasks.size());
    sl.tile_begin_at = static_cast<int32_t>(p.tile_begin.size());
    sl.tile_task_at = p.tile_task.size();
    const int64_t tile_rows = device::kSlots[slot].tile_rows;
    uint64_t tiles = 0;
    uint32_t local_task = 0;
    for (size_t i = 0; i < staged.size(); i++) {
      if (staged_slot[i] != slot || staged[i].depth != depth) continue;
      const mi_col_task& t = staged[i];
      p.tile_begin.push_back(static_cast<uint32_t>(tiles));
      const uint64_t nt = static_cast<uint64_t>((t.nrows + tile_rows - 1) / tile_rows);
      tiles += nt;
      if (tiles > 0xFFFFFFF0ull) throw InvalidInputException("plan has too many tiles");
      p.tile_task.insert(p.tile_task.end(), static_cast<size_t>(nt), local_task);
      sl.kernel_mask |= device::KernelMaskOfTask(slot, t);
      p.order[i] = {static_cast<int>(p.slices.size()), static_cast<int32_t>(local_task)};
      local_task++;
      p.tasks.push_back(t);
    }
    if (local_task == 0) continue;
    p.tile_begin.push_back(static_cast<uint32_t>(tiles));
    sl.n_tasks = static_cast<int32_t>(local_task);
    sl.total_tiles = static_cast<uint32_t>(tiles);
    p.total_tiles += sl.total_tiles;
    p.class_tiles[device::kSlots[slot].cls] += sl.total_tiles;
    p.slices.push_back(sl);
  }
}

std::vector<int64_t> PlanLayout::MapNullCounts(const int64_t* per_slot) const {
  // back to the caller's task order (non-encode tasks report 0)
  std::vector<int64_t> out(order.size(), 0);
  for (size_t i = 0; i < order.size(); i++) {
    const mi_col_task& t = tasks[static_cast<size_t>(slices[static_cast<size_t>(order[i].first)].first_task + order[i].second)];
    if (t.kind >= MI_K_ENC_COPY) out[i] = per_slot[static_cast<size_t>(t.param2)];
  }
  return out;
}

}  // namespace miarrow
