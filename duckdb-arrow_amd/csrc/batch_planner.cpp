// batch_planner.cpp -- see batch_planner.hpp.
#include "batch_planner.hpp"

#include <algorithm>
#include <cstring>

#include "union_format.hpp"

namespace miarrow {

namespace {
size_t RoundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }
void* OffsetHandle(int64_t off) { return reinterpret_cast<void*>(static_cast<uintptr_t>(off >= 0 ? off + 1 : 0)); }
}  // namespace

void BatchPlanner::Clear() {
  nodes.clear();
  tasks.clear();
  aux.clear();
  upload.clear();
  aux_fixups.clear();
  value_fixups.clear();
  arena_bytes = 0;
}

size_t BatchPlanner::Reserve(size_t bytes) {
  const size_t at = arena_bytes;
  arena_bytes += RoundUp(bytes, 256);
  return at;
}

// Every output array starts on an `array_align` boundary of the arena.  Measured on MI355X with fresh processes on one box
// (SF10 lineitem resident in HBM, ms per step): 256 B alignment 3.39-3.43, 4 KiB 3.39, 64 KiB 3.34-3.36, 2 MiB 3.40 -- the
// copy and dec128 kernels gain 2-3 % when a 16 KB tile never straddles a 64 KiB page fragment; that costs ~32 KiB of
// padding per (batch, column), 0.5 GB of 288 GB at SF10.  The scan operator's slots (PCIe bound) stay at 256 B.
void BatchPlanner::Alloc(int64_t rows, int32_t width, bool with_validity, size_t* data_off, int64_t* valid_off) {
  const size_t a = std::max<size_t>(opts.array_align, 256);
  *data_off = arena_bytes;
  arena_bytes += RoundUp(static_cast<size_t>(rows) * static_cast<size_t>(std::max(width, 1)) + 16, a);
  *valid_off = -1;
  if (with_validity) {
    *valid_off = static_cast<int64_t>(arena_bytes);
    arena_bytes += RoundUp(static_cast<size_t>((rows + 63) / 64) * 8 + 8, rows >= 65536 ? a : 256);
  }
}

std::pair<size_t, size_t> BatchPlanner::AddAbsentColumn(int64_t n, int32_t width) {
  size_t d;
  int64_t v;
  Alloc(n, width, true, &d, &v);
  return {d, static_cast<size_t>(v)};
}

int32_t BatchPlanner::AddColumn(const BatchPlacement& where, int32_t decoded_node, int64_t extra_rows) {
  const int64_t n = where.batch->nodes[static_cast<size_t>(decoded_node)].length;
  std::vector<int64_t> win;
  for (int64_t r = 0; r < n; r += MI_VECTOR_SIZE) win.push_back(r);
  win.push_back(n);
  if (n == 0) win.push_back(0);
  return AddNode(where, decoded_node, std::move(win), true, -1, 0, -1, extra_rows);
}

// One field node (and, recursively, its children): output slots + the transcode task.
// `win` = first row of every top-level 2048-row chunk window in this node's row space (+ the end): top-level columns and
// struct children of them have win[k] = 2048k (the tiles themselves); the child of a list starts its window k at
// offsets[win[k]], the child of a fixed_size_list at size * win[k].
int32_t BatchPlanner::AddNode(const BatchPlacement& where, int32_t ni, std::vector<int64_t> win, bool win_is_tiles,
                              int64_t parent_valid_off, int32_t parent_div, int32_t parent, int64_t extra_rows) {
  const DecodedBatch& b = *where.batch;
  const DecodedNode& nd = b.nodes[static_cast<size_t>(ni)];
  int32_t kind, w;
  int64_t param;
  if (!nd.field->Plan(&kind, &param, &w, nd.value_only))
    throw NotImplementedException("Arrow type " + nd.field->Format() + " of field '" + nd.field->name + "' is not decoded by the MI355X scan path");
  const int64_t n = nd.length;
  if (kind == MI_K_RUN_END) {
    // a list's child vector is cut into windows per chunk: runs would have to be split at them (DuckDB refuses it too)
    for (int32_t a = parent; a >= 0; a = nodes[static_cast<size_t>(a)].parent) {
      const int32_t at = nodes[static_cast<size_t>(a)].arrow_type;
      if (at == MI_AT_LIST || at == MI_AT_LARGE_LIST || at == MI_AT_MAP || at == MI_AT_FIXED_LIST)
        throw NotImplementedException("Column '" + nd.field->name + "': run-end encoded arrays inside a list / map / fixed_size_list are not decoded by the MI355X scan path");
    }
    if (nd.children.size() != 2) throw InternalException("run-end encoded field without exactly two children");
  }
  if (kind == MI_K_UNION) {
    // the members take their NULLs from masks in the union's row numbering (Supported() refuses these at bind already)
    for (int32_t a = parent; a >= 0; a = nodes[static_cast<size_t>(a)].parent) {
      const int32_t at = nodes[static_cast<size_t>(a)].arrow_type;
      if (at == MI_AT_LIST || at == MI_AT_LARGE_LIST || at == MI_AT_MAP || at == MI_AT_FIXED_LIST || at == MI_AT_RUN_END)
        throw NotImplementedException("Column '" + nd.field->name + "': unions inside a list / map / fixed_size_list / run-end encoded array are not decoded by the MI355X scan path");
    }
    if (nd.children.size() != nd.field->children.size() || nd.children.empty() || nd.children.size() > MI_MAX_UNION_MEMBERS)
      throw InternalException("union field whose nodes do not match its members");
  }
  const DecodedNode* ree_values = kind == MI_K_RUN_END ? &b.nodes[static_cast<size_t>(nd.children[1])] : nullptr;
  // values of a run-end array, member array of a dense union: decoded in their own row space, expanded by index afterwards
  const bool scratch = parent >= 0 && (nodes[static_cast<size_t>(parent)].kind == MI_K_RUN_END || nodes[static_cast<size_t>(parent)].kind == MI_K_UNION_DENSE);
  const int32_t idx = static_cast<int32_t>(nodes.size());
  nodes.emplace_back();
  auto span = [&](size_t k) { return k < nd.spans.size() ? nd.spans[k] : mi_buffer_span{0, 0}; };
  {
    PlannedNode& o = nodes.back();
    o.kind = kind;
    o.width = w;
    o.param = param;
    o.nrows = n;
    o.null_count = nd.null_count;
    o.arrow_type = nd.field->type;
    o.depth = nd.depth;
    o.parent = parent;
    o.win = win;
    o.source_node = ni;
    // reference behaviour for plain fixed-width columns: the vector aliases the Arrow buffer (DirectConversion) and an
    // array without NULLs leaves the ValidityMask unset
    if (opts.zero_copy_direct && kind == MI_K_COPY && nd.null_count == 0 && parent_valid_off < 0 && nd.spans.size() > 1 && !scratch &&
        !(where.no_alias && (*where.no_alias)[static_cast<size_t>(ni)]) && extra_rows == 0 && where.alloc_rows < 0) {
      o.alias_body_off = nd.spans[1].offset;
      return idx;
    }
    // a run-end array's NULLs are its values' NULLs
    int64_t nulls = ree_values ? ree_values->null_count : nd.null_count;
    if (kind == MI_K_UNION) {  // ... and a union's are its members': without a bitmap that can clear a bit every row is valid
      nulls = 0;
      for (int32_t cn : nd.children) {
        const DecodedNode& m = b.nodes[static_cast<size_t>(cn)];
        if (m.null_count != 0 || m.field->type == MI_AT_NULL) nulls = -1;
      }
      o.null_count = nulls;
    }
    const bool all_valid = opts.unset_all_valid && nulls == 0 && parent_valid_off < 0 && extra_rows == 0 && kind != MI_K_NULL;
    Alloc((where.alloc_rows >= 0 && nd.depth == 0 ? where.alloc_rows : n) + extra_rows, w, !all_valid, &o.data_off, &o.valid_off);
  }
  for (const auto& sp : nd.spans)
    if (sp.length > 0) upload.emplace_back(sp.offset, sp.length);
  const size_t data_off = nodes[static_cast<size_t>(idx)].data_off;
  const int64_t valid_off = nodes[static_cast<size_t>(idx)].valid_off;
  auto consumer_addr = [&](int64_t body_offset) { return where.consumer_base + static_cast<uint64_t>(body_offset); };
  mi_col_task t;
  std::memset(&t, 0, sizeof(t));
  t.out_data = OffsetHandle(static_cast<int64_t>(data_off));
  t.out_validity = OffsetHandle(valid_off);
  t.out_aux = OffsetHandle(parent_valid_off);
  t.flags = parent_div;
  t.depth = nd.depth;
  t.validity = span(0).length ? where.in_base + span(0).offset : nullptr;
  t.buf1 = nd.spans.size() > 1 ? where.in_base + span(1).offset : where.in_base;
  t.nrows = n;
  t.null_count = nd.null_count;
  t.kind = kind;
  t.param = param;
  std::vector<int64_t> child_win;
  int64_t aux_at = -1;
  switch (kind) {
    case MI_K_STR32: case MI_K_STR64:
      t.buf2 = where.in_base + span(2).offset;
      t.buf2_len = span(2).length;
      t.ptr_base = consumer_addr(span(2).offset);
      break;
    case MI_K_FIXED_BINARY:
      t.ptr_base = consumer_addr(span(1).offset);
      break;
    case MI_K_STRVIEW: {
      aux_at = static_cast<int64_t>(aux.size());
      for (size_t k = 2; k < nd.spans.size(); k++) {
        aux.push_back(consumer_addr(nd.spans[k].offset));
        aux.push_back(static_cast<uint64_t>(nd.spans[k].length));
      }
      if (nd.spans.size() <= 2) { aux.push_back(0); aux.push_back(0); }
      t.buf2_len = static_cast<int64_t>(nd.spans.size() > 2 ? nd.spans.size() - 2 : 0);
      break;
    }
    case MI_K_DICT: {
      if (!where.dict_len) throw InternalException("dictionary-encoded column without a dictionary resolver");
      nodes[static_cast<size_t>(idx)].dict_id = nd.field->dict_id;
      t.param2 = where.dict_len(nd.field->dict_id);
      break;
    }
    case MI_K_RUN_END: {
      // the values child decodes into a scratch vector of its own row space (one row per run) in an earlier slice of the plan
      const DecodedNode& re = b.nodes[static_cast<size_t>(nd.children[0])];
      const int64_t n_runs = re.length;
      std::vector<int64_t> vwin;
      for (int64_t r = 0; r < n_runs; r += MI_VECTOR_SIZE) vwin.push_back(r);
      vwin.push_back(n_runs);
      const int32_t vi = AddNode(where, nd.children[1], std::move(vwin), true, -1, 0, idx, 0);
      const PlannedNode& v = nodes[static_cast<size_t>(vi)];
      for (const auto& sp : re.spans)
        if (sp.length > 0) upload.emplace_back(sp.offset, sp.length);
      t.validity = nullptr;
      t.null_count = 0;
      if (v.valid_off >= 0 && v.null_count != 0) {
        t.validity = OffsetHandle(v.valid_off);
        t.null_count = v.null_count;
      }
      t.buf1 = where.in_base + (re.spans.size() > 1 ? re.spans[1].offset : 0);
      t.buf2 = OffsetHandle(static_cast<int64_t>(v.data_off));
      t.buf2_len = v.nrows;
      t.param2 = n_runs;
      t.ptr_base = v.ptr_base;
      PlannedNode& o = nodes[static_cast<size_t>(idx)];
      o.value_kind = v.kind;
      o.null_count = v.null_count;
      o.heap_size = v.heap_size;
      break;
    }
    case MI_K_UNION: {
      // tags in the node's data array; behind it one mask per member, each followed by a spare word
      const size_t m = nd.children.size();
      const bool dense = nd.field->unit == 1;
      const size_t stride = static_cast<size_t>((n + 63) / 64) * 8 + 8;
      const size_t mask_off = Reserve(m * stride);
      nodes[static_cast<size_t>(idx)].mask_off = static_cast<int64_t>(mask_off);
      nodes[static_cast<size_t>(idx)].mask_stride = static_cast<int64_t>(stride);
      t.validity = nullptr;
      t.null_count = 0;
      t.buf1 = where.in_base + span(0).offset;
      t.ptr_base = dense ? reinterpret_cast<uint64_t>(where.in_base + span(1).offset) : 0;
      t.param2 = static_cast<int64_t>(mask_off) - static_cast<int64_t>(data_off);
      t.buf2_len = static_cast<int64_t>(stride);
      // the union table (mi_arrow_ipc.h: MI_K_UNION)
      int8_t table[unionfmt::kTableEntries];
      const ArrowField& uf = *nd.field;
      unionfmt::BuildTable(uf.type_ids.data(), uf.has_type_ids ? static_cast<int>(uf.type_ids.size()) : -1, static_cast<int>(m), table);
      aux_at = static_cast<int64_t>(aux.size());
      aux.resize(aux.size() + unionfmt::kTableWords);
      std::memcpy(&aux[static_cast<size_t>(aux_at)], table, sizeof(table));
      for (int32_t cn : nd.children) {
        const DecodedNode& mn = b.nodes[static_cast<size_t>(cn)];
        const bool null_type = mn.field->type == MI_AT_NULL;
        const bool bitmap = !null_type && !mn.spans.empty() && mn.spans[0].length > 0;
        aux.push_back(bitmap ? reinterpret_cast<uint64_t>(where.in_base + mn.spans[0].offset) : 0);
        aux.push_back(static_cast<uint64_t>(mn.length));
        aux.push_back(static_cast<uint64_t>(bitmap ? mn.null_count : 0));
        aux.push_back(null_type ? unionfmt::kMemberNullType : 0);
      }
      break;
    }
    case MI_K_LIST32: case MI_K_LIST64: {
      if (nd.children.size() != 1) throw InternalException("list field without exactly one child");
      t.param = b.nodes[static_cast<size_t>(nd.children[0])].length;
      if (!win_is_tiles) {
        aux_at = static_cast<int64_t>(aux.size());
        for (int64_t r : win) aux.push_back(static_cast<uint64_t>(r));
        t.buf2_len = static_cast<int64_t>(win.size());
      }
      // the child's windows start at offsets[win[k]] (read from the host copy of the body)
      const uint8_t* offs = b.body + span(1).offset;
      child_win.reserve(win.size());
      int64_t prev = 0;
      for (int64_t r : win) {
        int64_t v = 0;
        if (n > 0) {
          if (r < 0 || r > n) throw InternalException("Arrow IPC validation failed: list window outside the column");
          if (kind == MI_K_LIST32) { int32_t x; std::memcpy(&x, offs + 4 * r, 4); v = x; }
          else std::memcpy(&v, offs + 8 * r, 8);
          // the offsets sampled here place the child vectors of every chunk: they are checked on the host (the device
          // checks all of them, but only flags) so that no window ever points outside the child column
          if (v < prev || v > t.param)
            throw InternalException("Arrow IPC validation failed: offsets buffer is not monotonically non-decreasing or exceeds the data buffer");
          prev = v;
        }
        child_win.push_back(v);
      }
      break;
    }
    default: break;
  }
  nodes[static_cast<size_t>(idx)].ptr_base = kind == MI_K_UNION ? 0 : t.ptr_base;
  if (kind != MI_K_RUN_END && kind != MI_K_UNION) nodes[static_cast<size_t>(idx)].heap_size = kind == MI_K_FIXED_BINARY ? span(1).length : t.buf2_len;
  // a struct without NULLs of its own or of a parent has nothing to compute when its validity stays unset
  const bool has_work = n > 0 && !(kind == MI_K_STRUCT && valid_off < 0);
  if (has_work) {
    if (aux_at >= 0) aux_fixups.emplace_back(tasks.size(), static_cast<size_t>(aux_at));
    if (kind == MI_K_RUN_END) value_fixups.push_back(tasks.size());  // (dense union members: AddUnionChildren)
    nodes[static_cast<size_t>(idx)].task = static_cast<int32_t>(tasks.size());
    tasks.push_back(t);
  }
  if (kind == MI_K_LIST32 || kind == MI_K_LIST64) {
    const int32_t c = AddNode(where, nd.children[0], child_win, false, -1, 0, idx, 0);
    nodes[static_cast<size_t>(idx)].children.push_back(c);
  } else if (kind == MI_K_UNION) {
    AddUnionChildren(where, ni, idx, win, win_is_tiles);
  } else if (kind == MI_K_STRUCT && !nd.children.empty()) {
    const bool fixed = nd.field->type == MI_AT_FIXED_LIST;
    const int64_t size = fixed ? param : 1;
    std::vector<int64_t> cw;
    for (int64_t r : win) cw.push_back(r * size);
    for (int32_t cn : nd.children) {
      const int32_t c = AddNode(where, cn, cw, win_is_tiles && !fixed, valid_off, static_cast<int32_t>(fixed ? size : 1), idx, 0);
      nodes[static_cast<size_t>(idx)].children.push_back(c);
    }
  }
  return idx;
}

// The children of a planned union node, as DuckDB's UNION vector lists them: the tag vector (the union's own data array), then
// one vector per member.  Sparse: the member array itself, a struct child whose parent words are the member's mask.  Dense:
// a vector of the union's length that an MI_K_UNION_DENSE task fills from the member array, which is decoded by its usual
// task into a scratch vector of its own row space (never aliased), as a run-end array's values are.
void BatchPlanner::AddUnionChildren(const BatchPlacement& where, int32_t ni, int32_t idx, const std::vector<int64_t>& win, bool win_is_tiles) {
  const DecodedBatch& b = *where.batch;
  const DecodedNode& nd = b.nodes[static_cast<size_t>(ni)];
  const bool dense = nd.field->unit == 1;
  const int64_t n = nd.length;
  const PlannedNode u = nodes[static_cast<size_t>(idx)];  // (a copy: `nodes` grows below)
  {
    const int32_t ti = static_cast<int32_t>(nodes.size());
    nodes.emplace_back();
    PlannedNode& tag = nodes.back();
    tag.synth = 1;
    tag.kind = MI_K_COPY;
    tag.width = 1;
    tag.param = 1;
    tag.arrow_type = MI_AT_INT;
    tag.nrows = n;
    tag.depth = u.depth + 1;
    tag.parent = idx;
    tag.win = win;
    tag.source_node = ni;
    tag.data_off = u.data_off;
    nodes[static_cast<size_t>(idx)].children.push_back(ti);
  }
  for (size_t k = 0; k < nd.children.size(); k++) {
    const int64_t mask = u.mask_off + static_cast<int64_t>(k) * u.mask_stride;
    if (!dense) {
      const int32_t c = AddNode(where, nd.children[k], win, win_is_tiles, mask, 1, idx, 0);
      nodes[static_cast<size_t>(idx)].children.push_back(c);
      continue;
    }
    const DecodedNode& mn = b.nodes[static_cast<size_t>(nd.children[k])];
    int32_t mk, mw;
    int64_t mp;
    if (!mn.field->Plan(&mk, &mp, &mw)) throw InternalException("dense union member without a decode kind");
    const int32_t di = static_cast<int32_t>(nodes.size());
    nodes.emplace_back();
    {
      PlannedNode& d = nodes.back();
      d.synth = 2;
      d.kind = MI_K_UNION_DENSE;
      d.value_kind = mk;
      d.width = mw;
      d.param = mw;
      d.arrow_type = mn.field->type;
      d.nrows = n;
      d.null_count = -1;
      d.depth = u.depth + 1;
      d.parent = idx;
      d.win = win;
      d.source_node = nd.children[k];
      Alloc(n, mw, true, &d.data_off, &d.valid_off);
    }
    nodes[static_cast<size_t>(idx)].children.push_back(di);
    std::vector<int64_t> vwin;
    for (int64_t r = 0; r < mn.length; r += MI_VECTOR_SIZE) vwin.push_back(r);
    vwin.push_back(mn.length);
    if (mn.length == 0) vwin.push_back(0);
    const int32_t vi = AddNode(where, nd.children[k], std::move(vwin), true, -1, 0, di, 0);
    const PlannedNode& v = nodes[static_cast<size_t>(vi)];
    PlannedNode& d = nodes[static_cast<size_t>(di)];
    d.ptr_base = v.ptr_base;
    d.heap_size = v.heap_size;
    if (n == 0) continue;
    mi_col_task t;
    std::memset(&t, 0, sizeof(t));
    t.kind = MI_K_UNION_DENSE;
    t.nrows = n;
    t.depth = d.depth;
    t.param = mw;
    t.flags = 1;
    t.buf1 = where.in_base + nd.spans[1].offset;
    t.buf2 = OffsetHandle(static_cast<int64_t>(v.data_off));
    t.buf2_len = v.nrows;
    if (v.valid_off >= 0 && v.null_count != 0) {
      t.validity = OffsetHandle(v.valid_off);
      t.null_count = v.null_count;
    }
    t.ptr_base = v.ptr_base;
    t.out_data = OffsetHandle(static_cast<int64_t>(d.data_off));
    t.out_validity = OffsetHandle(d.valid_off);
    t.out_aux = OffsetHandle(mask);
    value_fixups.push_back(tasks.size());
    d.task = static_cast<int32_t>(tasks.size());
    tasks.push_back(t);
  }
}

void BatchPlanner::Rebase(size_t first_task, uint8_t* arena_base, const uint8_t* aux_base) {
  auto addr = [&](void* handle) -> void* {
    const uintptr_t h = reinterpret_cast<uintptr_t>(handle);
    return h ? arena_base + (h - 1) : nullptr;
  };
  for (size_t i = first_task; i < tasks.size(); i++) {
    mi_col_task& t = tasks[i];
    t.out_data = addr(t.out_data);
    t.out_validity = addr(t.out_validity);
    t.out_aux = addr(t.out_aux);
  }
  for (auto& fx : aux_fixups)
    if (fx.first >= first_task) tasks[fx.first].buf2 = aux_base + fx.second * 8;
  for (size_t i : value_fixups)
    if (i >= first_task) {
      tasks[i].buf2 = addr(const_cast<void*>(tasks[i].buf2));
      tasks[i].validity = addr(const_cast<void*>(tasks[i].validity));
    }
}

}  // namespace miarrow
