// plan_layout.hpp -- what a transcode plan launches, worked out on the host without a device: the tasks validated and grouped
// into slices in launch order, the tile tables the kernels index, and the statistics.  Plan (engine.hpp) uploads it and launches.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "task_kind.hpp"

namespace miarrow {

// The tasks of one (slot, depth): one launch of the slot's kernels.
struct ClassSlice {
  device::LaunchSlot slot{};  // what launches it (a device::KernelClass value for the class kernels); device::kSlots[slot].cls accounts for it
  int32_t depth = 0;          // nesting depth of the tasks in this slice
  size_t tile_task_at = 0;    // index into PlanLayout::tile_task / d_tile_task
  int32_t first_task = 0;     // index into PlanLayout::tasks / d_tasks
  int32_t n_tasks = 0;
  int32_t tile_begin_at = 0;  // index into PlanLayout::tile_begin / d_tile_begin (n_tasks + 1 entries)
  uint32_t total_tiles = 0;
  uint32_t kernel_mask = 0;   // which kernels of the slot have tiles: device::KernelMaskOfTask over the tasks
};

// A plan = any number of (record batch, column) tasks, grouped by launch slot and nesting depth; every slice is one launch
// (lineitem: copy + dec128 + string = 3 launches for the whole table, however many batches).  A slot with a kernel of its own
// is accounted under a class (class_*, LaunchTimed): run-end and unions under misc, string views under enc_string, so a plan
// that has both adds encode_string_view to encode_string_1p's line -- time a kernel alone with a plan of its tasks alone.
struct PlanLayout {
  std::vector<mi_col_task> tasks;                 // slice by slice; encode tasks with depth 0 and param2 = their NULL-counter slot
  std::vector<std::pair<int, int32_t>> order;     // caller order -> (index into slices, index inside the slice)
  std::vector<uint32_t> tile_begin;               // per slice: first tile of every task, then the slice's tile count
  std::vector<uint32_t> tile_task;                // per slice: task index (within the slice) of every tile
  std::vector<ClassSlice> slices;                 // launch order: device::kSlots, pass by pass, depth by depth
  uint32_t class_tiles[device::kNumClasses] = {0};
  uint32_t total_tiles = 0;
  int64_t n_null_counts = 0;                      // encode tasks: one NULL counter each, in caller order
  bool is_encode = false;
  int64_t bytes_read = 0, bytes_written = 0, rows = 0;
  int64_t class_bytes_read[device::kNumClasses] = {0}, class_bytes_written[device::kNumClasses] = {0},
          class_rows[device::kNumClasses] = {0};

  //! per_slot = a host copy of the NULL counters (n_null_counts entries) -> NULL counts in the caller's task order
  std::vector<int64_t> MapNullCounts(const int64_t* per_slot) const;
};

//! Validates the tasks (InvalidInputException "task <i>: ...") and fills `out`, whose vectors keep their capacity and nothing else.
void LayOutPlan(const mi_col_task* tasks, int32_t n_tasks, PlanLayout* out);
inline PlanLayout LayOutPlan(const mi_col_task* tasks, int32_t n_tasks) {
  PlanLayout out;
  LayOutPlan(tasks, n_tasks, &out);
  return out;
}

}  // namespace miarrow
