// Internal to the K2 probe source (hdp_probe.hip: split / sweep paths, native queue): what needs HIP.
// The plain structs, constants and host planning of the sweep are in hdp_sweep_plan.h (no HIP).
// Not part of the C-ABI.
#pragma once

#include <vector>

#include "hdp_common.h"
#include "hdp_sweep_plan.h"

namespace hdp {

constexpr int kTileLd = 72;          // padded LDS row (floats) of the PROJ transpose tiles

// pinned staging ring -> device table region, stream-ordered (hdp_probe.hip)
int probe_tables_upload(const std::vector<char>& blob, void* dst, hipStream_t st);

}  // namespace hdp
