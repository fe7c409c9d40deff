// The launch sequence of uaps_label_instances (instances.hip) for callers inside the library: split.hip numbers and tabulates the
// pieces of its code map with the very launches label_instances runs on a class mask.
#pragma once
#include "call_common.hpp"

namespace uaps {
// what label_launches needs behind c.workspace (256-byte aligned): uaps_instances_workspace_bytes without its checks
size_t label_workspace_bytes(int B, int H, int W);
// Zeroes the table and enqueues the seven launches on c.stream; no host synchronisation.  The caller has checked every field the way
// uaps_label_instances does.  Returns hipGetLastError().
int label_launches(const uaps_instances_call& c);
}  // namespace uaps
