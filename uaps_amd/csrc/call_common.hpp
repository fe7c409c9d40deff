// What every entry point of the library may use, whatever it computes: the launch scaffold (block size, grid rule, the 2 GiB refusal,
// the alignment rule of the four-pixel form), the one statement of how a size-versioned *_call record is read, and the rules of a
// caller-owned workspace and of a class selection.  Host code and constants only: no kernel lives here.  The dispatch on C and on V,
// the fused-loss reduction and the per-pixel softmax helpers are loss_common.hpp's, which builds on this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/uaps_hip.h"
#include "hints.hpp"                           // UAPS_LAUNCH_MAIN, account_bytes

namespace uaps {
typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kTooBig = 2147483648.0;       // bytes: every tensor an entry point takes stays below 2 GiB

// one block per kThreads items, at least one and at most `cap` (the lanes stride over the rest)
inline int grid_for(long items, int cap) { const long g = (items + kThreads - 1) / kThreads; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }
// the four-pixel form needs 16-byte aligned float / int64 pointers and 4-byte aligned pseudo-label bytes
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The size-versioned copy rule of every *_call record: NULL or a struct_size below the first version's is refused; `out` is zeroed
// and receives the first version's v1_bytes alone -- what a later header appends is not read.  UAPS_EINVAL or UAPS_OK.
template <class T>
inline int read_call(const T* call, size_t v1_bytes, T& out) {
    if (!call || call->struct_size < v1_bytes) return UAPS_EINVAL;
    memset(&out, 0, sizeof out);
    memcpy(&out, call, v1_bytes);
    return UAPS_OK;
}
// the same for a record whose first version ends behind `stream` (every one so far)
template <class T>
inline int read_call(const T* call, T& out) { return read_call(call, offsetof(T, stream) + sizeof(uaps_stream_t), out); }

// sub-buffers of a workspace start on 256-byte boundaries, and so does the workspace
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool workspace_ok(const void* p, size_t have, size_t need) { return have >= need && (reinterpret_cast<uintptr_t>(p) & 255) == 0; }

// the n selected classes are distinct and none is the background
template <class T>
inline bool distinct_classes(const T* classes, int n, T background) {
    for (int k = 0; k < n; ++k) {
        if (classes[k] == background) return false;
        for (int j = 0; j < k; ++j)
            if (classes[j] == classes[k]) return false;
    }
    return true;
}
}  // namespace uaps
