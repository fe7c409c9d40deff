// One convolution call as the entry points of conv_fwd.hip / conv_wrw.hip / conv_ex.hip hand it on: everything that decides
// which kernel runs (shape, cfg, the pointers whose alignment matters, the optional operands) in one place.
#pragma once
#include <stddef.h>
#include "../../include/uaps_hip.h"

namespace uaps {

// forward / input gradient: x [B,Cin,H,W] * packed weights -> y [B,Cout,H,W] (the input gradient swaps the channel counts)
// x2 / Csplit: optional second input tensor holding channels [Csplit, Cin); y2 / Osplit likewise for the output
struct FwdCall {
    const float* x; const float* wp; const float* bias; float* y;
    int B, Cin, Cout, H, W, ks, cfg;
    void* stats;
    const float* x2; int Csplit;
    float* y2; int Osplit;
    const void* xf; float xf_slope; int groups;
};
int conv_fwd_run(const uaps_call_hints& h, const FwdCall& c, uaps_stream_t stream);
// the rocprofv3 name of the kernel conv_fwd_run would launch, or the code it would return (nothing launched, no HIP call)
int conv_fwd_name(const uaps_call_hints& h, const FwdCall& c, char* buf, size_t buflen);

// weight gradient, step 1: per-split partials of dy (x) [x, x2] into the workspace
struct WrwCall {
    const float* dy; const float* x; const float* x2; int Csplit;
    int want_bias, B, Cin, Cout, H, W, ks, cfg;
    void* ws; size_t ws_bytes;
    const void* xf; float xf_slope; int groups;
};
int conv_wrw_run(const uaps_call_hints& h, const WrwCall& c, uaps_stream_t stream);
int conv_wrw_name(const uaps_call_hints& h, const WrwCall& c, char* buf, size_t buflen);

}  // namespace uaps
