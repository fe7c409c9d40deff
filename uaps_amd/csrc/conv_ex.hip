// uaps_conv_ex (include/uaps_hip.h): the convolution entry points with every operand in one size-versioned struct, and
// uaps_conv_ex_variant: the name of the kernel the same struct would launch.
#include "../../include/uaps_hip.h"
#include <string.h>
#include <stddef.h>
#include "hints.hpp"
#include "conv_call.hpp"

namespace {

// the call a uaps_conv_call describes: FWD and BWD_DATA as a FwdCall (the input gradient with the channel counts exchanged), BWD_WEIGHT as a WrwCall
struct Decoded {
    int op;
    uaps_call_hints h;
    uaps::FwdCall fwd;
    uaps::WrwCall wrw;
    uaps_stream_t stream;
};

int decode(const uaps_conv_call* c, Decoded& d) {
    if (!c) return UAPS_EINVAL;
    const unsigned n = c->struct_size;
    // everything up to and including `stream` is mandatory; the hints record at the tail is the part that grows (ABI 3: `stream` sits
    // in front of it, so a client built against a shorter uaps_call_hints still has its stream where this library reads it)
    if (n < offsetof(uaps_conv_call, hints) || n > sizeof(uaps_conv_call)) return UAPS_EINVAL;
    uaps_conv_call a;
    memset(&a, 0, sizeof a);
    memcpy(&a, c, n);
    const unsigned hmax = n - (unsigned)offsetof(uaps_conv_call, hints);
    if (a.hints.struct_size > hmax) return UAPS_EINVAL;          // a hints record that claims more bytes than the caller's struct holds
    const bool two = a.x2 != nullptr && a.C1 > 0 && a.C1 < a.Cin;
    const int groups = a.xf_groups > 0 ? a.xf_groups : 1;
    d.op = a.op;
    d.stream = a.stream;
    switch (a.op) {
    case UAPS_CONV_FWD:
        if (a.xf && two) return UAPS_ERANGE;      // no two-tensor form of the staging-time BatchNorm
        d.fwd = {a.x, a.w_packed, a.bias, a.y, a.B, a.Cin, a.Cout, a.H, a.W, a.ks, a.cfg, a.stats, two ? a.x2 : nullptr, two ? a.C1 : -1,
                 nullptr, -1, a.xf, a.xf ? a.xf_slope : 0.f, a.xf ? groups : 1};
        break;
    case UAPS_CONV_BWD_DATA: {
        const bool two_out = a.y2 && a.C1 > 0 && a.C1 < a.Cin;
        d.fwd = {a.x, a.w_packed, nullptr, a.y, a.B, a.Cout, a.Cin, a.H, a.W, a.ks, a.cfg, nullptr, nullptr, -1,
                 two_out ? a.y2 : nullptr, two_out ? a.C1 : -1, nullptr, 0.f, 1};
        break;
    }
    case UAPS_CONV_BWD_WEIGHT:
        if (a.xf && two) return UAPS_ERANGE;
        d.wrw = {a.y_grad, a.x, two ? a.x2 : nullptr, two ? a.C1 : a.Cin, a.want_bias, a.B, a.Cin, a.Cout, a.H, a.W, a.ks, a.cfg,
                 a.workspace, a.workspace_bytes, a.xf, a.xf ? a.xf_slope : 0.f, a.xf ? groups : 1};
        break;
    default:
        return UAPS_EINVAL;
    }
    // the struct's hints are THIS call's hints (none when hints.struct_size == 0): nothing thread-local is read or written, and a
    // record pending from uaps_next_call_hints is left alone
    return uaps::read_hints(a.hints.struct_size ? &a.hints : nullptr, d.h);
}

}  // namespace

extern "C" int uaps_conv_ex(const uaps_conv_call* c) {
    Decoded d;
    const int rc = decode(c, d);
    if (rc) return rc;
    return d.op == UAPS_CONV_BWD_WEIGHT ? uaps::conv_wrw_run(d.h, d.wrw, d.stream) : uaps::conv_fwd_run(d.h, d.fwd, d.stream);
}

extern "C" int uaps_conv_ex_variant(const uaps_conv_call* c, char* buf, size_t buflen) {
    Decoded d;
    const int rc = decode(c, d);
    if (rc) return rc;
    return d.op == UAPS_CONV_BWD_WEIGHT ? uaps::conv_wrw_name(d.h, d.wrw, buf, buflen) : uaps::conv_fwd_name(d.h, d.fwd, buf, buflen);
}
