"""uaps_mid_bwd_fused on the host (no GPU): every refusal -- bad arguments, a call outside the kernel's one form, a workspace that
is too small -- comes back before any HIP call, so the fake non-null device pointers are never dereferenced; and the host predicate
beside it."""
import ctypes as C

import pytest
import torch

from uaps_amd import _lib, conv

EINVAL, ERANGE, EWORKSPACE, ENOFORM = -1, -2, -3, -4
P = 4096                        # a non-null, 16-byte aligned "device" pointer: the calls below must refuse before touching it


@pytest.fixture()
def L():
    mode = conv.get_mode()
    conv.set_mode("h16")
    yield _lib.lib()
    conv.set_mode(mode)


def _need(L, B=2, Cin=16, Cout=16, H=16, W=256, ks=3, cfg=0):
    n = C.c_size_t()
    assert L.uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfg, C.byref(n)) == 0
    return n.value


def _call(L, dact=P, y2=P, coef=P, slope2=0.01, groups2=1, y1=P, xf=P, slope=0.01, groups=1, wb=P, dyb=P, xb=P, mean=P, invstd=P, gamma=P,
          beta=P, want_bias=1, B=2, Cin=16, Cout=16, H=16, W=256, ks=3, cfg=0, g=P, partials=P, maxes=P, ws=P, ws_bytes=0):
    return L.uaps_mid_bwd_fused(dact, y2, coef, slope2, groups2, y1, xf, slope, groups, wb, dyb, 1.0, xb, 1.0, mean, invstd, gamma, beta,
                                want_bias, B, Cin, Cout, H, W, ks, cfg, g, partials, maxes, ws, ws_bytes, None)


def test_bad_arguments_are_refused(L):
    for name in ("dact", "y1", "xf", "wb", "mean", "invstd", "gamma", "beta", "g", "partials", "maxes", "ws"):
        assert _call(L, **{name: None}) == EINVAL, name
    for bad in ({"B": 0}, {"H": 0}, {"W": -1}, {"Cin": 0}, {"Cout": 0}, {"groups": 0}, {"B": 3, "groups": 2}, {"xf": P + 4},
                {"coef": None}, {"y2": None}, {"groups2": 0}, {"B": 3, "groups2": 2}):
        assert _call(L, **bad) == EINVAL, bad
    assert _call(L, slope=1.5) == ERANGE and _call(L, slope=-0.1) == ERANGE


def test_outside_the_form_nothing_is_launched(L):
    for bad in ({"W": 128}, {"H": 24}, {"Cout": 8}, {"Cin": 32}, {"ks": 1}, {"cfg": 2 << 24}, {"cfg": 1 << 28}, {"dyb": None}, {"xb": None},
                {"y2": None, "coef": None}, {"dact": P + 4}, {"y1": P + 8}, {"g": P + 4}, {"ws": P + 4}):
        assert _call(L, **bad) == ENOFORM, bad
    conv.set_mode("exact")
    assert _call(L) == ENOFORM
    conv.set_mode("split")
    assert _call(L) == ENOFORM


def test_the_workspace_is_the_weight_gradient_plans(L):
    need = _need(L)
    assert need % ((9 * 16 * 16 + 16) * 4) == 0
    assert _call(L, ws_bytes=need - 1) == EWORKSPACE and _call(L, ws_bytes=0) == EWORKSPACE
    assert _call(L, cfg=3, ws_bytes=_need(L, cfg=3) - 4) == EWORKSPACE


def test_the_host_predicate():
    mode = conv.get_mode()
    try:
        conv.set_mode("h16")
        ok = lambda cout, cin, H, W, ks=3: conv.mid_bwd_eligible(torch.empty(1, cout, H, W), torch.empty(1, cin, H, W), ks)
        assert ok(16, 16, 32, 256) == conv._FUSED_MID
        assert not ok(8, 16, 32, 256) and not ok(16, 32, 32, 256) and not ok(16, 16, 24, 256) and not ok(16, 16, 32, 128) and not ok(16, 16, 32, 256, ks=1)
        conv.set_mode("exact")
        assert not ok(16, 16, 32, 256)
    finally:
        conv.set_mode(mode)
