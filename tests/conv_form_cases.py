"""The convolution kernel forms of libuaps_hip.so, one case per kernel instantiation (tests/test_conv_form_table.py,
tests/test_gpu_conv_forms.py).

A case is a whole uaps_conv_call (include/uaps_hip.h): op, arithmetic mode, planner switches, shape, the optional operands, and the
name of the ONE kernel resolve_fwd (csrc/conv_fwd.hip) or resolve_wrw (csrc/conv_wrw.hip) must pick for it.  The CPU test checks the
names with uaps_conv_ex_variant; the GPU test runs every case against a float64 reference.  A planner change that moves a case onto
another kernel fails the CPU test instead of silently testing something else.

Shapes are chosen where kernels go wrong: ragged H and W (partial last tiles in both directions) where the form allows them, B = 1 and
odd B, channel counts off the channel block, concatenation splits at the smallest legal step (8 forward, 16 weight gradient), BatchNorm
groups with different coefficients, slopes 0 and 1.  The full-width-row forms need W % 256 == 0 and H % 16 == 0: there odd B and
several 16-row runs per workgroup, 512 / 768-wide maps for the column-strip forms.
"""
from __future__ import annotations

import ctypes as C
import re
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

FWD, BWD_DATA, WRW = 0, 1, 2
OPS = {FWD: "fwd", BWD_DATA: "bwd_data", WRW: "wrw"}
MODES = {"exact": 0, "split": 1, "h16": 2}
BOUNDED = 1 << 11            # UAPS_CONV_BOUNDED
X2_UP2 = 1 << 10             # UAPS_CONV_X2_UP2
EXACT = 1 << 28              # cfg bit 28: the fp32 matrix-instruction kernels
SEL16, SEL32 = 1 << 29, 2 << 29      # cfg bits 29-30: force the 16x16x32 / 32x32x16 split form
WIDE, NARROW = 1 << 8, 2 << 8        # cfg bits 8-9: 8 x 32 / 16 x 16 pixel tiles
# UAPS_TUNE_* (include/uaps_hip.h)
NO_SPLIT_FWD, NO_SPLIT_WRW, NO_SMALL, NO_HP16 = 1, 2, 4, 8
SHORT_TILES, NO_TALL_FWD, NO_ROW16, NO_ROW_WRW, DEEP_ROWS, G1_NARROW, NO_G, G_DEEP = 32, 64, 128, 256, 512, 1024, 2048, 4096


@dataclass(frozen=True)
class Case:
    kernel: str                      # the instantiation the call must resolve to (as rocprofv3 prints it, without namespace)
    op: int
    mode: str
    B: int
    Cin: int
    Cout: int
    H: int
    W: int
    ks: int = 3
    dil: int = 1
    tune: int = 0                    # UAPS_TUNE_* bits
    cfg: int = 0                     # planner overrides: channel block (low byte), tile (bits 8-9), EXACT / SEL*; not dilation or flags
    bounded: Tuple[int, ...] = ()    # operands with a bound: FWD 0 = x, 1 = x2; BWD_DATA 0 = dy; WRW 0 = dy, 1 = x, 2 = x2
    C1: int = 0                      # concatenation split: FWD / WRW x2 holds input channels [C1, Cin); BWD_DATA y2 output channels [C1, Cin)
    xf: Optional[Tuple[float, int]] = None      # staging-time BatchNorm + LeakyReLU of x: (slope, groups)
    stats: str = ""                  # FWD BatchNorm partials: "plain", "bounded" (UAPS_CONV_BOUNDED), "mean" (about stats_mean - stats_bias)
    up2: bool = False                # x2 is the half-resolution tensor, bilinearly up-sampled x2 while staged
    dyt: Optional[Tuple[float, int]] = None     # WRW: dy formed from d(activation) while staged: (slope, groups)
    bsum: Optional[Tuple[float, int]] = None    # BWD_DATA: BatchNorm-backward sums in the epilogue: (slope, groups)
    out_amax: bool = False
    want_bias: bool = False          # FWD: a bias; WRW: the bias gradient
    offset: int = 0                  # floats by which x is moved off 16-byte alignment (the vec = 1 forms)
    loose: bool = False              # bounds a loose power of two above max|operand| instead of max|operand| itself
    tag: str = ""                    # tells apart further cases of one kernel

    @property
    def id(self) -> str:
        return f"{OPS[self.op]}-{self.mode}-{self.kernel}{'-' + self.tag if self.tag else ''}".replace(" ", "")

    def cfg_word(self) -> int:
        c = self.cfg | (self.dil << 24 if self.dil > 1 else 0)
        if self.up2:
            c |= X2_UP2
        if self.stats == "bounded":
            c |= BOUNDED
        return c

    @property
    def two_in(self) -> bool:
        return self.op != BWD_DATA and 0 < self.C1 < self.Cin

    @property
    def two_out(self) -> bool:
        return self.op == BWD_DATA and 0 < self.C1 < self.Cin


def make_call(lib_mod, case: Case, ptrs: dict, stream=None):
    """The uaps_conv_call of `case` (uaps_amd._lib.ConvCall).  ptrs maps operand names (x, x2, w, bias, y, y2, dy, stats, xf, ws,
    bound0..2, out_amax, stats_mean, stats_bias, dyt_y, dyt_coef, dyt_out, bsum_*) to device addresses; what is absent stays null."""
    c = lib_mod.ConvCall()
    c.struct_size = C.sizeof(lib_mod.ConvCall)
    c.op, c.B, c.Cin, c.Cout, c.H, c.W, c.ks, c.cfg = case.op, case.B, case.Cin, case.Cout, case.H, case.W, case.ks, case.cfg_word()
    c.stream = stream
    c.C1 = case.C1 if case.C1 else case.Cin
    if case.op == FWD:
        c.x, c.w_packed, c.y = ptrs["x"], ptrs["w"], ptrs["y"]
        c.bias = ptrs.get("bias")
        c.stats = ptrs.get("stats")
    elif case.op == BWD_DATA:
        c.x, c.w_packed, c.y = ptrs["dy"], ptrs["w"], ptrs["y"]
        c.y2 = ptrs.get("y2")
    else:
        c.x, c.y_grad = ptrs["x"], ptrs["dy"]
        c.want_bias = int(case.want_bias)
        c.workspace, c.workspace_bytes = ptrs["ws"], ptrs.get("ws_bytes", 0)
    if case.op != BWD_DATA:
        c.x2 = ptrs.get("x2")
    if case.xf is not None:
        c.xf, c.xf_slope, c.xf_groups = ptrs["xf"], case.xf[0], case.xf[1]
    h = c.hints
    h.struct_size = C.sizeof(lib_mod.CallHints)
    for i in case.bounded:
        h.bound[i], h.mul[i] = ptrs[f"bound{i}"], 1.0
    h.out_amax = ptrs.get("out_amax")
    if case.stats == "mean":
        h.stats_mean, h.stats_bias = ptrs["stats_mean"], ptrs["stats_bias"]
    if case.dyt is not None:
        h.dyt_y, h.dyt_coef, h.dyt_out, h.dyt_slope, h.dyt_groups = ptrs["dyt_y"], ptrs["dyt_coef"], ptrs["dyt_out"], case.dyt[0], case.dyt[1]
    if case.bsum is not None:
        (h.bsum_y, h.bsum_mean, h.bsum_invstd, h.bsum_gamma, h.bsum_beta, h.bsum_partials, h.bsum_max) = (
            ptrs["bsum_y"], ptrs["bsum_mean"], ptrs["bsum_invstd"], ptrs["bsum_gamma"], ptrs["bsum_beta"], ptrs["bsum_partials"], ptrs["bsum_max"])
        h.bsum_slope, h.bsum_groups = case.bsum[0], case.bsum[1]
    return c


_FAKE_NAMES = ("x", "x2", "w", "bias", "y", "y2", "dy", "stats", "xf", "ws", "bound0", "bound1", "bound2", "out_amax", "stats_mean",
               "stats_bias", "dyt_y", "dyt_coef", "dyt_out", "bsum_y", "bsum_mean", "bsum_invstd", "bsum_gamma", "bsum_beta",
               "bsum_partials", "bsum_max")


def fake_ptrs(case: Case) -> dict:
    """16-byte aligned addresses that are never dereferenced (uaps_conv_ex_variant launches nothing), x moved by case.offset floats;
    only the operands the case has."""
    p = {k: (1 << 24) + (i << 16) for i, k in enumerate(_FAKE_NAMES)}
    p["x"] += 4 * case.offset
    if not case.two_in:
        del p["x2"]
    if not case.two_out:
        del p["y2"]
    if not case.want_bias:
        del p["bias"]
    if not case.stats:
        del p["stats"]
    if not case.out_amax:
        del p["out_amax"]
    return p


def variant(L, lib_mod, case: Case):
    """The name uaps_conv_ex_variant gives the case's call under the case's mode and tuning, or its return code."""
    L.uaps_conv_set_mode(MODES[case.mode])
    L.uaps_conv_set_tuning(case.tune)
    buf = C.create_string_buffer(128)
    rc = L.uaps_conv_ex_variant(C.byref(make_call(lib_mod, case, fake_ptrs(case))), buf, 128)
    return buf.value.decode() if rc == 0 else rc


# One case per conv compute kernel of the code object (found with sweep(full=True) and the hinted forms; ragged, odd-B and
# off-block shapes preferred).  Planner overrides (cfg, tune) only where no plain call reaches the instantiation.
CASES = [
    Case('conv_fwd_bn_kernel<1, 16, 16, 16, 8, 4, 1>', FWD, 'h16', 3, 3, 4, 9, 20, ks=1, bounded=(0,), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_fwd_bn_kernel<1, 16, 16, 32, 8, 4, 1>', FWD, 'h16', 3, 3, 20, 9, 20, ks=1, cfg=32, bounded=(0,), xf=(1.0, 3)),
    Case('conv_fwd_bn_kernel<1, 16, 16, 64, 8, 4, 1>', FWD, 'h16', 3, 3, 64, 9, 20, ks=1, cfg=64, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_fwd_bn_kernel<1, 8, 32, 16, 8, 4, 1>', FWD, 'h16', 3, 3, 4, 13, 36, ks=1, bounded=(0,), xf=(0.0, 3), loose=True),
    Case('conv_fwd_bn_kernel<1, 8, 32, 32, 8, 4, 1>', FWD, 'h16', 3, 3, 20, 13, 36, ks=1, cfg=32, bounded=(0,), xf=(1.0, 3), want_bias=True),
    Case('conv_fwd_bn_kernel<1, 8, 32, 64, 8, 4, 1>', FWD, 'h16', 3, 3, 64, 13, 36, ks=1, cfg=64, bounded=(0,), xf=(0.2, 3)),
    Case('conv_fwd_bn_kernel<3, 16, 16, 16, 8, 4, 1>', FWD, 'exact', 3, 12, 4, 9, 20, xf=(0.0, 3), want_bias=True),
    Case('conv_fwd_bn_kernel<3, 16, 16, 32, 8, 4, 1>', FWD, 'exact', 3, 12, 20, 9, 20, cfg=SEL16 | 32, xf=(1.0, 3)),
    Case('conv_fwd_bn_kernel<3, 16, 16, 64, 8, 4, 1>', FWD, 'h16', 3, 12, 64, 9, 20, cfg=NARROW | 64, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_fwd_bn_kernel<3, 8, 32, 16, 8, 4, 1>', FWD, 'exact', 3, 12, 4, 13, 36, xf=(0.0, 3)),
    Case('conv_fwd_bn_kernel<3, 8, 32, 32, 8, 4, 1>', FWD, 'exact', 3, 12, 20, 13, 36, cfg=SEL16 | 32, xf=(1.0, 3), want_bias=True),
    Case('conv_fwd_bn_kernel<3, 8, 32, 64, 8, 4, 1>', FWD, 'exact', 3, 12, 64, 13, 36, cfg=64, xf=(0.2, 3)),
    Case('conv_fwd_kernel<1, 16, 16, 16, 8, 1, 1>', FWD, 'h16', 1, 3, 4, 9, 20, ks=1, bounded=(0,), want_bias=True, offset=1, loose=True),
    Case('conv_fwd_kernel<1, 16, 16, 16, 8, 4, 1>', FWD, 'h16', 3, 3, 4, 9, 20, ks=1, bounded=(0,)),
    Case('conv_fwd_kernel<1, 16, 16, 32, 8, 1, 1>', FWD, 'h16', 1, 3, 20, 9, 20, ks=1, cfg=SEL16 | 32, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<1, 16, 16, 32, 8, 4, 1>', FWD, 'h16', 3, 3, 20, 9, 20, ks=1, cfg=32, bounded=(0,), loose=True),
    Case('conv_fwd_kernel<1, 16, 16, 64, 8, 1, 1>', FWD, 'h16', 1, 3, 64, 9, 20, ks=1, cfg=64, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<1, 16, 16, 64, 8, 4, 1>', FWD, 'h16', 3, 3, 64, 9, 20, ks=1, cfg=64, bounded=(0,)),
    Case('conv_fwd_kernel<1, 8, 32, 16, 8, 1, 1>', FWD, 'h16', 1, 3, 4, 13, 36, ks=1, bounded=(0,), want_bias=True, offset=1, loose=True),
    Case('conv_fwd_kernel<1, 8, 32, 16, 8, 4, 1>', FWD, 'h16', 3, 3, 4, 13, 36, ks=1, bounded=(0,)),
    Case('conv_fwd_kernel<1, 8, 32, 32, 8, 1, 1>', FWD, 'h16', 1, 3, 20, 13, 36, ks=1, cfg=SEL16 | 32, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<1, 8, 32, 32, 8, 4, 1>', FWD, 'h16', 3, 3, 20, 13, 36, ks=1, cfg=32, bounded=(0,), loose=True),
    Case('conv_fwd_kernel<1, 8, 32, 64, 8, 1, 1>', FWD, 'h16', 1, 3, 64, 13, 36, ks=1, cfg=64, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<1, 8, 32, 64, 8, 4, 1>', FWD, 'h16', 3, 3, 64, 13, 36, ks=1, cfg=64, bounded=(0,)),
    Case('conv_fwd_kernel<3, 16, 16, 16, 4, 1, 1>', FWD, 'h16', 1, 3, 4, 9, 20, bounded=(0,), want_bias=True, offset=1, loose=True),
    Case('conv_fwd_kernel<3, 16, 16, 16, 4, 4, 1>', FWD, 'h16', 3, 3, 4, 9, 20, bounded=(0,)),
    Case('conv_fwd_kernel<3, 16, 16, 16, 8, 1, 1>', FWD, 'h16', 1, 12, 4, 9, 20, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 16, 16, 32, 8, 1, 1>', FWD, 'h16', 3, 12, 20, 9, 20, cfg=SEL16 | 32, bounded=(0,), offset=1, loose=True),
    Case('conv_fwd_kernel<3, 16, 16, 32, 8, 4, 1>', FWD, 'exact', 1, 12, 20, 9, 20, cfg=SEL16 | 32, want_bias=True),
    Case('conv_fwd_kernel<3, 16, 16, 64, 8, 1, 1>', FWD, 'h16', 3, 12, 64, 9, 20, cfg=NARROW | 64, bounded=(0,), offset=1),
    Case('conv_fwd_kernel<3, 16, 16, 64, 8, 4, 1>', FWD, 'h16', 1, 12, 64, 9, 20, cfg=NARROW | 64, bounded=(0,), want_bias=True, loose=True),
    Case('conv_fwd_kernel<3, 8, 32, 16, 4, 1, 1>', FWD, 'h16', 3, 3, 4, 13, 36, bounded=(0,), offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 16, 4, 4, 1>', FWD, 'h16', 1, 3, 4, 13, 36, bounded=(0,), want_bias=True),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 1, 1>', FWD, 'h16', 3, 12, 4, 13, 36, bounded=(0,), offset=1, loose=True),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 1, 2>', FWD, 'h16', 1, 12, 4, 9, 20, dil=2, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 1, 4>', FWD, 'h16', 3, 12, 4, 9, 20, dil=4, bounded=(0,), offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 4, 2>', FWD, 'h16', 1, 12, 4, 9, 20, dil=2, bounded=(0,), want_bias=True, loose=True),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 4, 4>', FWD, 'h16', 3, 12, 4, 9, 20, dil=4, bounded=(0,)),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 1, 1>', FWD, 'h16', 1, 12, 20, 13, 36, cfg=SEL16 | 32, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 1, 2>', FWD, 'h16', 32, 12, 20, 64, 64, dil=2, bounded=(0,), offset=1, loose=True),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 1, 4>', FWD, 'h16', 32, 12, 20, 64, 64, dil=4, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 4, 1>', FWD, 'exact', 3, 12, 20, 13, 36, cfg=SEL16 | 32),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 4, 2>', FWD, 'exact', 32, 12, 20, 64, 64, dil=2, want_bias=True),
    Case('conv_fwd_kernel<3, 8, 32, 32, 8, 4, 4>', FWD, 'exact', 32, 12, 20, 64, 64, dil=4),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 1, 1>', FWD, 'h16', 1, 12, 64, 13, 36, cfg=64, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 1, 2>', FWD, 'h16', 32, 12, 64, 64, 64, dil=2, bounded=(0,), offset=1, loose=True),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 1, 4>', FWD, 'h16', 32, 12, 64, 64, 64, dil=4, bounded=(0,), want_bias=True, offset=1),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 4, 1>', FWD, 'exact', 3, 12, 64, 13, 36, cfg=64),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 4, 2>', FWD, 'exact', 32, 12, 64, 64, 64, dil=2, want_bias=True),
    Case('conv_fwd_kernel<3, 8, 32, 64, 8, 4, 4>', FWD, 'exact', 32, 12, 64, 64, 64, dil=4),
    Case('conv_g1h256_kernel', FWD, 'h16', 1, 64, 256, 33, 36, ks=1, bounded=(0,), want_bias=True),
    Case('conv_g1h_kernel<128>', FWD, 'h16', 1, 128, 128, 37, 36, ks=1, bounded=(0,), loose=True),
    Case('conv_g1s_kernel<128>', FWD, 'split', 1, 64, 256, 33, 36, ks=1, want_bias=True),
    Case('conv_h32_bn_kernel<32>', FWD, 'h16', 3, 3, 20, 13, 36, cfg=SEL32, bounded=(0,), xf=(0.2, 3)),
    Case('conv_h32_bn_kernel<64>', FWD, 'h16', 3, 12, 64, 13, 36, cfg=64, bounded=(0,), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_h32_kernel<32>', FWD, 'h16', 3, 3, 20, 13, 36, cfg=SEL32, bounded=(0,)),
    Case('conv_h32_kernel<64>', FWD, 'h16', 1, 12, 64, 13, 36, cfg=64, bounded=(0,), want_bias=True),
    Case('conv_h32d_kernel<32, 2>', FWD, 'h16', 3, 12, 20, 9, 20, dil=2, bounded=(0,), loose=True),
    Case('conv_h32d_kernel<32, 4>', FWD, 'h16', 1, 12, 20, 9, 20, dil=4, bounded=(0,), want_bias=True),
    Case('conv_h32d_kernel<64, 2>', FWD, 'h16', 32, 12, 64, 64, 64, dil=2, bounded=(0,)),
    Case('conv_h32d_kernel<64, 4>', FWD, 'h16', 32, 12, 64, 64, 64, dil=4, bounded=(0,), want_bias=True, loose=True),
    Case('conv_h32t_bn_kernel<32>', FWD, 'h16', 32, 3, 96, 64, 64, cfg=SEL32, bounded=(0,), xf=(1.0, 32)),
    Case('conv_h32t_kernel<32>', FWD, 'h16', 32, 3, 96, 64, 64, cfg=SEL32, bounded=(0,), want_bias=True),
    Case('conv_hfwd_bn_kernel<1, 16, 16, 16, 32>', FWD, 'h16', 3, 3, 4, 9, 20, ks=1, cfg=SEL16, bounded=(0,), xf=(0.0, 3), loose=True),
    Case('conv_hfwd_bn_kernel<1, 16, 16, 32, 32>', FWD, 'h16', 3, 3, 20, 9, 20, ks=1, cfg=SEL16 | 32, bounded=(0,), xf=(1.0, 3), want_bias=True),
    Case('conv_hfwd_bn_kernel<1, 8, 32, 16, 32>', FWD, 'h16', 3, 3, 4, 13, 36, ks=1, cfg=SEL16, bounded=(0,), xf=(0.2, 3)),
    Case('conv_hfwd_bn_kernel<1, 8, 32, 32, 32>', FWD, 'h16', 3, 3, 20, 13, 36, ks=1, cfg=SEL16 | 32, bounded=(0,), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hfwd_bn_kernel<3, 16, 16, 16, 16>', FWD, 'h16', 3, 12, 4, 9, 20, bounded=(0,), xf=(1.0, 3)),
    Case('conv_hfwd_bn_kernel<3, 16, 16, 16, 8>', FWD, 'h16', 3, 3, 4, 9, 20, cfg=SEL16, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_hfwd_bn_kernel<3, 16, 16, 32, 16>', FWD, 'h16', 3, 12, 20, 9, 20, cfg=SEL16 | 32, bounded=(0,), xf=(0.0, 3), loose=True),
    Case('conv_hfwd_bn_kernel<3, 16, 16, 32, 8>', FWD, 'h16', 3, 3, 20, 9, 20, cfg=SEL16 | 32, bounded=(0,), xf=(1.0, 3), want_bias=True),
    Case('conv_hfwd_bn_kernel<3, 8, 32, 16, 16>', FWD, 'h16', 3, 12, 4, 13, 36, tune=NO_HP16, bounded=(0,), xf=(0.2, 3)),
    Case('conv_hfwd_bn_kernel<3, 8, 32, 16, 8>', FWD, 'h16', 3, 3, 4, 13, 36, cfg=SEL16, bounded=(0,), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hfwd_bn_kernel<3, 8, 32, 32, 16>', FWD, 'h16', 3, 12, 20, 13, 36, cfg=SEL16 | 32, bounded=(0,), xf=(1.0, 3)),
    Case('conv_hfwd_bn_kernel<3, 8, 32, 32, 8>', FWD, 'h16', 3, 3, 20, 13, 36, cfg=SEL16 | 32, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_hfwd_kernel<1, 16, 16, 16, 32>', FWD, 'h16', 3, 3, 4, 9, 20, ks=1, cfg=SEL16, bounded=(0,), loose=True),
    Case('conv_hfwd_kernel<1, 16, 16, 32, 32>', FWD, 'h16', 1, 3, 20, 9, 20, ks=1, cfg=SEL16 | 32, bounded=(0,), want_bias=True),
    Case('conv_hfwd_kernel<1, 8, 32, 16, 32>', FWD, 'h16', 3, 3, 4, 13, 36, ks=1, cfg=SEL16, bounded=(0,)),
    Case('conv_hfwd_kernel<1, 8, 32, 32, 32>', FWD, 'h16', 1, 3, 20, 13, 36, ks=1, cfg=SEL16 | 32, bounded=(0,), want_bias=True, loose=True),
    Case('conv_hfwd_kernel<3, 16, 16, 16, 8>', FWD, 'h16', 3, 3, 4, 9, 20, cfg=SEL16, bounded=(0,)),
    Case('conv_hfwd_kernel<3, 16, 16, 32, 16>', FWD, 'h16', 1, 12, 20, 9, 20, cfg=SEL16 | 32, bounded=(0,), want_bias=True),
    Case('conv_hfwd_kernel<3, 16, 16, 32, 8>', FWD, 'h16', 3, 3, 20, 9, 20, cfg=SEL16 | 32, bounded=(0,), loose=True),
    Case('conv_hfwd_kernel<3, 8, 32, 16, 8>', FWD, 'h16', 1, 3, 4, 13, 36, cfg=SEL16, bounded=(0,), want_bias=True),
    Case('conv_hfwd_kernel<3, 8, 32, 32, 16>', FWD, 'h16', 3, 12, 20, 13, 36, cfg=SEL16 | 32, bounded=(0,)),
    Case('conv_hfwd_kernel<3, 8, 32, 32, 8>', FWD, 'h16', 1, 3, 20, 13, 36, cfg=SEL16 | 32, bounded=(0,), want_bias=True, loose=True),
    Case('conv_hg128_deep_kernel', FWD, 'h16', 3, 32, 128, 12, 32, tune=G_DEEP, bounded=(0,)),
    Case('conv_hg128_kernel', FWD, 'h16', 1, 32, 128, 12, 32, bounded=(0,), want_bias=True),
    Case('conv_hp16_bn_kernel<2>', FWD, 'h16', 3, 12, 4, 13, 36, bounded=(0,), xf=(0.0, 3), loose=True),
    Case('conv_hp16_bn_kernel<4>', FWD, 'h16', 3, 20, 4, 13, 36, bounded=(0,), xf=(1.0, 3), want_bias=True),
    Case('conv_hr16_bn_kernel<2>', FWD, 'h16', 3, 12, 4, 16, 256, bounded=(0,), xf=(0.2, 3)),
    Case('conv_hr16_bn_kernel<4>', FWD, 'h16', 3, 20, 4, 16, 256, bounded=(0,), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hr16_up_kernel', FWD, 'h16', 3, 32, 4, 16, 256, bounded=(0, 1), C1=16, up2=True),
    Case('conv_hr16w_bn_kernel<2>', FWD, 'h16', 3, 12, 4, 16, 512, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_hr16w_bn_kernel<4>', FWD, 'h16', 3, 20, 4, 16, 512, bounded=(0,), xf=(0.0, 3), loose=True),
    Case('conv_hr16wx2_kernel', FWD, 'h16', 1, 16, 32, 16, 512, bounded=(0,), want_bias=True),
    Case('conv_hr16x2_kernel', FWD, 'h16', 3, 16, 32, 16, 256, bounded=(0,)),
    Case('conv_s32_bn_kernel<32>', FWD, 'split', 3, 3, 20, 13, 36, cfg=SEL32, xf=(0.0, 3), want_bias=True),
    Case('conv_s32_bn_kernel<64>', FWD, 'split', 3, 12, 64, 13, 36, cfg=64, xf=(1.0, 3)),
    Case('conv_s32_kernel<32>', FWD, 'split', 1, 3, 20, 13, 36, cfg=SEL32, want_bias=True),
    Case('conv_s32_kernel<64>', FWD, 'split', 3, 12, 64, 13, 36, cfg=64),
    Case('conv_s32d_kernel<32, 2>', FWD, 'split', 1, 12, 20, 9, 20, dil=2, want_bias=True),
    Case('conv_s32d_kernel<32, 4>', FWD, 'split', 3, 12, 20, 9, 20, dil=4),
    Case('conv_s32d_kernel<64, 2>', FWD, 'split', 32, 12, 64, 64, 64, dil=2, want_bias=True),
    Case('conv_s32d_kernel<64, 4>', FWD, 'split', 32, 12, 64, 64, 64, dil=4),
    Case('conv_s32t_bn_kernel<32>', FWD, 'split', 32, 3, 96, 64, 64, cfg=SEL32, xf=(0.2, 32), want_bias=True),
    Case('conv_s32t_kernel<32>', FWD, 'split', 32, 3, 96, 64, 64, cfg=SEL32),
    Case('conv_sfwd_bn_kernel<1, 16, 16, 16, 32>', FWD, 'split', 3, 3, 4, 9, 20, ks=1, cfg=SEL16, xf=(1.0, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<1, 16, 16, 32, 32>', FWD, 'split', 3, 3, 20, 9, 20, ks=1, cfg=SEL16 | 32, xf=(0.2, 3)),
    Case('conv_sfwd_bn_kernel<1, 8, 32, 16, 32>', FWD, 'split', 3, 3, 4, 13, 36, ks=1, cfg=SEL16, xf=(0.0, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<1, 8, 32, 32, 32>', FWD, 'split', 3, 3, 20, 13, 36, ks=1, cfg=SEL16 | 32, xf=(1.0, 3)),
    Case('conv_sfwd_bn_kernel<3, 16, 16, 16, 16>', FWD, 'split', 3, 12, 4, 9, 20, xf=(0.2, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<3, 16, 16, 16, 8>', FWD, 'split', 3, 3, 4, 9, 20, cfg=SEL16, xf=(0.0, 3)),
    Case('conv_sfwd_bn_kernel<3, 16, 16, 32, 16>', FWD, 'split', 3, 12, 20, 9, 20, cfg=SEL16 | 32, xf=(1.0, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<3, 16, 16, 32, 8>', FWD, 'split', 3, 3, 20, 9, 20, cfg=SEL16 | 32, xf=(0.2, 3)),
    Case('conv_sfwd_bn_kernel<3, 8, 32, 16, 16>', FWD, 'split', 3, 12, 4, 13, 36, xf=(0.0, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<3, 8, 32, 16, 8>', FWD, 'split', 3, 3, 4, 13, 36, cfg=SEL16, xf=(1.0, 3)),
    Case('conv_sfwd_bn_kernel<3, 8, 32, 32, 16>', FWD, 'split', 3, 12, 20, 13, 36, cfg=SEL16 | 32, xf=(0.2, 3), want_bias=True),
    Case('conv_sfwd_bn_kernel<3, 8, 32, 32, 8>', FWD, 'split', 3, 3, 20, 13, 36, cfg=SEL16 | 32, xf=(0.0, 3)),
    Case('conv_sfwd_kernel<1, 16, 16, 16, 32>', FWD, 'split', 1, 3, 4, 9, 20, ks=1, cfg=SEL16, want_bias=True),
    Case('conv_sfwd_kernel<1, 16, 16, 32, 32>', FWD, 'split', 3, 3, 20, 9, 20, ks=1, cfg=SEL16 | 32),
    Case('conv_sfwd_kernel<1, 8, 32, 16, 32>', FWD, 'split', 1, 3, 4, 13, 36, ks=1, cfg=SEL16, want_bias=True),
    Case('conv_sfwd_kernel<1, 8, 32, 32, 32>', FWD, 'split', 3, 3, 20, 13, 36, ks=1, cfg=SEL16 | 32),
    Case('conv_sfwd_kernel<3, 16, 16, 16, 8>', FWD, 'split', 1, 3, 4, 9, 20, cfg=SEL16, want_bias=True),
    Case('conv_sfwd_kernel<3, 16, 16, 32, 16>', FWD, 'split', 3, 12, 20, 9, 20, cfg=SEL16 | 32),
    Case('conv_sfwd_kernel<3, 16, 16, 32, 8>', FWD, 'split', 1, 3, 20, 9, 20, cfg=SEL16 | 32, want_bias=True),
    Case('conv_sfwd_kernel<3, 8, 32, 16, 8>', FWD, 'split', 3, 3, 4, 13, 36, cfg=SEL16),
    Case('conv_sfwd_kernel<3, 8, 32, 32, 16>', FWD, 'split', 1, 12, 20, 13, 36, cfg=SEL16 | 32, want_bias=True),
    Case('conv_sfwd_kernel<3, 8, 32, 32, 8>', FWD, 'split', 3, 3, 20, 13, 36, cfg=SEL16 | 32),
    Case('conv_small_bn_kernel<8, 4>', FWD, 'h16', 3, 16, 4, 64, 64, bounded=(0,), xf=(0.2, 3), want_bias=True),
    Case('conv_fwd_kernel<3, 16, 16, 16, 8, 4, 1>', BWD_DATA, 'exact', 3, 3, 12, 9, 20),
    Case('conv_fwd_kernel<3, 8, 32, 16, 8, 4, 1>', BWD_DATA, 'exact', 1, 3, 12, 13, 36),
    Case('conv_g1h_kernel<64>', BWD_DATA, 'h16', 1, 64, 256, 33, 36, ks=1, bounded=(0,)),
    Case('conv_g1s_kernel<64>', BWD_DATA, 'split', 1, 64, 256, 33, 36, ks=1),
    Case('conv_hfwd_kernel<3, 16, 16, 16, 16>', BWD_DATA, 'h16', 3, 3, 12, 9, 20, bounded=(0,)),
    Case('conv_hfwd_kernel<3, 8, 32, 16, 16>', BWD_DATA, 'h16', 1, 3, 12, 13, 36, tune=NO_HP16, bounded=(0,)),
    Case('conv_hp16_kernel<2>', BWD_DATA, 'h16', 3, 3, 12, 13, 36, bounded=(0,), loose=True),
    Case('conv_hp16_kernel<4>', BWD_DATA, 'h16', 1, 3, 20, 13, 36, bounded=(0,)),
    Case('conv_hr16_bs_kernel', BWD_DATA, 'h16', 3, 16, 16, 16, 256, bounded=(0,), bsum=(0.2, 3)),
    Case('conv_hr16_kernel<2>', BWD_DATA, 'h16', 1, 3, 12, 16, 256, bounded=(0,), loose=True),
    Case('conv_hr16_kernel<4>', BWD_DATA, 'h16', 3, 3, 20, 16, 256, bounded=(0,)),
    Case('conv_hr16w_kernel<2>', BWD_DATA, 'h16', 1, 3, 12, 16, 512, bounded=(0,)),
    Case('conv_hr16w_kernel<4>', BWD_DATA, 'h16', 3, 3, 20, 16, 512, bounded=(0,), loose=True),
    Case('conv_sfwd_kernel<3, 16, 16, 16, 16>', BWD_DATA, 'split', 1, 3, 12, 9, 20),
    Case('conv_sfwd_kernel<3, 8, 32, 16, 16>', BWD_DATA, 'split', 3, 3, 12, 13, 36),
    Case('conv_small_kernel<8, 4>', BWD_DATA, 'h16', 1, 3, 16, 64, 64, bounded=(0,), loose=True),
    Case('conv_gw1h_kernel', WRW, 'h16', 1, 128, 128, 32, 32, ks=1, bounded=(0, 1)),
    Case('conv_gw1s_kernel', WRW, 'split', 1, 128, 128, 32, 32, ks=1, want_bias=True),
    Case('conv_hrwrw2_bn_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, tune=DEEP_ROWS, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_hrwrw2_bn_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 256, tune=DEEP_ROWS, bounded=(0, 1), xf=(1.0, 3), want_bias=True),
    Case('conv_hrwrw2_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, tune=DEEP_ROWS, bounded=(0, 1)),
    Case('conv_hrwrw2_kernel<2>', WRW, 'h16', 1, 20, 4, 16, 256, tune=DEEP_ROWS, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_hrwrw_bn_dt_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, bounded=(0, 1), xf=(1.0, 3), dyt=(1.0, 3)),
    Case('conv_hrwrw_bn_dt_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 256, bounded=(0, 1), xf=(0.2, 3), dyt=(0.2, 3), want_bias=True),
    Case('conv_hrwrw_bn_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_hrwrw_bn_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 256, bounded=(0, 1), xf=(1.0, 3), want_bias=True),
    Case('conv_hrwrw_dt_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, bounded=(0, 1), dyt=(0.2, 3)),
    Case('conv_hrwrw_dt_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 256, bounded=(0, 1), dyt=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hrwrw_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 256, bounded=(0, 1)),
    Case('conv_hrwrw_kernel<2>', WRW, 'h16', 1, 20, 4, 16, 256, bounded=(0, 1), want_bias=True),
    Case('conv_hrwrw_up_dt_kernel', WRW, 'h16', 3, 32, 4, 16, 256, bounded=(0, 1, 2), C1=16, up2=True, dyt=(0.0, 3), loose=True),
    Case('conv_hrwrw_up_kernel', WRW, 'h16', 1, 32, 4, 16, 256, bounded=(0, 1, 2), C1=16, up2=True, want_bias=True),
    Case('conv_hrwrww_bn_dt_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 512, bounded=(0, 1), xf=(0.2, 3), dyt=(0.2, 3)),
    Case('conv_hrwrww_bn_dt_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 512, bounded=(0, 1), xf=(0.0, 3), dyt=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hrwrww_bn_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 512, bounded=(0, 1), xf=(1.0, 3)),
    Case('conv_hrwrww_bn_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 512, bounded=(0, 1), xf=(0.2, 3), want_bias=True),
    Case('conv_hrwrww_dt_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 512, bounded=(0, 1), dyt=(0.0, 3), loose=True),
    Case('conv_hrwrww_dt_kernel<2>', WRW, 'h16', 3, 20, 4, 16, 512, bounded=(0, 1), dyt=(1.0, 3), want_bias=True),
    Case('conv_hrwrww_kernel<1>', WRW, 'h16', 3, 3, 4, 16, 512, bounded=(0, 1)),
    Case('conv_hrwrww_kernel<2>', WRW, 'h16', 1, 20, 4, 16, 512, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_hwrw_bn_kernel<4, 1, 1>', WRW, 'h16', 3, 16, 4, 9, 20, tune=SHORT_TILES, bounded=(0, 1), xf=(1.0, 3)),
    Case('conv_hwrw_bn_kernel<4, 1, 2>', WRW, 'h16', 3, 20, 4, 9, 20, tune=SHORT_TILES, bounded=(0, 1), xf=(0.2, 3), want_bias=True),
    Case('conv_hwrw_bn_kernel<4, 2, 1>', WRW, 'h16', 3, 16, 20, 9, 20, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_hwrw_bn_kernel<4, 2, 2>', WRW, 'h16', 3, 20, 20, 9, 20, bounded=(0, 1), xf=(1.0, 3), want_bias=True),
    Case('conv_hwrw_bn_kernel<8, 1, 1>', WRW, 'h16', 3, 16, 4, 9, 20, bounded=(0, 1), xf=(0.2, 3)),
    Case('conv_hwrw_bn_kernel<8, 1, 2>', WRW, 'h16', 3, 20, 4, 9, 20, bounded=(0, 1), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_hwrw_d_kernel<4, 2, 2, 2>', WRW, 'h16', 3, 16, 4, 13, 36, dil=2, bounded=(0, 1)),
    Case('conv_hwrw_d_kernel<4, 2, 2, 4>', WRW, 'h16', 1, 16, 4, 13, 36, dil=4, bounded=(0, 1), want_bias=True),
    Case('conv_hwrw_kernel<4, 1, 1>', WRW, 'h16', 3, 16, 4, 9, 20, tune=SHORT_TILES, bounded=(0, 1), loose=True),
    Case('conv_hwrw_kernel<4, 1, 2>', WRW, 'h16', 1, 20, 4, 9, 20, tune=SHORT_TILES, bounded=(0, 1), want_bias=True),
    Case('conv_hwrw_kernel<4, 2, 1>', WRW, 'h16', 3, 16, 20, 9, 20, bounded=(0, 1)),
    Case('conv_hwrw_kernel<4, 2, 2>', WRW, 'h16', 1, 20, 20, 9, 20, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_hwrw_kernel<8, 1, 1>', WRW, 'h16', 3, 16, 4, 9, 20, bounded=(0, 1)),
    Case('conv_hwrw_kernel<8, 1, 2>', WRW, 'h16', 1, 20, 4, 9, 20, bounded=(0, 1), want_bias=True),
    Case('conv_small_wrw_bn_kernel', WRW, 'h16', 3, 16, 4, 64, 64, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_small_wrw_kernel', WRW, 'h16', 1, 16, 4, 64, 64, bounded=(0, 1), want_bias=True),
    Case('conv_swrw_bn_kernel<4, 1, 1>', WRW, 'split', 3, 16, 4, 9, 20, xf=(0.2, 3)),
    Case('conv_swrw_bn_kernel<4, 1, 2>', WRW, 'split', 3, 20, 4, 9, 20, xf=(0.0, 3), want_bias=True),
    Case('conv_swrw_bn_kernel<4, 2, 1>', WRW, 'split', 3, 16, 20, 9, 20, xf=(1.0, 3)),
    Case('conv_swrw_bn_kernel<4, 2, 2>', WRW, 'split', 3, 20, 20, 9, 20, xf=(0.2, 3), want_bias=True),
    Case('conv_swrw_kernel<4, 1, 1>', WRW, 'split', 3, 16, 4, 9, 20),
    Case('conv_swrw_kernel<4, 1, 2>', WRW, 'split', 1, 20, 4, 9, 20, want_bias=True),
    Case('conv_swrw_kernel<4, 2, 1>', WRW, 'split', 3, 16, 20, 9, 20),
    Case('conv_swrw_kernel<4, 2, 2>', WRW, 'split', 1, 20, 20, 9, 20, want_bias=True),
    Case('conv_wrw_bn_kernel<1, 16, 16, 1, 1, 4, 1>', WRW, 'h16', 3, 3, 4, 9, 20, ks=1, bounded=(0, 1), xf=(1.0, 3)),
    Case('conv_wrw_bn_kernel<1, 16, 16, 1, 2, 4, 1>', WRW, 'h16', 3, 20, 4, 9, 20, ks=1, bounded=(0, 1), xf=(0.2, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<1, 16, 16, 2, 1, 4, 1>', WRW, 'h16', 3, 3, 20, 9, 20, ks=1, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_wrw_bn_kernel<1, 4, 32, 2, 2, 4, 1>', WRW, 'h16', 3, 20, 20, 13, 36, ks=1, bounded=(0, 1), xf=(1.0, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<1, 8, 16, 2, 2, 4, 1>', WRW, 'h16', 3, 20, 20, 9, 20, ks=1, bounded=(0, 1), xf=(0.2, 3)),
    Case('conv_wrw_bn_kernel<1, 8, 32, 1, 1, 4, 1>', WRW, 'h16', 3, 3, 4, 13, 36, ks=1, bounded=(0, 1), xf=(0.0, 3), want_bias=True, loose=True),
    Case('conv_wrw_bn_kernel<1, 8, 32, 1, 2, 4, 1>', WRW, 'h16', 3, 20, 4, 13, 36, ks=1, bounded=(0, 1), xf=(1.0, 3)),
    Case('conv_wrw_bn_kernel<1, 8, 32, 2, 1, 4, 1>', WRW, 'h16', 3, 3, 20, 13, 36, ks=1, bounded=(0, 1), xf=(0.2, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<3, 16, 16, 1, 1, 4, 1>', WRW, 'h16', 3, 3, 4, 9, 20, bounded=(0, 1), xf=(0.0, 3), loose=True),
    Case('conv_wrw_bn_kernel<3, 16, 16, 1, 2, 4, 1>', WRW, 'exact', 3, 20, 4, 9, 20, xf=(1.0, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<3, 16, 16, 2, 1, 4, 1>', WRW, 'h16', 3, 3, 20, 9, 20, bounded=(0, 1), xf=(0.2, 3)),
    Case('conv_wrw_bn_kernel<3, 4, 32, 2, 2, 4, 1>', WRW, 'exact', 3, 20, 20, 13, 36, xf=(0.0, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<3, 8, 16, 2, 2, 4, 1>', WRW, 'exact', 3, 20, 20, 9, 20, xf=(1.0, 3)),
    Case('conv_wrw_bn_kernel<3, 8, 32, 1, 1, 4, 1>', WRW, 'h16', 3, 3, 4, 13, 36, bounded=(0, 1), xf=(0.2, 3), want_bias=True),
    Case('conv_wrw_bn_kernel<3, 8, 32, 1, 2, 4, 1>', WRW, 'exact', 3, 20, 4, 13, 36, xf=(0.0, 3)),
    Case('conv_wrw_bn_kernel<3, 8, 32, 2, 1, 4, 1>', WRW, 'h16', 3, 3, 20, 13, 36, bounded=(0, 1), xf=(1.0, 3), want_bias=True),
    Case('conv_wrw_kernel<1, 16, 16, 1, 1, 1, 1>', WRW, 'h16', 3, 3, 4, 9, 20, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 16, 16, 1, 1, 4, 1>', WRW, 'h16', 1, 3, 4, 9, 20, ks=1, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_wrw_kernel<1, 16, 16, 1, 2, 1, 1>', WRW, 'h16', 3, 20, 4, 9, 20, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 16, 16, 1, 2, 4, 1>', WRW, 'h16', 1, 20, 4, 9, 20, ks=1, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<1, 16, 16, 2, 1, 1, 1>', WRW, 'h16', 3, 3, 20, 9, 20, ks=1, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<1, 16, 16, 2, 1, 4, 1>', WRW, 'h16', 1, 3, 20, 9, 20, ks=1, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<1, 4, 32, 2, 2, 1, 1>', WRW, 'h16', 3, 20, 20, 13, 36, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 4, 32, 2, 2, 4, 1>', WRW, 'h16', 1, 20, 20, 13, 36, ks=1, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_wrw_kernel<1, 8, 16, 2, 2, 1, 1>', WRW, 'h16', 3, 20, 20, 9, 20, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 8, 16, 2, 2, 4, 1>', WRW, 'h16', 1, 20, 20, 9, 20, ks=1, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<1, 8, 32, 1, 1, 1, 1>', WRW, 'h16', 3, 3, 4, 13, 36, ks=1, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<1, 8, 32, 1, 1, 4, 1>', WRW, 'h16', 1, 3, 4, 13, 36, ks=1, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<1, 8, 32, 1, 2, 1, 1>', WRW, 'h16', 3, 20, 4, 13, 36, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 8, 32, 1, 2, 4, 1>', WRW, 'h16', 1, 20, 4, 13, 36, ks=1, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_wrw_kernel<1, 8, 32, 2, 1, 1, 1>', WRW, 'h16', 3, 3, 20, 13, 36, ks=1, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<1, 8, 32, 2, 1, 4, 1>', WRW, 'h16', 1, 3, 20, 13, 36, ks=1, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<3, 16, 16, 1, 1, 1, 1>', WRW, 'h16', 3, 3, 4, 9, 20, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<3, 16, 16, 1, 1, 4, 1>', WRW, 'h16', 1, 3, 4, 9, 20, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<3, 16, 16, 1, 2, 1, 1>', WRW, 'h16', 3, 20, 4, 9, 20, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<3, 16, 16, 1, 2, 4, 1>', WRW, 'exact', 1, 20, 4, 9, 20, want_bias=True),
    Case('conv_wrw_kernel<3, 16, 16, 2, 1, 1, 1>', WRW, 'h16', 3, 3, 20, 9, 20, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<3, 16, 16, 2, 1, 4, 1>', WRW, 'h16', 1, 3, 20, 9, 20, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 1, 1>', WRW, 'h16', 3, 20, 20, 13, 36, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 1, 2>', WRW, 'h16', 1, 12, 4, 9, 20, dil=2, cfg=EXACT, bounded=(0, 1), want_bias=True, offset=1),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 1, 4>', WRW, 'h16', 3, 12, 4, 9, 20, dil=4, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 4, 1>', WRW, 'exact', 1, 20, 20, 13, 36, want_bias=True),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 4, 2>', WRW, 'h16', 3, 12, 4, 9, 20, dil=2, bounded=(0, 1)),
    Case('conv_wrw_kernel<3, 4, 32, 2, 2, 4, 4>', WRW, 'h16', 1, 12, 4, 9, 20, dil=4, bounded=(0, 1), want_bias=True),
    Case('conv_wrw_kernel<3, 8, 16, 2, 2, 1, 1>', WRW, 'h16', 3, 20, 20, 9, 20, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<3, 8, 16, 2, 2, 4, 1>', WRW, 'exact', 1, 20, 20, 9, 20, want_bias=True),
    Case('conv_wrw_kernel<3, 8, 32, 1, 1, 1, 1>', WRW, 'h16', 3, 3, 4, 13, 36, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<3, 8, 32, 1, 1, 4, 1>', WRW, 'h16', 1, 3, 4, 13, 36, bounded=(0, 1), want_bias=True, loose=True),
    Case('conv_wrw_kernel<3, 8, 32, 1, 2, 1, 1>', WRW, 'h16', 3, 20, 4, 13, 36, cfg=EXACT, bounded=(0, 1), offset=1),
    Case('conv_wrw_kernel<3, 8, 32, 1, 2, 4, 1>', WRW, 'exact', 1, 20, 4, 13, 36, want_bias=True),
    Case('conv_wrw_kernel<3, 8, 32, 2, 1, 1, 1>', WRW, 'h16', 3, 3, 20, 13, 36, cfg=EXACT, bounded=(0, 1), offset=1, loose=True),
    Case('conv_wrw_kernel<3, 8, 32, 2, 1, 4, 1>', WRW, 'h16', 1, 3, 20, 13, 36, bounded=(0, 1), want_bias=True),
]
# second tensors at the smallest legal split (8 forward and input gradient, 16 weight gradient) in the three arithmetics, and more
# statistics variants
CASES += [
    Case("conv_h32_kernel<32>", FWD, "h16", 3, 24, 20, 13, 36, bounded=(0, 1), C1=8, want_bias=True, stats="plain", tag="cat8"),
    Case("conv_s32_kernel<32>", FWD, "split", 3, 48, 20, 13, 36, C1=16, stats="mean", tag="cat16"),
    Case("conv_fwd_kernel<3, 8, 32, 16, 8, 4, 1>", FWD, "exact", 1, 24, 12, 13, 36, C1=8, tag="cat8"),
    Case("conv_fwd_kernel<3, 16, 16, 16, 8, 4, 1>", FWD, "h16", 1, 40, 16, 9, 20, bounded=(0, 1), C1=8, tag="cat8"),
    Case("conv_hfwd_kernel<3, 8, 32, 16, 16>", BWD_DATA, "h16", 3, 40, 20, 13, 36, bounded=(0,), C1=8, tag="cat8"),
    Case("conv_sfwd_kernel<3, 8, 32, 16, 16>", BWD_DATA, "split", 1, 48, 32, 13, 36, C1=16, tag="cat16"),
    Case("conv_fwd_kernel<3, 16, 16, 16, 8, 4, 1>", BWD_DATA, "exact", 3, 24, 12, 9, 20, C1=8, tag="cat8"),
    Case("conv_hwrw_kernel<4, 2, 2>", WRW, "h16", 3, 48, 20, 13, 36, bounded=(0, 1, 2), C1=16, want_bias=True, tag="cat16"),
    Case("conv_swrw_kernel<4, 2, 2>", WRW, "split", 3, 48, 20, 13, 36, C1=16, tag="cat16"),
    Case("conv_wrw_kernel<3, 16, 16, 1, 2, 4, 1>", WRW, "exact", 1, 40, 12, 9, 20, cfg=EXACT, C1=16, tag="cat16"),
    Case("conv_hr16_kernel<2>", FWD, "h16", 3, 16, 16, 32, 256, bounded=(0,), stats="bounded", want_bias=True, tag="stats"),
    Case("conv_hfwd_kernel<3, 8, 32, 16, 16>", FWD, "h16", 3, 64, 48, 13, 36, bounded=(0,), loose=True, stats="mean", tag="stats"),
]

# out_amax (max|y| raised into a bound) exists in the fp32-instruction tile kernels only (check_fwd: UAPS_ENOFORM elsewhere, see
# OUT_AMAX_REFUSED): the U-Net's 1x1 projection form in each arithmetic mode, 3x3 tiles of both shapes, the vec = 1 form, with
# statistics and with the staging-time BatchNorm
CASES += [
    Case("conv_fwd_kernel<1, 8, 32, 16, 8, 4, 1>", FWD, "h16", 3, 16, 16, 17, 44, ks=1, bounded=(0,), out_amax=True, want_bias=True, tag="amax"),
    Case("conv_fwd_kernel<1, 16, 16, 16, 8, 4, 1>", FWD, "split", 1, 16, 12, 9, 20, ks=1, out_amax=True, tag="amax"),
    Case("conv_fwd_kernel<3, 8, 32, 16, 8, 4, 1>", FWD, "split", 1, 8, 20, 13, 36, out_amax=True, stats="plain", tag="amax"),
    Case("conv_fwd_kernel<3, 16, 16, 16, 8, 4, 1>", FWD, "exact", 3, 40, 48, 9, 20, out_amax=True, want_bias=True, tag="amax"),
    Case("conv_fwd_kernel<3, 8, 32, 16, 8, 1, 1>", FWD, "exact", 3, 40, 48, 13, 36, out_amax=True, offset=1, tag="amax"),
    Case("conv_fwd_bn_kernel<3, 8, 32, 16, 8, 4, 1>", FWD, "exact", 3, 16, 20, 13, 36, xf=(1.0, 3), out_amax=True, tag="amax"),
]

# calls of the split and row forms with out_amax: refused before launch (nothing in the table can check a bound they never raise)
OUT_AMAX_REFUSED = [
    Case("", FWD, "h16", 3, 16, 16, 16, 256, bounded=(0,), out_amax=True),       # conv_hr16_kernel<2> without it
    Case("", FWD, "split", 3, 16, 16, 16, 256, out_amax=True),                    # conv_sfwd_kernel
    Case("", FWD, "h16", 1, 128, 128, 32, 32, bounded=(0,), out_amax=True),      # conv_hg128_kernel
    Case("", FWD, "h16", 3, 12, 4, 9, 20, bounded=(0,), xf=(0.2, 3), out_amax=True),
]

# Instantiations that are built and listed in a launch switch but that no call can reach, with the resolver's reason.
UNREACHABLE = {
    "conv_hg128_bn_kernel": "resolve_fwd takes the HG128 form only when !xf (the staging-time BatchNorm keeps the tile kernels)",
}


def _options(op: int, Cin: int, ks: int):
    """The optional-operand variants of one call (bounds as the h16 mode needs them)."""
    nb = {FWD: (0,), BWD_DATA: (0,), WRW: (0, 1)}[op]
    yield dict(bounded=nb)
    yield dict(bounded=nb, offset=1, cfg=EXACT if op == WRW else 0)
    if op != BWD_DATA:
        yield dict(bounded=nb, xf=(0.01, 1))
    if op == FWD:
        yield dict(bounded=nb, stats="plain")
        yield dict(bounded=nb, stats="bounded")
        yield dict(bounded=nb, xf=(0.01, 1), stats="plain")
        yield dict(bounded=nb, out_amax=True)
        for c in (SEL16, SEL16 | 32, SEL32, 32, 64, WIDE, NARROW, NARROW | 64):
            yield dict(bounded=nb, cfg=c)
            yield dict(bounded=nb, cfg=c, xf=(0.01, 1))
            yield dict(bounded=nb, cfg=c, offset=1)
    if op == BWD_DATA:
        yield dict(bounded=nb, bsum=(0.01, 1))
        for c in (SEL16, SEL16 | 32, 64, NARROW | 64):
            yield dict(bounded=nb, cfg=c)
    if op == WRW:
        yield dict(bounded=nb, dyt=(0.01, 1))
        yield dict(bounded=nb, xf=(0.01, 1), dyt=(0.01, 1))
        yield dict(bounded=nb, want_bias=True)
    if Cin >= 32 and Cin % 32 == 0:
        two = (0, 1) if op == FWD else (0, 1, 2) if op == WRW else (0,)
        yield dict(bounded=two, C1=Cin // 2)
        if op == FWD:
            yield dict(bounded=two, C1=Cin // 2, stats="plain")
        if op != BWD_DATA:
            yield dict(bounded=two, C1=Cin // 2, up2=True)
            if op == WRW:
                yield dict(bounded=two, C1=Cin // 2, up2=True, dyt=(0.01, 1))
    if ks == 3 and Cin > 4:
        for dil in (2, 4):
            yield dict(bounded=nb, dil=dil)
            yield dict(bounded=nb, dil=dil, offset=1, cfg=EXACT if op == WRW else 0)


def sweep(full: bool = False):
    """Calls in the spirit of a planner sweep: op x mode x tuning bits x channels x map sizes x ks x dilation x bounds x
    concatenation x xf x statistics x alignment x the hinted forms (up2, dyt, bsum) x planner overrides, with and without a second
    input or output tensor.  The CPU test runs the quick form (a few seconds) and requires that it names no UNREACHABLE kernel."""
    chans = (3, 4, 8, 16, 24, 32, 48, 64, 128, 256, 512) if full else (3, 8, 16, 32, 64, 128, 256)
    maps = ((8, 8), (12, 20), (16, 16), (16, 24), (32, 32), (36, 40), (64, 64), (16, 256), (32, 256), (16, 512), (128, 128),
            (256, 256)) if full else ((12, 20), (16, 16), (32, 32), (64, 64), (16, 256), (16, 512))
    tunes = (0, NO_SMALL, NO_HP16, NO_ROW16, NO_ROW_WRW, DEEP_ROWS, G1_NARROW, NO_G, G_DEEP, NO_TALL_FWD, SHORT_TILES,
             NO_SPLIT_FWD | NO_SPLIT_WRW)
    for mode in ("h16", "split", "exact"):
        for tune in (tunes if mode == "h16" else (0,)):
            for (H, W) in maps:
                for B in ((1, 4, 32) if full else (3, 32) if (H, W) in ((32, 32), (64, 64)) else (3,)):
                    for Cin in chans:
                        for Cout in chans:
                            for ks in (3, 1):
                                for op in (FWD, BWD_DATA, WRW):
                                    base = Case("", op, mode, B, Cin, Cout, H, W, ks, tune=tune)
                                    for o in _options(op, Cin, ks):
                                        if tune and (o.get("cfg") or o.get("dil") or o.get("offset")):
                                            continue
                                        c = replace(base, **o)
                                        yield c if mode == "h16" else replace(c, bounded=())


# ---- inputs, float64 reference and the bar (shared by the GPU test and the CPU discrimination test) ---------------------------

TAU_Y = 5e-6          # pointwise bar of y and dx: |got - ref| <= TAU * sum|a*b| (the bar test_split_mode_is_as_accurate_as... holds)
TAU_DW = 2e-6         # the weight gradient's: 2.2x the largest measured on the correct kernels of all three modes (profiles/conv_forms_dw_tau.txt)
RMS_FACTOR = 3.0      # precision: RMS((got - ref) / R) <= RMS_FACTOR * the same of torch float32 on one CPU thread + RMS_FLOOR
RMS_FLOOR = 2.5e-7    # (a correct two-piece fp16 operand carries 22 significant bits: ~2^-22 of R; fp32 CPU sums of few terms less)


def lognormal(g, shape, spread=2.0):
    """Magnitudes spread over e^(+-3 spread) so that every piece of every operand matters; ~3 % exact zeros."""
    import torch
    v = torch.randn(shape, generator=g, dtype=torch.float64) * torch.exp(spread * torch.randn(shape, generator=g, dtype=torch.float64))
    v[torch.rand(shape, generator=g, dtype=torch.float64) < 0.03] = 0.0
    return v.float()


def make_inputs(case: Case, seed: int = 0) -> dict:
    """float32 CPU tensors of one case: x [B,Cin,H,W] (with x2's channels; up2: x2 is x2_low [B,Cin-C1,H/2,W/2]), w, bias, dy, and the
    coefficient tensors of xf / dyt / bsum / stats_mean.  One input channel is all zero."""
    import torch
    g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(case.id.encode()) % 100003)      # the same data in every process
    B, Cin, Cout, H, W, ks = case.B, case.Cin, case.Cout, case.H, case.W, case.ks
    d = {}
    x = lognormal(g, (B, Cin, H, W))
    x[:, Cin // 2] = 0.0
    d["x"] = x
    if case.up2:
        d["x2_low"] = lognormal(g, (B, Cin - case.C1, H // 2, W // 2))
    d["w"] = lognormal(g, (Cout, Cin, ks, ks), 1.0) / float(Cin * ks * ks) ** 0.5
    d["bias"] = lognormal(g, (Cout,), 1.0)
    d["dy"] = lognormal(g, (B, Cout, H, W))
    if case.xf is not None:
        G = case.xf[1]
        d["xf"] = torch.stack([torch.exp(0.5 * torch.randn(G, Cin, generator=g, dtype=torch.float64)) *
                               torch.where(torch.rand(G, Cin, generator=g) < 0.2, -1.0, 1.0).double(),
                               3.0 * torch.randn(G, Cin, generator=g, dtype=torch.float64)], -1).float()      # (scale, shift) per group
    if case.stats == "mean":
        d["stats_mean"] = (5.0 * torch.randn(Cout, generator=g)).float()
        d["stats_bias"] = torch.randn(Cout, generator=g).float()
    if case.dyt is not None or case.bsum is not None:
        G = (case.dyt or case.bsum)[1]
        C = Cout if case.dyt is not None else Cin
        mean = torch.randn(G, C, generator=g, dtype=torch.float64)
        invstd = torch.exp(0.5 * torch.randn(G, C, generator=g, dtype=torch.float64))
        gamma = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
        beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
        yraw = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2.0
        # keep the BatchNorm output away from 0, where the sign test of the LeakyReLU derivative could go either way in fp32
        gi = torch.arange(B) // (B // G)
        mu, ist = mean[gi][:, :, None, None], invstd[gi][:, :, None, None]
        z = (yraw - mu) * ist * gamma[None, :, None, None] + beta[None, :, None, None]
        zf = torch.where(z.abs() < 1e-3, torch.where(z < 0, -1e-3, 1e-3), z)
        yraw = mu + (zf - beta[None, :, None, None]) / (gamma[None, :, None, None] * ist)
        d["bn"] = dict(y=yraw.float(), mean=mean.float(), invstd=invstd.float(), gamma=gamma.float(), beta=beta.float(), slope=(case.dyt or case.bsum)[0])
        if case.dyt is not None:
            md = 0.1 * torch.randn(G, C, generator=g, dtype=torch.float64)
            mdx = 0.1 * torch.randn(G, C, generator=g, dtype=torch.float64)
            coef = torch.zeros(G, C, 8, dtype=torch.float64)
            coef[..., 0], coef[..., 1], coef[..., 2], coef[..., 3], coef[..., 4], coef[..., 5] = mean, invstd, gamma * invstd, beta.expand(G, C), md, mdx
            d["dyt_coef"] = coef.float()
    return d


def _groups_index(B: int, G: int):
    import torch
    return torch.arange(B) // (B // G)


def _up2_matrix(n: int):
    """[2 n, n] bilinear align_corners weights as the kernels (and ATen's fp32 upsample_bilinear2d) form them: the source
    coordinate r * x with r = (n - 1) / (2 n - 1) and the weights (1 - l, l) rounded to fp32; the interpolation itself is exact."""
    import numpy as np
    import torch
    r = np.float32(n - 1) / np.float32(2 * n - 1)
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for x in range(2 * n):
        sx = np.float32(r * np.float32(x))
        i0 = int(sx)
        l1 = np.float32(sx - np.float32(i0))
        m[x, i0] += float(np.float32(1) - l1)
        m[x, min(i0 + 1, n - 1)] += float(l1)
    return m


def upsample2x(low):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) of a float64 [B, C, h, w] tensor with the kernels' weights."""
    mh, mw = _up2_matrix(low.shape[2]), _up2_matrix(low.shape[3])
    return mh @ low @ mw.T


def staged_input(case: Case, inp: dict, absolute: bool = False):
    """The contraction's input operand in float64 (FWD / WRW): [x, up2(x2_low)] and the staging-time BatchNorm + LeakyReLU; with
    absolute, the same operation on |operands| (a bound of every term's magnitude)."""
    import torch
    import torch.nn.functional as F
    x = inp["x"].double()
    if case.up2:
        low = inp["x2_low"].double()
        up = upsample2x(low.abs() if absolute else low)
        x = torch.cat([x[:, :case.C1], up], 1)
    if absolute:
        x = x.abs()
    if case.xf is not None:
        gi = _groups_index(case.B, case.xf[1])
        sc, sh = inp["xf"].double()[gi][..., 0, None, None], inp["xf"].double()[gi][..., 1, None, None]
        if absolute:
            x = x * sc.abs() + sh.abs()
        else:
            z = x * sc + sh
            x = torch.maximum(z, case.xf[0] * z)
    return x


def true_dy(case: Case, inp: dict, absolute: bool = False):
    """WRW with dyt: dy = gamma invstd (d - mean(d) - x_hat mean(d x_hat)), d = g or slope g by the sign of the BatchNorm output."""
    import torch
    dy = inp["dy"].double()
    if case.dyt is None:
        return dy.abs() if absolute else dy
    gi = _groups_index(case.B, case.dyt[1])
    c = inp["dyt_coef"].double()[gi][..., None, None]           # [B, C, 8, 1, 1]
    yc = inp["bn"]["y"].double() - c[:, :, 0]
    z = yc * c[:, :, 2] + c[:, :, 3]
    d = torch.where(z > 0, dy, dy * case.dyt[0])
    if absolute:
        return c[:, :, 2].abs() * (d.abs() + c[:, :, 4].abs() + (yc * c[:, :, 1]).abs() * c[:, :, 5].abs())
    return c[:, :, 2] * (d - c[:, :, 4] - yc * c[:, :, 1] * c[:, :, 5])


def contract(case: Case, a, b):
    """The case's contraction in a's dtype: FWD y = conv(a = input, b = w); BWD_DATA dx = conv_transpose(a = dy, b = w);
    WRW dw = conv2d_weight(a = input, b = dy)."""
    import torch
    import torch.nn.functional as F
    pad, dil = case.dil * (case.ks // 2), case.dil
    if case.op == FWD:
        return F.conv2d(a, b, None, padding=pad, dilation=dil)
    if case.op == BWD_DATA:
        return torch.nn.grad.conv2d_input((case.B, case.Cin, case.H, case.W), b, a, padding=pad, dilation=dil)
    return torch.nn.grad.conv2d_weight(a, (case.Cout, case.Cin, case.ks, case.ks), b, padding=pad, dilation=dil)


def operands(case: Case, inp: dict, absolute: bool = False):
    """(a, b, additive term) of the case's main result in float64."""
    w = inp["w"].double()
    if case.op == FWD:
        bias = inp["bias"].double() if case.want_bias else None
        return staged_input(case, inp, absolute), (w.abs() if absolute else w), (bias.abs() if absolute and bias is not None else bias)
    if case.op == BWD_DATA:
        dy = inp["dy"].double()
        return (dy.abs() if absolute else dy), (w.abs() if absolute else w), None
    return staged_input(case, inp, absolute), true_dy(case, inp, absolute), None


def h16_floors(case: Case, inp: dict):
    """The magnitudes below which a two-piece fp16 operand no longer carries 22 significant bits: 2^-18 of its bound (csrc/conv_split.hpp,
    h16_scale): the caller's bound for a tensor operand (loose or tight as the case hands it), max|w| for the packed weights, which
    uaps_conv_pack_weights scales by their own maximum.  None for the kernels without fp16 pieces."""
    import numpy as np
    if not (case.mode == "h16" and case.bounded and re.match(r"conv_(h|g1h|gw1h)", case.kernel)):
        return None

    def bound(t, caller_bound):
        m = float(t.abs().max())
        return 2.0 ** (np.floor(np.log2(max(m, 1e-30))) + 2) if case.loose and caller_bound else m
    a, b, _ = operands(case, inp)
    return 2.0 ** -18 * bound(a, True), 2.0 ** -18 * bound(b, case.op == WRW)      # WRW: b is dy, a bounded tensor; else the weights


def reference(case: Case, inp: dict, rounding=None, floors=None) -> dict:
    """float64 main result `ref`, its term magnitude `M` = the operation on |a|, |b| (sum |a*b|), and R = sqrt(sum (a*b)^2).
    rounding(t) -> t, if given, is applied to both contraction operands first (emulated kernel arithmetic).  floors (h16_floors):
    nonzero operand magnitudes count as at least these in M and R (the documented precision of the fp16 pieces, relative to the
    bound below 2^-18 of it; zeros stay exact)."""
    import torch
    a, b, add = operands(case, inp)
    am, bm, addm = operands(case, inp, absolute=True)
    ra, rb = (rounding(a), rounding(b)) if rounding else (a, b)
    ref = contract(case, ra, rb)
    if floors is not None:
        am = torch.where(am > 0, am.clamp_min(floors[0]), am)
        bm = torch.where(bm > 0, bm.clamp_min(floors[1]), bm)
    M = contract(case, am, bm)
    R2 = contract(case, am * am, bm * bm)
    if add is not None:
        ref = ref + add[None, :, None, None]
        M = M + addm[None, :, None, None]
        R2 = R2 + (add * add)[None, :, None, None]
    return dict(ref=ref, M=M, R=torch.sqrt(R2))


def fp32_cpu_rms(case: Case, inp: dict, ref: dict) -> float:
    """RMS((torch float32 on one CPU thread - ref) / R): the precision the kernels are held to (same operands, fp32 arithmetic)."""
    import torch
    a, b, add = operands(case, inp)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = contract(case, a.float(), b.float()).double()
    finally:
        torch.set_num_threads(n)
    if add is not None:
        got = got + add.float().double()[None, :, None, None]
    return rel_rms(got, ref)


def rel_rms(got, ref: dict) -> float:
    import torch
    R = ref["R"]
    m = R > 0
    if not bool(m.any()):
        return 0.0
    e = ((got.double() - ref["ref"]) / torch.where(m, R, torch.ones_like(R)))[m]
    return float(torch.sqrt((e * e).mean()))


def check(got, ref: dict, tau: float, base_rms: float) -> Tuple[bool, dict]:
    """The bar: pointwise |got - ref| <= tau * M (wrong, missing or doubled terms, borders included), and the precision
    RMS((got - ref) / R) <= RMS_FACTOR * base_rms + RMS_FLOOR (a lost operand piece averages out pointwise at large K, not here)."""
    import torch
    got = got.double()
    err = (got - ref["ref"]).abs()
    M = ref["M"]
    finite = bool(torch.isfinite(got).all())
    ratio = float(torch.where(M > 0, err / torch.where(M > 0, M, torch.ones_like(M)), torch.where(err > 0, float("inf"), 0.0)).max()) if finite else float("inf")
    rms = rel_rms(got, ref) if finite else float("inf")
    ok = finite and ratio <= tau and rms <= RMS_FACTOR * base_rms + RMS_FLOOR
    return ok, dict(max_err_over_M=ratio, rms=rms, fp32_rms=base_rms)


def round_bits(t, bits: int):
    """t (float64) rounded to `bits` significant bits."""
    import torch
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def pieces(t, bits: int, n: int):
    """The sum of the first n pieces of a split of t into `bits`-bit pieces (fp16: 11, bf16: 8)."""
    out = t * 0
    r = t
    for _ in range(n):
        p = round_bits(r, bits)
        out = out + p
        r = r - p
    return out
