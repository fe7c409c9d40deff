"""The table of convolution kernel forms (tests/conv_form_cases.py), on the CPU: every case resolves to the kernel it names, the
cases and the UNREACHABLE list together cover every conv compute kernel of the built code object, a planner sweep reaches no
UNREACHABLE kernel, and the float64 bar of tests/test_gpu_conv_forms.py passes correct emulated arithmetic and fails each of a set
of subtle emulated mistakes."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

import conv_form_cases as F
from conv_form_cases import BWD_DATA, FWD, WRW

LLVM = "/opt/rocm/lib/llvm/bin"
# the compute kernels of the forward / input-gradient and weight-gradient forms: every __global__ taking ConvFwdArgs / ConvWrwArgs
# (packing, weight scaling and the reductions take other argument structs)
_KERNEL = re.compile(r"^(?:void )?uaps::(conv_[a-z0-9_]*kernel(?:<[^>]*>)?)\(uaps::Conv(?:Fwd|Wrw)Args\)$")


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    lib = _lib.lib()
    lib.uaps_conv_get_tuning.restype = C.c_uint
    prev = (lib.uaps_conv_get_mode(), lib.uaps_conv_get_tuning())
    yield lib
    lib.uaps_conv_set_mode(prev[0])
    lib.uaps_conv_set_tuning(prev[1])


def conv_kernel_symbols(so_path: str) -> set:
    """Demangled names of the conv compute kernels in the gfx950 code objects of so_path (extracted as tools/isa_lint.py does)."""
    tmp = tempfile.mkdtemp(prefix="uaps_syms_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(so_path, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs = sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950*")))
        assert objs, "no gfx950 code object in " + so_path
        names = set()
        for o in objs:
            out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", "--demangle", o], check=True, stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, text=True).stdout
            for line in out.splitlines():
                cols = line.split(None, 7)
                if len(cols) == 8 and cols[3] == "FUNC":
                    m = _KERNEL.match(cols[7].strip())
                    if m:
                        names.add(m.group(1))
        return names
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_every_case_resolves_to_its_named_kernel(L):
    """A planner change that moves a case onto another kernel fails here, instead of the GPU test silently testing something else."""
    from uaps_amd import _lib
    wrong = [(c.id, F.variant(L, _lib, c)) for c in F.CASES if F.variant(L, _lib, c) != c.kernel]
    assert not wrong, wrong
    assert len({c.id for c in F.CASES}) == len(F.CASES)
    assert any(c.out_amax for c in F.CASES) and any(c.bsum for c in F.CASES) and any(c.dyt for c in F.CASES) and any(c.up2 for c in F.CASES)
    ENOFORM = -4
    assert all(F.variant(L, _lib, c) == ENOFORM for c in F.OUT_AMAX_REFUSED)


def test_cases_and_unreachable_cover_every_conv_kernel_of_the_code_object():
    from uaps_amd import _lib
    built = conv_kernel_symbols(_lib.LIB_PATH)
    assert len(built) > 200, len(built)
    named = {c.kernel for c in F.CASES}
    assert not (named & set(F.UNREACHABLE)), "a kernel with a case is listed as unreachable"
    assert all(len(r) > 20 for r in F.UNREACHABLE.values())
    untested = sorted(built - named - set(F.UNREACHABLE))
    assert not untested, f"{len(untested)} conv kernels without a case (add one to conv_form_cases.CASES, or to UNREACHABLE with the reason): {untested}"
    stale = sorted((named | set(F.UNREACHABLE)) - built)
    assert not stale, f"cases / UNREACHABLE entries for kernels the code object does not hold: {stale}"


def test_no_call_of_a_planner_sweep_reaches_an_unreachable_kernel(L):
    from uaps_amd import _lib
    reached, n = set(), 0
    for c in F.sweep():
        v = F.variant(L, _lib, c)
        n += 1
        if isinstance(v, str):
            reached.add(v)
    assert n > 100000
    assert not (reached & set(F.UNREACHABLE)), sorted(reached & set(F.UNREACHABLE))
    # the sweep is broad: it reaches almost every named kernel by itself
    named = {c.kernel for c in F.CASES}
    assert len(reached & named) >= len(named) - 10


# ---- the bar against emulated arithmetic ----------------------------------------------------------------------------------------

def _pick(pred):
    for c in F.CASES:
        if pred(c):
            return c
    raise AssertionError("no such case in the table")


def _discrimination_cases():
    return {
        "fwd_cat": _pick(lambda c: c.op == FWD and c.two_in and not c.up2 and c.ks == 3 and c.W % 32),
        "fwd_bn": _pick(lambda c: c.op == FWD and c.xf is not None and c.xf[1] > 1 and c.ks == 3 and c.Cin >= 16 and c.H % 8),
        "bwd": _pick(lambda c: c.op == BWD_DATA and c.ks == 3 and c.H % 8 and c.W % 32 and c.Cout >= 16),
        "wrw": _pick(lambda c: c.op == WRW and c.ks == 3 and c.dyt is None and not c.up2 and c.B > 1 and c.H % 4),
    }


def _bar(case, inp, ref, got):
    tau = F.TAU_DW if case.op == WRW else F.TAU_Y
    return F.check(got, ref, tau, F.fp32_cpu_rms(case, inp, ref))


@pytest.mark.parametrize("which", ["fwd_cat", "fwd_bn", "bwd", "wrw"])
def test_the_bar_passes_correct_arithmetic_and_fails_subtle_mistakes(which):
    case = _discrimination_cases()[which]
    inp = F.make_inputs(case)
    ref = F.reference(case, inp, floors=F.h16_floors(case, inp))
    ok, st = _bar(case, inp, ref, F.reference(case, inp, rounding=lambda v: F.pieces(v, 11, 2))["ref"])
    assert ok, ("two fp16 pieces (22 significant bits) must pass", st)
    # fp32 arithmetic: the operands rounded to 24 significant bits (the staged BatchNorm output is not an fp32 value) and the
    # contraction evaluated in float32 on the CPU -- products and sums rounded as the exact fp32 kernels round them
    a, b, add = F.operands(case, inp)
    got32 = F.contract(case, F.round_bits(a, 24).float(), F.round_bits(b, 24).float()).double()
    if add is not None:
        got32 = got32 + add[None, :, None, None]
    ok, st = _bar(case, inp, ref, got32)
    assert ok, ("fp32 arithmetic must pass", st)
    assert st["max_err_over_M"] > 0                # (not the reference itself)
    mutants = {
        "the high fp16 piece only": F.reference(case, inp, rounding=lambda v: F.pieces(v, 11, 1))["ref"],
        "two bf16 pieces only": F.reference(case, inp, rounding=lambda v: F.pieces(v, 8, 2))["ref"],
    }
    if case.op != WRW:
        got = ref["ref"].clone()                   # one 3x3 tap missing on the right border column (the middle-row tap that reads inside the map)
        inp2 = dict(inp)
        w = inp["w"].clone()
        w[..., 1, 0 if case.op == FWD else 2] = 0.0
        inp2["w"] = w
        got[..., -1] = F.reference(case, inp2)["ref"][..., -1]
        mutants["a tap missing on the border column"] = got
        got = ref["ref"].clone()
        th, tw = case.H % 8 or 8, case.W % 32 or (case.W % 16 or 16)
        got[..., -th:, -tw:] = 0.0
        mutants["the last partial tile zeroed"] = got
    if case.two_in:
        inp2 = dict(inp)
        x = inp["x"].clone()
        x[:, [case.C1 - 1, case.C1]] = x[:, [case.C1, case.C1 - 1]]
        inp2["x"] = x
        mutants["x2[0] and x[Csplit - 1] swapped"] = F.reference(case, inp2)["ref"]
    if case.xf is not None and case.xf[1] > 1:
        inp2 = dict(inp)
        xf = inp["xf"].clone()
        xf[1] = xf[0]
        inp2["xf"] = xf
        mutants["BatchNorm group 0's coefficients on group 1"] = F.reference(case, inp2)["ref"]
    if case.op == WRW:
        a, b, _ = F.operands(case, inp)
        part = torch.zeros_like(a)
        part[case.B - 1, :, :4] = a[case.B - 1, :, :4]
        mutants["one pixel split of the reduction dropped"] = ref["ref"] - F.contract(case, part, b)
    assert len(mutants) >= 3
    for what, got in mutants.items():
        ok, st = _bar(case, inp, ref, got)
        assert not ok, (which, what, "passed the bar", st)
