"""The form of the fused input gradient + fold of up4's first convolution (csrc/up_bwd_row.hip), on the CPU: the host predicate accepts a
size only where the float32 index rule of the x2 align_corners interpolation gives the four-tap support 2 i - 1 .. 2 i + 2 that the
kernel's fold assumes, it reports that support the way a NumPy float32 restatement of resample.hip's tap_weight does, and the kernel's
symbol stays outside the table of tests/test_conv_form_table.py."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import test_conv_form_table as T

OK, ENOFORM, EINVAL = 0, -4, -1


def support_np(n_in: int):
    """(min, max) of o - 2 i over every (output index o, input index i) with a non-zero tap_weight, in float32 as the kernels
    evaluate it: sx = fl(r * o), i0 = (int)sx, i1 = i0 + (i0 < n_in - 1), l1 = fl(sx - i0), l0 = fl(1 - l1)."""
    n_out = 2 * n_in
    r = np.float32(n_in - 1) / np.float32(n_out - 1)
    o = np.arange(n_out)
    sx = (r * o.astype(np.float32)).astype(np.float32)
    i0 = sx.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (sx - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    same = i0 == i1
    w0 = np.where(same, (l0 + l1).astype(np.float32), l0)
    w1 = np.where(same, np.float32(0), l1)
    d = np.concatenate([(o - 2 * i0)[w0 != 0], (o - 2 * i1)[w1 != 0]])
    return int(d.min()), int(d.max())


def _support(L, n_in):
    lo, hi = C.c_int(), C.c_int()
    assert L.uaps_up_fold_support(n_in, C.byref(lo), C.byref(hi)) == OK
    return lo.value, hi.value


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    return _lib.lib()


def test_the_support_is_reported_as_the_float32_rule_gives_it(L):
    for n_in in [1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 31, 64, 100, 128, 255, 256, 333, 512, 1000, 4096] + list(range(8, 513, 8)):
        assert _support(L, n_in) == support_np(n_in), n_in
    assert L.uaps_up_fold_support(0, C.byref(C.c_int()), C.byref(C.c_int())) == EINVAL
    assert L.uaps_up_fold_support(8, None, None) == EINVAL


def test_the_predicate_accepts_only_the_four_tap_support(L):
    four = lambda n: (lambda s: s[0] >= -1 and s[1] <= 2)(support_np(n))
    assert four(128), "the 256-wide row itself folds with four taps"
    accepted = 0
    for H in range(16, 1025, 16):
        want = OK if four(H // 2) and four(128) else ENOFORM
        assert L.uaps_up_bwd_fused_form(H, 256) == want, H
        accepted += want == OK
    assert accepted > 0
    for H, W in ((24, 256), (8, 256), (16, 128), (16, 512), (16, 255)):
        assert L.uaps_up_bwd_fused_form(H, W) == ENOFORM, (H, W)
    assert L.uaps_up_bwd_fused_form(0, 256) == EINVAL
    # the sizes the benchmark and the trainer tests run at
    for H in (16, 32, 48, 256):
        assert L.uaps_up_bwd_fused_form(H, 256) == OK, H


def test_the_grid_is_one_workgroup_per_run_up_to_one_per_cu(L):
    assert L.uaps_up_bwd_fused_grid(1, 16) == 1
    assert L.uaps_up_bwd_fused_grid(32, 256) == 256
    assert L.uaps_up_bwd_fused_grid(300, 16) == 256
    assert L.uaps_up_bwd_fused_grid(2, 24) == EINVAL


def test_the_kernel_is_not_a_case_of_the_conv_form_table():
    """tests/test_conv_form_table.py wants a case for every conv_*kernel(ConvFwdArgs | ConvWrwArgs): this kernel has its own argument
    struct and name, and is tested by tests/test_gpu_up_fold_fused.py."""
    from uaps_amd import _lib
    tmp = tempfile.mkdtemp(prefix="uaps_syms_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_lib.LIB_PATH, local)
        subprocess.run([os.path.join(T.LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        found = []
        for o in sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950*"))):
            out = subprocess.run([os.path.join(T.LLVM, "llvm-readelf"), "-sW", "--demangle", o], check=True, stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, text=True).stdout
            for line in out.splitlines():
                cols = line.split(None, 7)
                if len(cols) == 8 and cols[3] == "FUNC" and "up_bwd_row_kernel" in cols[7]:
                    found.append(cols[7].strip())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert set(found) == {"uaps::up_bwd_row_kernel(uaps::UpBwdArgs)"}, found      # (listed by both symbol tables)
    assert not T._KERNEL.match(found[0])
