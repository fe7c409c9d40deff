"""Mean Teacher / UAMT on the host (no GPU): argument checks of the four new C entry points -- each bad call returns before any
HIP call, so fake non-null device pointers are never dereferenced -- and the schedules the trainers follow (MT/MT_train.py,
UAMT/UA_MT_train.py)."""
import ctypes as C
import math

import pytest

from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _arr(vals, t=C.c_void_p):
    return (t * len(vals))(*vals)


def test_ema_update_refuses_bad_arguments(L):
    e, p, n = _arr([P, P]), _arr([P, P]), _arr([16, 16], C.c_long)
    assert L.uaps_ema_update(None, p, n, 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, None, n, 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, None, 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, n, 0, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, n, -1, 0.5, 0.5, None) == EINVAL
    # a bad SECOND pair: nothing is launched for the first one either
    assert L.uaps_ema_update(_arr([P, None]), p, n, 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, _arr([P, None]), n, 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, _arr([16, 0], C.c_long), 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, _arr([16, -3], C.c_long), 2, 0.5, 0.5, None) == EINVAL
    assert L.uaps_ema_update(e, p, _arr([16, 1 << 29], C.c_long), 2, 0.5, 0.5, None) == ERANGE      # 2 GiB of fp32


def test_teacher_noise_refuses_bad_arguments(L):
    for fn, extra in ((L.uaps_teacher_noise, None), (L.uaps_teacher_noise_apply, P)):
        def call(x=P, B=2, Ci=3, H=8, W=8, T=8, out=P):
            if extra is None:
                return fn(x, B, Ci, H, W, T, 1, 0, out, None)
            return fn(x, extra, B, Ci, H, W, T, out, None)
        assert call(x=None) == EINVAL
        assert call(out=None) == EINVAL
        for bad in ({"B": 0}, {"Ci": 0}, {"H": -1}, {"W": 0}, {"T": -1}, {"T": 17}):
            assert call(**bad) == EINVAL, bad
        assert call(B=64, Ci=3, H=2048, W=2048, T=8) == ERANGE        # 9 x 64 x 3 x 2048^2 floats >= 2 GiB
    assert L.uaps_teacher_noise_apply(P, None, 2, 3, 8, 8, 8, P, None) == EINVAL


def test_mc_consistency_refuses_bad_arguments(L):
    n = C.c_size_t()
    assert L.uaps_mc_consistency_workspace_bytes(C.byref(n)) == 0 and n.value >= 8
    assert L.uaps_mc_consistency_workspace_bytes(None) == EINVAL
    ws = n.value

    def fwd(s=P, e=P, mc=P, T=8, B=2, Cc=4, H=8, W=8, mask=P, unc=None, out=P, w=P, wb=None):
        return L.uaps_mc_consistency_fwd(s, e, mc, T, B, Cc, H, W, 0.5, mask, unc, out, w, ws if wb is None else wb, None)
    assert fwd(s=None) == EINVAL
    assert fwd(e=None) == EINVAL
    assert fwd(out=None) == EINVAL
    assert fwd(mask=None) == EINVAL                      # mask mode must store the mask its backward reads
    assert fwd(mc=None, T=8, mask=None) == EINVAL        # MT mode has no T
    assert fwd(mc=None, T=0, mask=None, unc=P) == EINVAL
    for bad in ({"B": 0}, {"H": 0}, {"W": -2}, {"T": -1}, {"T": 17}):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(B=64, Cc=8, H=1024, W=1024, T=16) == ERANGE
    assert fwd(w=None) == EWORKSPACE and fwd(wb=8) == EWORKSPACE

    def bwd(s=P, e=P, mask=P, g=P, out=P, B=2, Cc=4, H=8, W=8, ds=P):
        return L.uaps_mc_consistency_bwd(s, e, mask, g, out, B, Cc, H, W, ds, None)
    for bad in ({"s": None}, {"e": None}, {"g": None}, {"ds": None}, {"mask": None}, {"out": None}, {"B": 0}, {"H": -1}, {"W": 0}):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(Cc=9) == ERANGE
    assert bwd(B=128, Cc=8, H=1024, W=1024) == ERANGE


def test_pair_ops_refuse_bad_arguments(L):
    """The sibling consistency terms of pair_ops.hip (include/uaps_hip.h: C in [2, 8], any output may be NULL, the workspace is
    needed for a mean only).  Their header block promises no 2 GiB refusal, and they make none: the kernels index with 64-bit offsets."""
    n = C.c_size_t()
    assert L.uaps_pair_workspace_bytes(C.byref(n)) == 0 and n.value >= 4
    assert L.uaps_pair_workspace_bytes(None) == EINVAL
    ws = n.value

    def fwd(a=P, b=P, probs=0, B=2, Cc=4, H=8, W=8, mse=P, klm=P, mean=P, w=P, wb=None):
        return L.uaps_softmax_pair_fwd(a, b, probs, B, Cc, H, W, mse, klm, mean, w, ws if wb is None else wb, None)
    for bad in ({"a": None}, {"b": None}, {"B": 0}, {"H": 0}, {"W": -1}, {"mse": None, "klm": None, "mean": None}):
        assert fwd(**bad) == EINVAL, bad
        assert fwd(probs=1, **bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(w=None) == EWORKSPACE and fwd(wb=ws - 1) == EWORKSPACE
    assert fwd(Cc=9, w=None) == ERANGE                      # the class count is looked at before the workspace

    def mse(a=P, b=P, g=P, B=2, Cc=4, H=8, W=8, da=P):
        return L.uaps_softmax_mse_bwd(a, b, g, B, Cc, H, W, da, None)
    for bad in ({"a": None}, {"b": None}, {"g": None}, {"da": None}, {"B": 0}, {"H": -1}, {"W": 0}):
        assert mse(**bad) == EINVAL, bad
    assert mse(Cc=1) == ERANGE and mse(Cc=9) == ERANGE

    def kl(a=P, b=P, g=P, B=2, Cc=4, H=8, W=8, da=P):
        return L.uaps_softmax_kl_bwd(a, b, g, B, Cc, H, W, da, None)
    for bad in ({"a": None}, {"b": None}, {"da": None}, {"B": -1}, {"H": 0}, {"W": 0}, {"g": None, "B": 0}):
        assert kl(**bad) == EINVAL, bad
    assert kl(Cc=1) == ERANGE and kl(Cc=9, g=None) == ERANGE

    def klmap(a=P, b=P, g=P, B=2, Cc=4, H=8, W=8, da=P, db=P):
        return L.uaps_softmax_klmap_bwd(a, b, g, B, Cc, H, W, da, db, None)
    for bad in ({"a": None}, {"b": None}, {"g": None}, {"da": None, "db": None}, {"B": 0}, {"H": 0}, {"W": -3}):
        assert klmap(**bad) == EINVAL, bad
    assert klmap(Cc=1, db=None) == ERANGE and klmap(Cc=9, da=None) == ERANGE

    def ent(p=P, B=2, Cc=4, H=8, W=8, m=P, mean=P, w=P, wb=None):
        return L.uaps_entropy_map(p, B, Cc, H, W, m, mean, w, ws if wb is None else wb, None)
    for bad in ({"p": None}, {"B": 0}, {"H": 0}, {"W": 0}, {"m": None, "mean": None}):
        assert ent(**bad) == EINVAL, bad
    assert ent(Cc=1) == ERANGE and ent(Cc=9) == ERANGE
    assert ent(w=None) == EWORKSPACE and ent(wb=0) == EWORKSPACE and ent(m=None, wb=ws - 1) == EWORKSPACE


def test_ema_alpha_schedule():
    from uaps_amd.mean_teacher import ema_alpha
    assert ema_alpha(0.99, 0) == (0.0, 1.0)                   # step 0: the teacher becomes a copy of the student
    for k in (1, 5, 50, 98, 99, 100, 500, 10 ** 6):
        a, oma = ema_alpha(0.99, k)
        assert a == min(1 - 1 / (k + 1), 0.99) and oma == 1.0 - a, k
    assert ema_alpha(0.99, 1) == (0.5, 0.5)
    assert ema_alpha(0.999, 10 ** 6)[0] == 0.999


def test_uamt_threshold_and_ramp_divisors():
    from uaps_amd import mean_teacher as mt
    from uaps_amd.ramps import sigmoid_rampup
    for cw in (0.0, 0.001, 0.05, 0.1):
        assert mt.uamt_threshold(cw) == pytest.approx((0.75 + 2.5 * cw) * math.log(2), rel=1e-15)
    assert mt.UAMTTrainer.ramp_divisor_default == 80 and mt.MeanTeacherTrainer.ramp_divisor_default == 150
    # the trainers' schedule objects without a model: the weight as UA_MT_train.py:74-76 / MT_train.py:75-77 form it
    for cls, div in ((mt.UAMTTrainer, 80), (mt.MeanTeacherTrainer, 150)):
        tr = cls.__new__(cls)
        tr.c1, tr.rampup, tr.ramp_divisor = 0.1, 200.0, cls.ramp_divisor_default
        for it in (0, div - 1, div, 5 * div + 3, 300 * div):
            tr.iter_num = it
            assert tr.consistency_weight() == 0.1 * sigmoid_rampup(it // div, 200.0), (cls.__name__, it)


def test_mt_consistency_gate():
    from uaps_amd import mean_teacher as mt
    assert mt.MeanTeacherTrainer.gate_iters == 1000 and mt.UAMTTrainer.gate_iters == 0
    tr = mt.MeanTeacherTrainer.__new__(mt.MeanTeacherTrainer)
    tr.gate_iters = 1000
    for it, open_ in ((0, False), (999, False), (1000, True), (5000, True)):
        tr.iter_num = it
        assert tr.gated_weight(0.25) == (0.25 if open_ else 0.0), it
    tr = mt.UAMTTrainer.__new__(mt.UAMTTrainer)
    tr.iter_num = 0
    assert tr.gated_weight(0.25) == 0.25


def test_uamt_trainer_refuses_odd_or_too_many_passes():
    import torch
    from uaps_amd import mean_teacher as mt
    m = torch.nn.Linear(2, 2)
    for T in (0, 3, 18):
        with pytest.raises(ValueError):
            mt.UAMTTrainer(m, m, T=T)


def test_mc_consistency_refuses_cpu_tensors():
    import torch
    from uaps_amd import mean_teacher as mt
    s = torch.zeros(1, 4, 4, 4)
    with pytest.raises(_lib.UapsHipError):
        mt.mc_consistency(s, s)
    with pytest.raises(_lib.UapsHipError):
        mt.teacher_inputs(torch.zeros(1, 3, 4, 4), 8)
