"""CCT / DCT on the host (no GPU): argument checks of the new C entry points -- each bad call returns before any HIP call, so fake
non-null device pointers are never dereferenced -- the CCT network, the ramp the two trainers follow (CCT/CCT_train.py,
DCT/DCT_train.py) and DCTTrainer's rotation stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from uaps_amd import _lib

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
P = 4096                        # a non-null "device" pointer: the calls below must refuse before touching it


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _arr(vals):
    return (C.c_void_p * len(vals))(*vals)


def _ws(L):
    n = C.c_size_t()
    assert L.uaps_cct_dct_workspace_bytes(C.byref(n)) == 0 and n.value >= 1024 * 8 * 4
    assert L.uaps_cct_dct_workspace_bytes(None) == EINVAL
    return n.value


def test_cct_consistency_refuses_bad_arguments(L):
    ws = _ws(L)

    def fwd(heads=None, D=4, b0=0, B=2, Cc=4, H=8, W=8, out=P, w=P, wb=None):
        h = _arr([P] * 8) if heads is None else heads
        return L.uaps_cct_consistency_fwd(h, D, b0, B, Cc, H, W, out, w, ws if wb is None else wb, None)
    assert L.uaps_cct_consistency_fwd(None, 4, 0, 2, 4, 8, 8, P, P, ws, None) == EINVAL
    assert fwd(out=None) == EINVAL
    assert fwd(heads=_arr([P, P, None, P])) == EINVAL                      # a null head
    for bad in ({"D": 1}, {"D": 9}, {"D": 0}, {"b0": -1}, {"B": 0}, {"H": 0}, {"W": -3}):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(B=64, Cc=8, H=1024, W=1024) == ERANGE                        # 2 GiB of fp32
    assert fwd(b0=60, B=4, Cc=8, H=1024, W=1024) == ERANGE                  # the window's end counts
    assert fwd(w=None) == EWORKSPACE and fwd(wb=16) == EWORKSPACE

    def bwd(heads=None, D=4, b0=0, B=2, Cc=4, H=8, W=8, g=P, dheads=None):
        h = _arr([P] * 8) if heads is None else heads
        d = _arr([P] * 8) if dheads is None else dheads
        return L.uaps_cct_consistency_bwd(h, D, b0, B, Cc, H, W, g, d, None)
    assert L.uaps_cct_consistency_bwd(None, 4, 0, 2, 4, 8, 8, P, _arr([P] * 4), None) == EINVAL
    assert L.uaps_cct_consistency_bwd(_arr([P] * 4), 4, 0, 2, 4, 8, 8, P, None, None) == EINVAL
    assert bwd(g=None) == EINVAL
    assert bwd(dheads=_arr([P, P, P, None])) == EINVAL
    for bad in ({"D": 1}, {"D": 9}, {"b0": -2}, {"B": 0}, {"H": -1}, {"W": 0}):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(Cc=1) == ERANGE and bwd(B=64, Cc=8, H=1024, W=1024) == ERANGE


def test_rot90_batch_refuses_bad_arguments(L):
    def call(xl=P, xu=P, B=2, Ci=3, H=8, W=8, k=1, out=P, rot=None):
        return L.uaps_rot90_batch(xl, xu, B, Ci, H, W, k, out, rot, None)
    for bad in ({"xl": None}, {"xu": None}, {"out": None}, {"B": 0}, {"Ci": 0}, {"H": -1}, {"W": 0}, {"k": -1}, {"k": 4}):
        assert call(**bad) == EINVAL, bad
    assert call(H=8, W=12, k=1) == EINVAL                                   # [B, Cin, W, H] cannot share the buffer
    assert call(H=8, W=12, k=3) == EINVAL
    assert call(B=64, Ci=3, H=2048, W=2048, k=0) == ERANGE
    h = _lib.CallHints()
    h.struct_size = C.sizeof(_lib.CallHints) + 8                           # a client newer than the library
    assert L.uaps_rot90_batch_h(C.byref(h), P, P, 2, 3, 8, 8, 0, P, None, None) == EINVAL
    assert L.uaps_rot90_batch_h(None, None, P, 2, 3, 8, 8, 0, P, None, None) == EINVAL
    assert "uaps_rot90_batch" in _lib.HINTED and "uaps_rot90_batch_h" in _lib.SIGNATURES


def test_rot_consistency_refuses_bad_arguments(L):
    ws = _ws(L)

    def fwd(r=P, rb0=0, u=P, ub0=0, B=2, Cc=4, H=8, W=8, k=1, out=P, w=P, wb=None):
        return L.uaps_rot_consistency_fwd(r, rb0, u, ub0, B, Cc, H, W, k, out, w, ws if wb is None else wb, None)
    for bad in ({"r": None}, {"u": None}, {"out": None}, {"k": -1}, {"k": 4}, {"rb0": -1}, {"ub0": -1}, {"B": 0}, {"H": 0}, {"W": -1}):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(Cc=1) == ERANGE and fwd(Cc=9) == ERANGE
    assert fwd(B=64, Cc=8, H=1024, W=1024) == ERANGE
    assert fwd(w=None) == EWORKSPACE and fwd(wb=4) == EWORKSPACE

    def bwd(r=P, rb0=0, u=P, ub0=0, B=2, Cc=4, H=8, W=8, k=1, g=P, dr=P, du=P):
        return L.uaps_rot_consistency_bwd(r, rb0, u, ub0, B, Cc, H, W, k, g, dr, du, None)
    for bad in ({"r": None}, {"u": None}, {"g": None}, {"dr": None}, {"du": None}, {"k": 5}, {"k": -1}, {"ub0": -3}, {"B": 0}):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(Cc=9) == ERANGE


def test_cct_net_is_the_uaps_net_with_aux_dropout_0_3():
    from uaps_amd import net_factory
    from uaps_amd.unet import UNet_UAPS
    torch.manual_seed(0)
    a, b = net_factory("unet_cct"), net_factory("unet_uaps")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape for k in sa)
    heads = sorted({k.split(".")[0] for k in sa})
    assert heads == ["aux_decoder1", "aux_decoder2", "aux_decoder3", "encoder", "main_decoder"]       # UNet_CCT's keys
    assert a.aux_dropout_p == 0.3 and a.n_aux == 3
    assert b.aux_dropout_p == 0.5 and UNet_UAPS(3, 4).aux_dropout_p == 0.5
    with pytest.raises(ValueError):
        UNet_UAPS(3, 4, aux_dropout_p=1.0)


def test_ramp_divisor_150_and_no_gate():
    from uaps_amd import cct_dct
    from uaps_amd.ramps import sigmoid_rampup
    for cls in (cct_dct.CCTTrainer, cct_dct.DCTTrainer):
        assert cls.ramp_divisor_default == 150
        tr = cls.__new__(cls)
        tr.c1, tr.rampup, tr.ramp_divisor = 0.1, 200.0, cls.ramp_divisor_default
        for it in (0, 1, 149, 150, 151, 5 * 150 + 3, 300 * 150):
            tr.iter_num = it
            assert tr.consistency_weight() == 0.1 * sigmoid_rampup(it // 150, 200.0), (cls.__name__, it)
            assert tr.consistency_weights() == (tr.consistency_weight(), 0.0)
        tr.iter_num = 0
        assert tr.consistency_weight() > 0                                  # no iteration gate (CCT_train.py:194, DCT_train.py:186)


def _dct(seed, rank=0, monkey=None):
    from uaps_amd import cct_dct, dist
    if monkey is not None:
        monkey.setattr(dist, "rank", lambda: rank)
    return cct_dct.DCTTrainer(torch.nn.Conv2d(3, 4, 1), seed=seed)


def test_dct_rot_times_stream_is_seeded_and_survives_a_state_round_trip(monkeypatch):
    from uaps_amd.trainer import _rng_state_numpy, _rng_state_plain
    a, b = _dct(7), _dct(7)
    ka = [a.draw_rot_times() for _ in range(64)]
    assert ka == [b.draw_rot_times() for _ in range(64)]
    assert set(ka) == {0, 1, 2, 3}
    assert ka != [_dct(8).draw_rot_times() for _ in range(64)]
    assert ka != [_dct(7, rank=1, monkey=monkeypatch).draw_rot_times() for _ in range(64)]
    st = _rng_state_plain(a.rot_rng)
    nxt = [a.draw_rot_times() for _ in range(16)]
    c = _dct(99)
    c.rot_rng.set_state(_rng_state_numpy(st))
    assert [c.draw_rot_times() for _ in range(16)] == nxt
    ck = a.state_for_checkpoint(1, 0.5, dataparallel_prefix=False)
    for key in ("epoch", "best_dice_1", "state_dict", "optimizer", "rot_rng", "perturb_rng", "np_global_rng"):
        assert key in ck, key


def test_cct_dct_wrappers_refuse_cpu_tensors():
    from uaps_amd import cct_dct
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(_lib.UapsHipError):
        cct_dct.cct_consistency([z, z])
    with pytest.raises(_lib.UapsHipError):
        cct_dct.rot_consistency(z, z, 1)
    with pytest.raises(_lib.UapsHipError):
        cct_dct.rot90_batch(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), 1)
