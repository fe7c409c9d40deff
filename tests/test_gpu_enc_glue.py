"""-m gpu: the encoder's glue launches folded into their neighbours (include/uaps_hip.h, "Encoder glue"), each against the two
launches it replaces, on the same operands, through the C ABI, bit for bit:
  * uaps_fanin_perturbed_bn_sums_h + uaps_bn_act_bwd_partials_h  ==  uaps_fanin_perturbed + uaps_bn_act_bwd_grouped_bias_h
  * uaps_bn_act_fwd_train_partials_pool_h                        ==  uaps_bn_act_fwd_train_partials_h + uaps_maxpool2x2_fwd
The replaced launches are held against float64 by tests/test_gpu_ops_forms.py and tests/test_gpu_bn_forms.py; equality carries their
accuracy over.  Then the host side: the record that carries the sums from the fan-in to the BatchNorm node, and whole training steps."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOFORM = -4
SENTINEL = -12345.678
SLOPE = 0.01


def _L():
    from uaps_amd import _lib
    return _lib.lib()


def _st():
    from uaps_amd import _lib
    return _lib.current_stream(torch.device(DEV))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _t(rng, shape, scale=1.0):
    return torch.tensor((rng.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


# ---- fan-in that also forms the BatchNorm-backward sums --------------------------------------------------------------------------

def _fan_case(B, groups, Cc, H, W, modes, seed, off0=1000):
    rng = np.random.default_rng(seed)
    s = dict(B=B, groups=groups, C=Cc, H=H, W=W, modes=list(modes), n=len(modes), seed=0x1234567890ABCDEF ^ seed)
    g, keep, offs = [], [], []
    for k, m in enumerate(modes):
        if m == 4:
            g.append(_t(rng, (B, Cc, H // 2, W // 2)))
            keep.append(torch.tensor(rng.integers(0, 4, (B, Cc, H // 2, W // 2)).astype(np.uint8)).to(DEV))
        else:
            g.append(_t(rng, (B, Cc, H, W)))
            keep.append(torch.tensor(rng.integers(0, 2, (B, H, W)).astype(np.uint8)).to(DEV) if m == 3 else None)
        offs.append([off0 + 7919 * (k * groups + q) for q in range(groups)])
    s.update(g=g, keep=keep, offs=offs)
    s["y"] = _t(rng, (B, Cc, H, W), 2.0)
    s["mean"] = _t(rng, (groups * Cc,), 0.3)
    s["invstd"] = torch.tensor(rng.uniform(0.3, 1.5, groups * Cc).astype(np.float32)).to(DEV)
    s["gamma"] = torch.tensor(rng.uniform(0.5, 1.5, Cc).astype(np.float32) * rng.choice([-1.0, 1.0], Cc).astype(np.float32)).to(DEV)
    s["beta"] = _t(rng, (Cc,), 0.5)
    s["nch"] = (H * W + 4095) // 4096
    return s


def _fan_args(s):
    n, G = s["n"], s["groups"]
    return ((C.c_void_p * n)(*[t.data_ptr() for t in s["g"]]), (C.c_int * n)(*s["modes"]),
            (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in s["keep"]]),
            (C.c_uint64 * (n * G))(*[o for row in s["offs"] for o in row]), n, G, s["seed"], 0.3, 0.5, s["B"], s["C"], s["H"], s["W"])


def _bn_ws(s):
    n = C.c_size_t()
    assert _L().uaps_bn_workspace_bytes(s["B"], s["C"], s["H"], s["W"], C.byref(n)) == 0
    return torch.zeros(n.value, dtype=torch.uint8, device=DEV)


def _dx_outputs(s):
    from uaps_amd import bounds
    return dict(dy=torch.full_like(s["y"], SENTINEL), dgamma=torch.full((s["C"],), SENTINEL, device=DEV),
                dbeta=torch.full((s["C"],), SENTINEL, device=DEV), dcb=torch.full((s["C"],), SENTINEL, device=DEV),
                am=bounds.new_amax(torch.device(DEV)))


def _two_launches(s):
    from uaps_amd import _lib
    L, B, Cc, H, W = _L(), s["B"], s["C"], s["H"], s["W"]
    out = torch.full_like(s["y"], SENTINEL)
    assert L.uaps_fanin_perturbed(*_fan_args(s), out.data_ptr(), _st()) == 0
    o, ws = _dx_outputs(s), _bn_ws(s)
    rc = L.uaps_bn_act_bwd_grouped_bias_h(_lib.mk_hints((), o["am"]), out.data_ptr(), s["y"].data_ptr(), s["gamma"].data_ptr(), s["beta"].data_ptr(),
                                          s["mean"].data_ptr(), s["invstd"].data_ptr(), SLOPE, 0.0, 0, 0, B, Cc, H, W, s["groups"],
                                          o["dy"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), o["dcb"].data_ptr(),
                                          ws.data_ptr(), ws.numel(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    partials = ws[:Cc * B * s["nch"] * 8].view(torch.float32).view(Cc, B, s["nch"], 2).clone()      # the workspace starts with them
    return dict(out=out, partials=partials, **o)


def _fused(s, out=None, partials=None):
    from uaps_amd import _lib
    L, B, Cc, H, W = _L(), s["B"], s["C"], s["H"], s["W"]
    out = torch.full_like(s["y"], SENTINEL) if out is None else out
    partials = torch.full((Cc, B, s["nch"], 2), SENTINEL, device=DEV) if partials is None else partials
    rc = L.uaps_fanin_perturbed_bn_sums_h(None, *_fan_args(s), out.data_ptr(), s["y"].data_ptr(), s["gamma"].data_ptr(), s["beta"].data_ptr(),
                                          s["mean"].data_ptr(), s["invstd"].data_ptr(), SLOPE, partials.data_ptr(), _st())
    assert rc == 0
    o = _dx_outputs(s)
    rc = L.uaps_bn_act_bwd_partials_h(_lib.mk_hints((), o["am"]), partials.data_ptr(), s["nch"], out.data_ptr(), s["y"].data_ptr(),
                                      s["gamma"].data_ptr(), s["beta"].data_ptr(), s["mean"].data_ptr(), s["invstd"].data_ptr(), SLOPE, B, Cc, H, W,
                                      s["groups"], o["dy"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), o["dcb"].data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return dict(out=out, partials=partials, **o)


def _check_fan(s):
    ref, got = _two_launches(s), _fused(s)
    assert not (ref["out"] == SENTINEL).any() and not (ref["dy"] == SENTINEL).any()
    for k in ("out", "partials", "dy", "dgamma", "dbeta", "dcb", "am"):
        assert _same(ref[k], got[k]), k
    assert float(ref["am"].max()) > 0.0
    # a second launch into re-dirtied buffers: the same bits
    got["out"].fill_(7.0), got["partials"].fill_(7.0)
    again = _fused(s, got["out"], got["partials"])
    for k in ("out", "partials", "dy", "dgamma", "dbeta", "dcb", "am"):
        assert _same(ref[k], again[k]), k


FAN_SHAPES = {
    "one_short_chunk": (4, 2, 3, 8, 8, (0, 1, 2, 3)),
    "chunk_and_tail": (2, 1, 5, 72, 64, (0, 3, 1, 2, 4)),
    "four_groups_all_modes": (4, 4, 2, 16, 16, (0, 1, 2, 3, 4)),
}


@pytest.mark.parametrize("name", list(FAN_SHAPES))
def test_fan_in_with_sums_equals_the_two_launches_and_repeats(name):
    B, G, Cc, H, W, modes = FAN_SHAPES[name]
    _check_fan(_fan_case(B, G, Cc, H, W, modes, seed=len(name)))


def test_fan_in_with_a_philox_offset_that_carries_into_the_high_word():
    s = _fan_case(4, 2, 3, 8, 8, (0, 1, 2, 3), seed=3, off0=(1 << 32) - 2 * 7919 - 20)      # FeatureNoise, group 0: counters 2^32 - 20 ... 2^32 + 27
    _check_fan(s)


@pytest.mark.parametrize("what", ["out", "y", "gradient"])
def test_fan_in_with_sums_refuses_a_misaligned_pointer(what):
    s = _fan_case(2, 1, 3, 8, 8, (0, 1, 2), seed=5)
    L = _L()
    buf = torch.full((s["y"].numel() + 8,), SENTINEL, device=DEV)
    partials = torch.full((s["C"], s["B"], s["nch"], 2), SENTINEL, device=DEV)
    out_ptr, y_ptr = buf.data_ptr(), s["y"].data_ptr()
    if what == "out":
        out_ptr += 4
    elif what == "y":
        ybuf = torch.zeros(s["y"].numel() + 8, device=DEV)
        y_ptr = ybuf.data_ptr() + 4
    else:
        gbuf = torch.zeros(s["y"].numel() + 8, device=DEV)
        s["g"][1] = gbuf[1:1 + s["y"].numel()]
    rc = L.uaps_fanin_perturbed_bn_sums_h(None, *_fan_args(s), out_ptr, y_ptr, s["gamma"].data_ptr(), s["beta"].data_ptr(),
                                          s["mean"].data_ptr(), s["invstd"].data_ptr(), SLOPE, partials.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == ENOFORM
    assert bool((buf == SENTINEL).all()) and bool((partials == SENTINEL).all())


# ---- BatchNorm apply pass that also writes the 2x2 max-pool ----------------------------------------------------------------------

def _pool_case(B, Cc, H, W, groups, seed, plant=True):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B, Cc, H, W)).astype(np.float32)
    # the statistics come as partials (one part per image) of the clean tensor: the planted values below never reach them
    partials = np.stack([y.sum(axis=(2, 3)), (y * y).sum(axis=(2, 3))], axis=-1).transpose(1, 0, 2)[:, :, None, :]      # [C, B, 1, 2]
    if plant:
        y[0, 0, 0:2, 0:2] = 1.5                              # a four-way tie: the first position wins
        y[0, 0, 0:2, 2:4] = [[-9.0, 2.5], [2.5, -9.0]]      # a tie of positions 1 and 2
        y[0, 1, 2:4, 4:6] = -np.inf                          # gamma > 0: the window is -inf after BatchNorm + LeakyReLU
        y[1, 0, 0:2, 6:8] = [[0.1, np.nan], [0.2, 0.3]]      # one NaN
        y[1, 1, 2:4, 0:2] = [[np.nan, 0.1], [np.nan, 9.0]]   # two NaNs: the later one is kept
        y[B - 1, Cc - 1, H - 2:, W - 2:] = [[1.0, 1.0], [3.0, 3.0]]      # the last window of the tensor, a tie in its second row
    return dict(B=B, C=Cc, H=H, W=W, groups=groups, y=torch.tensor(y).to(DEV), partials=torch.tensor(np.ascontiguousarray(partials)).to(DEV),
                gamma=torch.tensor(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).to(DEV), beta=_t(rng, (Cc,), 0.5),
                cbias=_t(rng, (Cc,), 0.1))


def _bn_fwd(s, pool, out=None, pooled=None, idx=None):
    L, B, Cc, H, W = _L(), s["B"], s["C"], s["H"], s["W"]
    r = dict(out=torch.full_like(s["y"], SENTINEL) if out is None else out,
             mean=torch.full((s["groups"] * Cc,), SENTINEL, device=DEV), invstd=torch.full((s["groups"] * Cc,), SENTINEL, device=DEV),
             rm=torch.full((Cc,), 0.25, device=DEV), rv=torch.full((Cc,), 0.75, device=DEV), nbt=torch.full((1,), 3, dtype=torch.int64, device=DEV),
             pooled=torch.full((B, Cc, H // 2, W // 2), SENTINEL, device=DEV) if pooled is None else pooled,
             idx=torch.full((B, Cc, H // 2, W // 2), 77, dtype=torch.uint8, device=DEV) if idx is None else idx)
    ws = _bn_ws(s)
    args = (None, s["partials"].data_ptr(), 1, s["y"].data_ptr(), s["cbias"].data_ptr(), s["gamma"].data_ptr(), s["beta"].data_ptr(),
            r["rm"].data_ptr(), r["rv"].data_ptr(), r["nbt"].data_ptr(), 0.1, 1e-5, SLOPE, 0.0, 0, 0, B, Cc, H, W, s["groups"],
            r["out"].data_ptr(), r["mean"].data_ptr(), r["invstd"].data_ptr(), ws.data_ptr(), ws.numel(), _st())
    if pool:
        r["rc"] = L.uaps_bn_act_fwd_train_partials_pool_h(*args, r["pooled"].data_ptr(), r["idx"].data_ptr())
    else:
        r["rc"] = L.uaps_bn_act_fwd_train_partials_h(*args)
        if r["rc"] == 0:
            r["rc"] = L.uaps_maxpool2x2_fwd(r["out"].data_ptr(), B, Cc, H, W, r["pooled"].data_ptr(), r["idx"].data_ptr(), _st())
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("shape", [(2, 3, 4, 8, 1), (2, 2, 72, 64, 2)])
def test_apply_with_pool_equals_apply_then_pool(shape):
    B, Cc, H, W, G = shape
    s = _pool_case(B, Cc, H, W, G, seed=H)
    ref, got = _bn_fwd(s, False), _bn_fwd(s, True)
    assert ref["rc"] == 0 and got["rc"] == 0
    for k in ("out", "pooled", "idx", "mean", "invstd", "rm", "rv", "nbt"):
        assert _same(ref[k], got[k]), k
    # the planted windows, spelled out (torch's rules: first maximum in scan order, a NaN replaces what came before it)
    idx, pooled = got["idx"].cpu(), got["pooled"].cpu()
    assert idx[0, 0, 0, 0] == 0 and idx[0, 0, 0, 1] == 1
    assert idx[0, 1, 1, 2] == 0 and pooled[0, 1, 1, 2] == -np.inf
    assert idx[1, 0, 0, 3] == 1 and torch.isnan(pooled[1, 0, 0, 3])
    assert idx[1, 1, 1, 0] == 2 and torch.isnan(pooled[1, 1, 1, 0])
    assert idx[B - 1, Cc - 1, H // 2 - 1, W // 2 - 1] == 2
    # and again into re-dirtied outputs
    got["out"].fill_(7.0), got["pooled"].fill_(7.0), got["idx"].fill_(9)
    again = _bn_fwd(s, True, got["out"], got["pooled"], got["idx"])
    for k in ("out", "pooled", "idx"):
        assert _same(ref[k], again[k]), k


@pytest.mark.parametrize("H,W", [(4, 12), (3, 8)])
def test_apply_with_pool_refuses_other_shapes_and_writes_nothing(H, W):
    s = _pool_case(2, 3, H, W, 1, seed=1, plant=False)
    r = _bn_fwd(s, True)
    assert r["rc"] == ENOFORM
    for k in ("out", "pooled", "mean", "invstd"):
        assert bool((r[k] == SENTINEL).all()), k
    assert bool((r["idx"] == 77).all()) and bool((r["rm"] == 0.25).all()) and bool((r["rv"] == 0.75).all()) and int(r["nbt"]) == 3


# ---- the record between the fan-in and the BatchNorm node ------------------------------------------------------------------------

def _block_backward(glue, scope=True, hook=False, second_consumer=False):
    """ConvBlock -> feature fan-out (two perturbed copies + the pooled map) -> a weighted sum; the gradients of the block's parameters
    and of its input, and how many sums records the fan-in handed up."""
    import contextlib
    from uaps_amd import fused, lazybn, perturb, unet
    torch.manual_seed(2)
    blk = unet.ConvBlock(3, 8, 0.1).to(DEV).train()
    rng = np.random.default_rng(8)
    x = _t(rng, (4, 3, 16, 32)).requires_grad_(True)
    ws = [_t(rng, (4, 8, 16, 32)) for _ in range(3)] + [_t(rng, (4, 8, 8, 16))]
    seen = []
    prev, before = fused.ENC_GLUE, lazybn.sums_total()
    fused.ENC_GLUE = glue
    try:
        perturb.manual_seed(7, 0)
        np.random.seed(7)
        with (lazybn.scope() if scope else contextlib.nullcontext()), fused.stat_groups(2):
            f = blk(x, feature="pool")
            assert (getattr(f, "_uaps_bn_src", None) is not None) == glue
            if hook:
                f.register_hook(lambda g: seen.append(g.clone()))
            fan = perturb.perturbed_fan_out(f, ("noise", "dropout"), 2, 0.3, with_pool=True, sole_consumer=True)
            loss = sum((a * w).sum() for a, w in zip(fan, ws))
            if second_consumer:
                loss = loss + (f * ws[0]).sum()
            loss.backward()
    finally:
        fused.ENC_GLUE = prev
    torch.cuda.synchronize()
    grads = [x.grad] + [p.grad for p in blk.parameters()]
    return grads, lazybn.sums_total() - before, seen, [b.clone() for b in blk.buffers()]


def test_block_backward_with_the_record_equals_the_separate_launches():
    ref, n_ref, _, buf_ref = _block_backward(False)
    got, n_got, _, buf_got = _block_backward(True)
    assert n_ref == 0 and n_got == 1
    for a, b in zip(ref + buf_ref, got + buf_got):
        assert _same(a, b)
    # outside a trainer's scope the pooled map still comes from the apply pass, the sums from their own launch
    loose, n_loose, _, _ = _block_backward(True, scope=False)
    assert n_loose == 0
    for a, b in zip(ref, loose):
        assert _same(a, b)


def test_a_hook_on_the_feature_gets_the_plain_path_and_the_true_gradient():
    ref, _, seen_ref, _ = _block_backward(False, hook=True)
    got, n_got, seen, _ = _block_backward(True, hook=True)
    assert n_got == 0 and len(seen) == len(seen_ref) == 1 and _same(seen[0], seen_ref[0])
    for a, b in zip(ref, got):
        assert _same(a, b)


def test_a_record_nobody_took_fails_the_step():
    from uaps_amd import lazybn
    with pytest.raises(RuntimeError):
        _block_backward(True, second_consumer=True)      # the fan was not the feature's only consumer: autograd sums, the record is lost
    lazybn.reset()
    lazybn.assert_none_pending()


# ---- whole steps -----------------------------------------------------------------------------------------------------------------

def test_training_steps_eager_replayed_and_with_the_switch_off(monkeypatch):
    """Four steps at 2 + 2 images of 64 x 64 with decoder streams: the eager step, the captured-and-replayed step and the eager step with
    UAPS_FUSED_ENC_GLUE off end with the same parameters, buffers and losses bit for bit; every eager step hands up one record per
    encoder level."""
    import uaps_amd
    from uaps_amd import fused, lazybn, unet
    torch.manual_seed(4)
    m = [uaps_amd.UNet_UAPS(3, 4, feature_chns=[8, 16, 16, 32, 32])]
    m += [copy.deepcopy(m[0]), copy.deepcopy(m[0])]
    monkeypatch.setattr(unet, "_DECODER_STREAMS", True)
    trs = [uaps_amd.UAPSTrainer(m[0].to(DEV), base_lr=1e-3, seed=7, step_state=True),
           uaps_amd.UAPSTrainer(m[1].to(DEV), base_lr=1e-3, seed=7, use_graph=True),
           uaps_amd.UAPSTrainer(m[2].to(DEV), base_lr=1e-3, seed=7, step_state=True)]
    rng = np.random.default_rng(5)
    losses = [[], [], []]
    for i in range(4):
        xl, xu = _t(rng, (2, 3, 64, 64)), _t(rng, (2, 3, 64, 64))
        y = torch.tensor(uaps_amd.data.synthetic_masks(rng, 2, 4, 64, 64)).to(DEV)
        for k, tr in enumerate(trs):
            monkeypatch.setattr(fused, "ENC_GLUE", k != 2)
            uaps_amd.perturb.manual_seed(7, 0)
            np.random.seed(7)
            before = lazybn.sums_total()
            losses[k].append(float(tr.train_step(xl, y, xu)["loss"]))
            if k == 0:
                assert lazybn.sums_total() - before == 5
            if k == 2:
                assert lazybn.sums_total() == before
    assert trs[1].step_graph.graph is not None
    torch.cuda.synchronize()
    assert losses[0] == losses[1] == losses[2] and len(set(losses[0])) == 4
    for k in (1, 2):
        for (n, pa), pb in zip(m[0].named_parameters(), m[k].parameters()):
            assert torch.equal(pa, pb), (k, n)
        for (n, ba), bb in zip(m[0].named_buffers(), m[k].buffers()):
            assert torch.equal(ba, bb), (k, n)
