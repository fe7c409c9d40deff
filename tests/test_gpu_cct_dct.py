"""CCT / DCT on the GPU: the kernels of csrc/loss_cct_dct.hip against float64 restatements of CCT/CCT_train.py and DCT/DCT_train.py,
the grouped forward against separate forwards, the CCT net's p = 0.3 Dropout, whole trainer steps against a float64 oracle built from
oracle.uaps_oracle, checkpoints, the epoch loop and the kernels one step launches."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---- 1. CCT consistency ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [2, 4, 8])
@pytest.mark.parametrize("B,C,H,W", [(2, 4, 64, 64), (3, 7, 33, 45), (16, 4, 256, 256)])
def test_cct_consistency_vs_float64(B, C, H, W, D):
    from oracle import uaps_oracle as O
    from uaps_amd import cct_dct, sibling
    g = torch.Generator().manual_seed(B * 31 + C * 7 + D)
    zs = [torch.randn(B, C, H, W, generator=g) * 2 for _ in range(D)]
    zd = [z.double().requires_grad_(True) for z in zs]
    ref = O.cct_consistency(zd[0], zd[1:])
    (ref * 0.37).backward()
    zg = [z.to(DEV).requires_grad_(True) for z in zs]
    loss, out = cct_dct.cct_consistency_full(zg)
    (loss * 0.37).backward()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5)
    with torch.no_grad():
        sums = [float(((torch.softmax(zd[0], 1) - torch.softmax(z, 1)) ** 2).sum()) for z in zd[1:]]
    np.testing.assert_allclose(out[1:].cpu().double().numpy(), sums, rtol=1e-5)
    for k in range(D):
        scale = float(zd[k].grad.abs().max())
        err = float((zg[k].grad.cpu().double() - zd[k].grad).abs().max())
        assert err <= 1e-5 * scale, (k, err, scale)
    if D == 4 and B <= 3:                      # the composed call form of sibling.py computes the same term
        with torch.no_grad():
            comp = sibling.cct_consistency_loss(zg[0].detach(), [z.detach() for z in zg[1:]])
        np.testing.assert_allclose(float(loss), float(comp), rtol=2e-6)


@pytest.mark.parametrize("H,W", [(64, 64), (33, 45)])
def test_cct_window_inside_a_larger_batch_leaves_other_rows_untouched(H, W):
    from oracle import uaps_oracle as O
    from uaps_amd import _lib, cct_dct
    N, b0, B, Cc, D = 7, 3, 3, 5, 4
    g = torch.Generator().manual_seed(H)
    zs = [torch.randn(N, Cc, H, W, generator=g) * 2 for _ in range(D)]
    zd = [z[b0:b0 + B].double().requires_grad_(True) for z in zs]
    ref = O.cct_consistency(zd[0], zd[1:])
    ref.backward()
    zg = [z.to(DEV) for z in zs]
    loss = cct_dct.cct_consistency_full(zg, b0, B)[0]
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5)
    sentinel = 12345.0
    dz = [torch.full_like(z, sentinel) for z in zg]
    one = torch.ones((), device=DEV)
    L = _lib.lib()
    assert L.uaps_cct_consistency_bwd(_lib.ptr_array(zg), D, b0, B, Cc, H, W, one.data_ptr(), _lib.ptr_array(dz),
                                      _lib.current_stream(torch.device(DEV))) == 0
    for k in range(D):
        d = dz[k].cpu()
        assert bool((d[:b0] == sentinel).all()) and bool((d[b0 + B:] == sentinel).all()), k
        scale = float(zd[k].grad.abs().max())
        assert float((d[b0:b0 + B].double() - zd[k].grad).abs().max()) <= 1e-5 * scale, k
    # the autograd form: zero gradient outside the window
    zr = [z.clone().requires_grad_(True) for z in zg]
    cct_dct.cct_consistency(zr, b0, B).backward()
    assert float(zr[1].grad[:b0].abs().max()) == 0.0 and float(zr[1].grad[b0 + B:].abs().max()) == 0.0


# ---- 2. rot90_batch -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(3, 3, 64, 64), (2, 3, 40, 72), (2, 1, 33, 17)])
def test_rot90_batch_is_bit_identical_to_torch(shape, k):
    from uaps_amd import bounds, cct_dct
    B, Ci, H, W = shape
    g = torch.Generator().manual_seed(k * 10 + H)
    xl, xu = torch.randn(shape, generator=g).to(DEV), (torch.randn(shape, generator=g) * 3).to(DEV)
    batch, rot = cct_dct.rot90_batch(xl, xu, k)
    want_rot = torch.rot90(xu, k, [2, 3])
    if k % 2 and H != W:
        assert rot is not None and batch.shape[0] == 2 * B
        assert torch.equal(batch, torch.cat([xl, xu])) and torch.equal(rot, want_rot)
        every = torch.cat([batch.flatten(), rot.flatten()])
    else:
        assert rot is None and torch.equal(batch, torch.cat([xl, xu, want_rot]))
        every = batch.flatten()
    b = bounds.get(batch)
    if b is not None:                          # the bound is max|.| of everything written
        got = float(b[0].max())
        assert got == float(every.abs().max()), (got, float(every.abs().max()))


def test_rot90_batch_amax_through_the_raw_entry_point():
    from uaps_amd import _lib, bounds
    xl, xu = torch.randn(2, 3, 48, 80, device=DEV), torch.randn(2, 3, 48, 80, device=DEV) * 5
    out = torch.empty(4, 3, 48, 80, device=DEV)
    rot = torch.empty(2, 3, 80, 48, device=DEV)
    am = bounds.new_amax(torch.device(DEV))
    rc = _lib.lib().uaps_rot90_batch_h(_lib.mk_hints((), am), xl.data_ptr(), xu.data_ptr(), 2, 3, 48, 80, 3, out.data_ptr(), rot.data_ptr(),
                                       _lib.current_stream(torch.device(DEV)))
    assert rc == 0
    assert torch.equal(rot, torch.rot90(xu, 3, [2, 3]))
    assert float(am.max()) == float(torch.cat([xl, xu]).abs().max())


# ---- 3. rotation consistency -----------------------------------------------------------------------------------------------------

def _rot_ref(r, u, k):
    rd, ud = r.double().requires_grad_(True), u.double().requires_grad_(True)
    loss = torch.mean((torch.softmax(rd, 1) - torch.rot90(torch.softmax(ud, 1), k, [2, 3])) ** 2)      # DCT_train.py:188
    (loss * 0.61).backward()
    return loss.detach(), rd.grad, ud.grad


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [2, 4, 7])
@pytest.mark.parametrize("HW", [(64, 64), (64, 96), (33, 45)])
def test_rot_consistency_vs_float64(k, C, HW):
    from uaps_amd import cct_dct
    H, W = HW
    B = 3
    g = torch.Generator().manual_seed(k + 10 * C + H)
    u = torch.randn(B, C, H, W, generator=g) * 2
    r = torch.randn((B, C, W, H) if k % 2 else (B, C, H, W), generator=g) * 2
    ref, gr, gu = _rot_ref(r, u, k)
    rg, ug = r.to(DEV).requires_grad_(True), u.to(DEV).requires_grad_(True)
    loss = cct_dct.rot_consistency(rg, ug, k)
    (loss * 0.61).backward()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5)
    for got, want in ((rg.grad, gr), (ug.grad, gu)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_rot_consistency_windows_of_one_batch():
    """r and u as rows of ONE [3B] tensor (the trainer's call form): loss and both gradients land in their rows."""
    from uaps_amd import cct_dct
    B, C, H, W, k = 2, 4, 64, 64, 1
    z = torch.randn(3 * B, C, H, W, device=DEV) * 2
    ref, gr, gu = _rot_ref(z[2 * B:].cpu(), z[B:2 * B].cpu(), k)
    out = cct_dct._rot_fwd(z, 2 * B, z, B, B, k)
    np.testing.assert_allclose(float(out[0]), float(ref), rtol=1e-5)
    dz = torch.full_like(z, 7.0)
    g = torch.full((), 0.61, device=DEV)
    cct_dct._rot_bwd(z, 2 * B, z, B, B, k, g, dz, dz)
    assert bool((dz[:B] == 7.0).all())
    assert float((dz[2 * B:].cpu().double() - gr).abs().max()) <= 1e-5 * float(gr.abs().max())
    assert float((dz[B:2 * B].cpu().double() - gu).abs().max()) <= 1e-5 * float(gu.abs().max())


# ---- 4. grouped forward ---------------------------------------------------------------------------------------------------------

def _unet(C=4, seed=0, dropout=False):
    import uaps_amd
    torch.manual_seed(seed)
    m = uaps_amd.UNet(3, C)
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m


def test_forward_groups_matches_three_separate_forwards():
    """Tolerance as test_gpu_mean_teacher's grouped Monte-Carlo forward: the same kernels, BatchNorm partial sums formed about the
    running mean as it stands when the layer runs."""
    import copy
    net = _unet(seed=12).to(DEV).train()
    sep = copy.deepcopy(net)
    xs = [torch.randn(2, 3, 64, 64, device=DEV) for _ in range(3)]
    with torch.no_grad():
        got = net.forward_groups(xs)
        ref = torch.cat([sep(x) for x in xs])
    assert float((got - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    for (n, a), (_, b) in zip(net.named_buffers(), sep.named_buffers()):
        if a.is_floating_point():
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=n)
        else:
            assert torch.equal(a, b), n
    with pytest.raises(ValueError):
        net.forward_groups(torch.cat(xs), groups=4)


# ---- 5. the CCT net's Dropout ------------------------------------------------------------------------------------------------------

def test_cct_net_aux_dropout_keeps_70_percent_scaled_by_1_over_0_7():
    import uaps_amd
    from uaps_amd import perturb
    torch.manual_seed(3)
    net = uaps_amd.net_factory("unet_cct", 3, 4).to(DEV).train()
    seen = {}
    net.main_decoder.register_forward_pre_hook(lambda m, a: seen.__setitem__("clean", [t.detach().clone() for t in a[0]]))
    net.aux_decoder2.register_forward_pre_hook(lambda m, a: seen.__setitem__("drop", [t.detach().clone() for t in a[0]]))
    with torch.no_grad():
        net(torch.randn(4, 3, 64, 64, device=DEV))
    f, d = seen["clean"][0], seen["drop"][0]
    nz = f != 0
    keep = (d != 0) & nz
    frac = float(keep.double().sum() / nz.double().sum())
    n = float(nz.double().sum())
    assert abs(frac - 0.7) < 5 * (0.21 / n) ** 0.5 + 1e-3, frac                    # 5 sigma of a Bernoulli(0.7) mean
    torch.testing.assert_close(d[keep], f[keep] * np.float32(1 / 0.7), rtol=2e-7, atol=0)
    # the fused fan-out's backward re-applies the forward's mask
    x = torch.randn(2, 16, 64, 64, device=DEV, requires_grad=True)
    outs = perturb.perturbed_fan_out(x, ["noise", "dropout", "feature_dropout"], 1, 0.3, drop_p=0.3)
    keep2 = (outs[2] != 0).to(torch.uint8)
    gy = torch.randn_like(x)
    (outs[2] * gy).sum().backward()
    torch.testing.assert_close(x.grad, perturb.dropout_with(gy, keep2, p=0.3), rtol=1e-6, atol=0)


# ---- 6.-7. trainer steps against a float64 oracle ------------------------------------------------------------------------------------

def _sd64(model):
    sd = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for k in sd:
        if k.endswith(".weight") or k.endswith(".bias"):
            sd[k].requires_grad_(True)
    return sd


def _compare(model, ref, res, captured, init, lr=1e-3, floor=1e-5, rel=5e-3):
    """The tolerances of test_gpu_mean_teacher._run_and_compare.  `floor`: the absolute floor of the gradient check (a LeakyReLU
    derivative that flips at a pre-activation within rounding of 0 moves an element by ~1e-6..1e-5)."""
    assert res["cw"] == ref["cw"]
    for key in ("ce", "dice", "consistency"):
        np.testing.assert_allclose(float(res[key]), float(ref[key]), rtol=2e-5, err_msg=key)
    np.testing.assert_allclose(float(res["loss"]), ref["loss"], rtol=2e-5)
    checked = 0
    for n, p in model.named_parameters():
        g_ref = ref["grads"][n]
        scale = float(g_ref.abs().max())
        err = float((captured[n].cpu().double() - g_ref).abs().max())
        assert err <= max(rel * scale, floor), f"{n}: max err {err:.3e} vs scale {scale:.3e}"
        sure = g_ref.abs() > max(1e-5, 1e-2 * scale)
        delta, delta_ref = p.detach().cpu() - init[n], (ref["new"][n] - init[n].double()).float()
        checked += int(sure.sum())
        if sure.any():
            assert float((delta[sure] - delta_ref[sure]).abs().max()) <= 0.02 * lr, n
    assert checked > 10000


def _adam_ref(sd, loss, out):
    loss.backward()
    pkeys = [k for k in sd if sd[k].requires_grad]
    out["grads"] = {k: sd[k].grad.clone() for k in pkeys}
    torch.optim.Adam([sd[k] for k in pkeys], lr=1e-3).step()
    out["new"] = {k: sd[k].detach() for k in pkeys}
    out["loss"] = float(loss)
    return out


def _hooks(model):
    captured = {}
    hs = [p.register_hook(lambda g, n=n: captured.__setitem__(n, g.detach().clone())) for n, p in model.named_parameters()]
    return captured, hs


def _cct_heads64(x, sd, rnd):
    from oracle import uaps_oracle as O
    f = O.encoder_forward(x, sd, "encoder", True, dropout=[0.0] * 5)
    return [O.decoder_forward(f, sd, "main_decoder", True),
            O.decoder_forward([O.feature_noise(t, n) for t, n in zip(f, rnd["noise"])], sd, "aux_decoder1", True),
            O.decoder_forward([O.feature_bernoulli(t, m, 0.3) for t, m in zip(f, rnd["mask"])], sd, "aux_decoder2", True),
            O.decoder_forward([O.feature_dropout(t, u) for t, u in zip(f, rnd["u"])], sd, "aux_decoder3", True)]


@pytest.mark.parametrize("iter_num", [0, 12000])
def test_cct_step_vs_float64_oracle(iter_num):
    import uaps_amd
    from oracle import uaps_oracle as O
    from uaps_amd import perturb, unet
    from uaps_amd.ramps import get_current_consistency_weight
    rng = np.random.default_rng(21 + iter_num)
    B, C, H, W = 2, 4, 64, 64
    torch.manual_seed(22)
    model = unet.UNet_UAPS(3, C, n_aux=3, dropout=[0.0] * 5, aux_dropout_p=0.3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.7, 1.3); m.bias.uniform_(-0.2, 0.2)
    x_l = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    x_u = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    y_l = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
    fshapes = [(c, H >> i, W >> i) for i, c in enumerate(unet.FEATURE_CHANNELS)]
    rec = {t: {"noise": [torch.tensor(rng.uniform(-0.3, 0.3, s).astype(np.float32)) for s in fshapes],
               "mask": [torch.tensor((rng.random((B,) + s) < 0.7).astype(np.float32)) for s in fshapes],
               "u": [float(rng.uniform(0.7, 0.9)) for _ in fshapes]} for t in ("l", "u")}
    # ---- float64 oracle: CCT_train.py:163-207 ----
    sd = _sd64(model)
    lab, un = _cct_heads64(x_l.double(), sd, rec["l"]), _cct_heads64(x_u.double(), sd, rec["u"])
    ces = [O.cross_entropy(z, y_l) for z in lab]
    dices = [O.dice_loss(y_l.unsqueeze(1), z) for z in lab]
    sup = (sum(ces) + sum(dices)) / 8
    cw = get_current_consistency_weight(0.1, iter_num, 200, 150)
    cons = O.cct_consistency(un[0], un[1:])
    ref = _adam_ref(sd, sup + cw * cons, {"ce": float(sum(ces)), "dice": float(sum(dices)), "consistency": float(cons), "cw": cw})
    # ---- HIP path, the draws injected through forward_pair (as test_gpu_graph.py does) ----
    init = {k: v.detach().clone() for k, v in model.named_parameters()}
    model.to(DEV)

    def dev(t):
        d = rec[t]
        return [n.to(DEV) for n in d["noise"]], [m.to(DEV) for m in d["mask"]], d["u"]

    (nl, ml, ul), (nu, mu, uu) = dev("l"), dev("u")
    drop = functools.partial(perturb.dropout_with, p=0.3)

    def both(fn, fs, a, b):
        return [torch.cat([fn(f[:B].contiguous(), x), fn(f[B:].contiguous(), y)]) for f, x, y in zip(fs, a, b)]
    pert = [lambda fs: both(perturb.feature_noise_with, fs, nl, nu), lambda fs: both(drop, fs, ml, mu),
            lambda fs: [perturb.feature_dropout_with(f, (a, b)) for f, a, b in zip(fs, ul, uu)]]
    orig = model.forward_pair
    model.forward_pair = lambda a, b, perturbations=None: orig(a, b, perturbations=pert)
    tr = uaps_amd.CCTTrainer(model, base_lr=1e-3)
    tr.iter_num = iter_num
    captured, hs = _hooks(model)
    res = tr.train_step(x_l.to(DEV), y_l.to(DEV), x_u.to(DEV))
    for h in hs:
        h.remove()
    # the four heads' supervised terms enter with weight 1/8: the decoders' weight gradients are ~1e-3, where one flip costs 1.3e-5
    _compare(model, ref, res, captured, init, floor=2e-5)
    assert float(res["consistency"]) > 0 and np.isfinite(float(res["unsup"]))


def _dct_oracle(model, x_l, y_l, x_u, k, iter_num):
    from oracle import uaps_oracle as O
    from uaps_amd.ramps import get_current_consistency_weight
    sd = _sd64(model)

    def fwd(x):
        return O.decoder_forward(O.encoder_forward(x.double(), sd, "encoder", True, dropout=[0.0] * 5), sd, "decoder", True)
    lab, un, ro = fwd(x_l), fwd(x_u), fwd(torch.rot90(x_u, k, [2, 3]))               # DCT_train.py:165, 170, 175
    ce, dice = O.cross_entropy(lab, y_l), O.dice_loss(y_l.unsqueeze(1), lab)
    cw = get_current_consistency_weight(0.1, iter_num, 200, 150)
    cons = torch.mean((torch.softmax(ro, 1) - torch.rot90(torch.softmax(un, 1), k, [2, 3])) ** 2)
    return _adam_ref(sd, 0.5 * (ce + dice) + cw * cons, {"ce": float(ce), "dice": float(dice), "consistency": float(cons), "cw": cw}), sd


@pytest.mark.parametrize("k,HW,iter_num", [(0, (64, 64), 0), (1, (64, 64), 12000), (2, (64, 64), 300), (3, (64, 64), 0),
                                           (1, (64, 96), 12000)])
def test_dct_step_vs_float64_oracle(k, HW, iter_num):
    import uaps_amd
    H, W = HW
    rng = np.random.default_rng(40 + k + H + W)
    B, C = 4, 4                                     # the batch and the confident logits of test_gpu_mean_teacher's steps
    model = _unet(C, seed=41)
    with torch.no_grad():
        model.decoder.out_conv.weight.mul_(8.0)
    x_l = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    x_u = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
    y_l = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
    ref, sd = _dct_oracle(model, x_l, y_l, x_u, k, iter_num)
    init = {n: v.detach().clone() for n, v in model.named_parameters()}
    model.to(DEV)
    tr = uaps_amd.DCTTrainer(model, base_lr=1e-3)
    tr.iter_num = iter_num
    captured, hs = _hooks(model)
    res = tr.train_step(x_l.to(DEV), y_l.to(DEV), x_u.to(DEV), rot_times=k)
    for h in hs:
        h.remove()
    assert res["rot_times"] == k
    # the split path (64 x 96 and 96 x 64 maps, other convolution forms): single elements measured at 0.51 % (a conv weight) and 1.1 %
    # (a BatchNorm weight) of their scale, while the loss terms agree to 2e-5
    _compare(model, ref, res, captured, init, rel=2e-2 if H != W else 5e-3)
    # running statistics: three train-mode forwards, labelled -> unlabelled -> rotated
    for n, b in model.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            torch.testing.assert_close(b.cpu().double(), sd[n], rtol=1e-4, atol=1e-5, msg=n)


# ---- 8. checkpoints and the epoch loop ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["cct", "dct"])
def test_checkpoint_round_trip_resumes_bit_identically(tmp_path, which):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=3, device=DEV)

    def trainer():
        torch.manual_seed(5)
        if which == "cct":
            return uaps_amd.CCTTrainer(uaps_amd.net_factory("unet_cct", 3, 4).to(DEV))
        return uaps_amd.DCTTrainer(_unet(seed=5, dropout=True).to(DEV))
    a = trainer()
    a.train_step(*data.items[0])
    path = str(tmp_path / f"{which}.pth")
    a.save_checkpoint(path, 1, 0.5)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("epoch", "best_dice_1", "state_dict", "optimizer", "perturb_rng", "np_global_rng") + (("rot_rng",) if which == "dct" else ()):
        assert key in ck, key
    ra = [a.train_step(*data.items[i]) for i in (1, 2)]
    b = trainer()
    b.load_checkpoint(path)
    rb = [b.train_step(*data.items[i]) for i in (1, 2)]
    for x, y in zip(ra, rb):
        for key in ("loss", "ce", "dice", "consistency"):
            assert torch.equal(x[key], y[key]), key
        if which == "dct":
            assert x["rot_times"] == y["rot_times"]
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


@pytest.mark.parametrize("which", ["cct", "dct"])
def test_fit_two_short_epochs_with_validation(which):
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=2, device=DEV)
    lab = [(xl, yl) for xl, yl, _ in data.items]
    unl = [(xu, yl) for _, yl, xu in data.items]
    torch.manual_seed(6)
    model = uaps_amd.net_factory("unet_cct", 3, 4) if which == "cct" else uaps_amd.net_factory("unet", 3, 4)
    tr = (uaps_amd.CCTTrainer if which == "cct" else uaps_amd.DCTTrainer)(model.to(DEV))
    hist = tr.fit(lab, unl, lab, epochs=3, iter_per_epoch=3)
    assert len(hist) == 2 and tr.iter_num == 4
    for rec in hist:
        assert np.isfinite(rec["loss"]) and np.isfinite(rec["val_mdice"]) and np.isfinite(rec["val_ce"])


# ---- 9. what one step launches --------------------------------------------------------------------------------------------------------

def _kernel_counts(step):
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()}


def _no_aten_softmax_flip_cat(counts):
    bad = {n: c for n, c in counts.items() if "at::" in n and any(s in n.lower() for s in ("softmax", "flip", "catarray"))}
    assert not bad, bad


def test_one_step_launches_each_new_kernel_once_and_no_aten_softmax_flip_or_cat():
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=1, device=DEV)
    xl, yl, xu = data.items[0]
    torch.manual_seed(7)
    cct = uaps_amd.CCTTrainer(uaps_amd.net_factory("unet_cct", 3, 4).to(DEV))
    try:
        counts = _kernel_counts(lambda: cct.train_step(xl, yl, xu))
    except Exception as e:                                   # pragma: no cover
        pytest.skip(f"device profiling not available here: {e}")
    if not any("cct_fwd_kernel" in n for n in counts):
        pytest.skip("the profiler recorded no device kernels of this package")
    assert sum(c for n, c in counts.items() if "cct_fwd_kernel" in n) == 1
    assert sum(c for n, c in counts.items() if "cct_bwd_kernel" in n) == 1
    _no_aten_softmax_flip_cat(counts)
    dct = uaps_amd.DCTTrainer(_unet(seed=8, dropout=True).to(DEV))
    counts = _kernel_counts(lambda: dct.train_step(xl, yl, xu, rot_times=1))
    assert sum(c for n, c in counts.items() if "rot90_batch_kernel" in n) == 1
    assert sum(c for n, c in counts.items() if "rot_cons_kernel" in n and "false" in n) == 1
    assert sum(c for n, c in counts.items() if "rot_cons_kernel" in n and "true" in n) == 1
    _no_aten_softmax_flip_cat(counts)
