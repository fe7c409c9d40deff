"""The supervised loss family on the GPU: the kernels of csrc/loss_seg.hip against the reference-generated fixture g11_seglosses.npz
and against the float64 restatements of tests/segloss_ref.py, their ignore / bad-label / scaling semantics, the {CE, Dice} selection
against uaps_sup_loss, BaselineTrainer steps with a SegLoss against float64 steps, and what a forward + backward launches."""
import os

import numpy as np
import pytest
import torch

import segloss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_seglosses.npz")


# ---- 1. the fixture of the reference -----------------------------------------------------------------------------------------------

def _fixture_check(g, pre, name, value, grad):
    """The bars of test_cps_loss_matches_the_reference_fixture: terms rtol 2e-5, gradients rtol 1e-3 / atol 2e-5 max|g|."""
    print(pre + name, float(value), float(g[pre + name]))
    np.testing.assert_allclose(float(value), float(g[pre + name]), rtol=2e-5, err_msg=pre + name)
    if pre + "d" + name in g.files:
        ref = g[pre + "d" + name]
        np.testing.assert_allclose(grad.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * np.abs(ref).max(), err_msg=pre + "d" + name)


@pytest.mark.parametrize("through", ["entry_points", "segloss"])
def test_seg_losses_match_the_reference_fixture(through):
    from uaps_amd import seg_losses as S
    g = np.load(GOLD)
    for pre, name, lab, _ in R.fixture_cases(g):
        z = torch.tensor(g[pre + "logits"], device=DEV, requires_grad=True)
        y = torch.tensor(g[pre + lab].astype(np.int64), device=DEV)
        if through == "entry_points":
            v = R.entry_point(name, g, pre, y, z)
        else:
            out = R.seg_loss_for(name, g, pre)(z, y)
            v = out.loss
            sc = S.seg_scalars(out.scalars, z.shape[1])
            assert float(sc["bad"]) == 0.0 and float(sc[R.term_of(name)]) == float(v.detach())
        assert v.is_cuda and v.dim() == 0
        v.backward()
        _fixture_check(g, pre, name, v.detach(), z.grad)


# ---- 2. float64 sweep --------------------------------------------------------------------------------------------------------------
# (B, H, W): one pixel a lane with 23 blocks; a single row; four pixels a lane with 5 blocks; four pixels a lane inside one block.
_SHAPES = [(3, 37, 53), (2, 1, 40), (4, 32, 40), (2, 16, 24)]
_SWEEP = [(B, C, H, W, ign, False) for C in (2, 3, 4, 7, 8) for B, H, W in _SHAPES for ign in (False, True)]
_SWEEP += [(2, 4, 16, 24, True, True), (2, 7, 16, 24, False, True)]      # logits one float off 16-byte alignment: one pixel a lane
# more items than the 1024 x 256 lanes of the largest grid, so lanes take a second trip through the grid-stride loop: 262 205
# one-pixel items (229 x 229 is odd) and 278 528 four-pixel items.  These two run the all-six-terms spec only.
_MULTI_TRIP = [(5, 2, 229, 229, True, False), (17, 2, 256, 256, True, False)]
_SWEEP += _MULTI_TRIP
# Bars: 1e-5 on the terms, the gradient and the class sum of a pixel's gradient (of max|g|).  A case that does not hold them gets
# 4 x the error of the same restatement evaluated in fp32 by torch on the CPU against the float64 one, measured on that case
# (profiles/segloss_forms_tau.txt): (B, C, H, W) -> {quantity: bar}.
_TAU = {}


def _specs(C, gen):
    """All six terms at once with unequal coefficients, then each term alone (focal at gamma 2 and at a non-integer gamma)."""
    cw = (0.5 + 1.5 * torch.rand(C, generator=gen)).tolist()
    alpha = (0.25 + 0.75 * torch.rand(C, generator=gen)).tolist()
    dsq = (0.5 + torch.rand(C, generator=gen)).tolist()
    kw = dict(class_weight=cw, focal_gamma=1.5, focal_alpha=alpha, tversky=(0.3, 0.7), dice_sq_weight=dsq)
    coefs = {"ce": 0.83, "focal": 0.31, "dice": 0.57, "jaccard": 1.3, "tversky": 0.44, "dice_sq": 0.71}
    out = [(coefs, kw)] + [({k: 1.0}, kw) for k in R.TERMS]
    out.append(({"focal": 1.0}, dict(kw, focal_gamma=2.0)))
    return out


def _ref_loss(coefs, kw, y, zd, ignore):
    terms = R.seg_terms(y, zd, class_weight=kw["class_weight"], ignore=ignore, focal_gamma=kw["focal_gamma"],
                        focal_alpha=kw["focal_alpha"], tversky=kw["tversky"], dice_sq_weight=kw["dice_sq_weight"])
    return sum(c * terms[k] for k, c in coefs.items()), terms


def _device_logits(z, misaligned):
    """z on the GPU as a leaf; `misaligned`: a contiguous view that starts one float into its buffer."""
    if not misaligned:
        return z.to(DEV).requires_grad_(True)
    buf = torch.empty(z.numel() + 1, device=DEV)
    buf[1:] = z.reshape(-1).to(DEV)
    v = buf[1:].view(z.shape).detach().requires_grad_(True)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("B,C,H,W,ign,misaligned", _SWEEP)
def test_seg_kernels_vs_float64(B, C, H, W, ign, misaligned):
    """The bars of test_cps_kernels_vs_float64 (the same arithmetic: fp32 exp / log / division a few ulp per pixel, fp32 sums over at
    most a lane's pixels, then a block's lanes, and double across blocks): terms rtol 1e-5, gradient error <= 1e-5 max|g|, class sum
    of each pixel's gradient <= 1e-5 max|g| (see _TAU); two runs give the same bits."""
    from uaps_amd import seg_losses as S
    gen = torch.Generator().manual_seed(B * 131 + C * 17 + H * 3 + W + 7 * ign)
    z = torch.randn(B, C, H, W, generator=gen) * 2
    y = torch.randint(0, C, (B, H, W), generator=gen)
    ignore = None
    if ign:
        ignore = 255
        y[:, :, 3:9] = 255                                   # a planted strip
        y[0, 0, 0] = 255
    tau = {"terms": 1e-5, "grad": 1e-5, "sum": 1e-5, **_TAU.get((B, C, H, W), {})}
    specs = _specs(C, gen)
    for coefs, kw in specs[:1] if (B, C, H, W, ign, misaligned) in _MULTI_TRIP else specs:
        zd = z.double().requires_grad_(True)
        ref, terms = _ref_loss(coefs, kw, y, zd, ignore)
        ref.backward()
        crit = S.SegLoss(coefs, ignore_index=ignore, **kw)
        zg = _device_logits(z, misaligned)
        out = crit(zg, y.to(DEV))
        out.loss.backward()
        sc = S.seg_scalars(out.scalars, C)
        tag = (tuple(coefs), kw["focal_gamma"])
        for k in coefs:
            print(tag, k, float(sc[k]), float(terms[k]))
            np.testing.assert_allclose(float(sc[k]), float(terms[k]), rtol=tau["terms"], err_msg=str((tag, k)))
        np.testing.assert_allclose(float(out.loss.detach()), float(ref.detach()), rtol=tau["terms"], err_msg=str(tag))
        assert float(sc["bad"]) == 0.0 and float(sc["n_valid"]) == float((y != 255).sum())
        scale = float(zd.grad.abs().max())
        err = float((zg.grad.cpu().double() - zd.grad).abs().max())
        csum = float(zg.grad.sum(dim=1).abs().max())
        print(tag, "grad err", err, "class sum", csum, "scale", scale)
        assert err <= tau["grad"] * scale, (tag, err, scale)
        assert csum <= tau["sum"] * scale, (tag, csum, scale)
        if ign:
            assert float(zg.grad[:, :, :, 3:9].abs().max()) == 0.0           # ignored pixels: exactly zero
        # two runs give the same bits
        zh = _device_logits(z, misaligned)
        again = crit(zh, y.to(DEV))
        again.loss.backward()
        assert torch.equal(again.scalars, out.scalars) and torch.equal(zh.grad, zg.grad), tag


# ---- 3. semantics ------------------------------------------------------------------------------------------------------------------

def _small(C=4, B=2, H=16, W=24, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=gen) * 2, torch.randint(0, C, (B, H, W), generator=gen)


def test_all_ignored_gives_nan_ce_as_torch_and_zero_gradient():
    from uaps_amd import seg_losses as S
    z, _ = _small()
    y = torch.full((2, 16, 24), 255)
    ref = torch.nn.functional.cross_entropy(z, y, ignore_index=255)
    assert bool(torch.isnan(ref))
    zg = z.to(DEV).requires_grad_(True)
    loss = S.ce_loss(y.to(DEV), zg, [1.0, 2.0, 3.0, 4.0], ignore=255)
    assert bool(torch.isnan(loss))
    loss.backward()
    assert float(zg.grad.abs().max()) == 0.0                                  # every pixel is ignored: dz = 0, not NaN


def test_out_of_range_label_is_counted_and_gets_zero_gradient():
    from uaps_amd import seg_losses as S
    z, y = _small()
    y[1, 7, 5], y[0, 0, 1], y[0, 3, 3] = 9, -1, 255
    crit = S.SegLoss({k: 1.0 for k in S.TERMS}, ignore_index=255)
    zg = z.to(DEV).requires_grad_(True)
    out = crit(zg, y.to(DEV))
    out.loss.backward()
    sc = S.seg_scalars(out.scalars, 4)
    assert float(sc["bad"]) == 2.0 and float(sc["n_valid"]) == 2 * 16 * 24 - 3
    for b, h, w in ((1, 7, 5), (0, 0, 1), (0, 3, 3)):
        assert float(zg.grad[b, :, h, w].abs().max()) == 0.0
    zd = z.double().requires_grad_(True)
    ref = sum(R.seg_terms(y, zd, ignore=255).values())
    np.testing.assert_allclose(float(out.loss.detach()), float(ref.detach()), rtol=1e-5)
    assert int((zg.grad.abs().sum(dim=1) > 0).sum()) == 2 * 16 * 24 - 3


def test_bwd_overwrites_nan_and_null_grad_means_one():
    import ctypes as C
    from uaps_amd import _lib, seg_losses as S
    z, y = _small()
    z, y = z.to(DEV), y.to(DEV)
    spec = S.SegLoss({k: 0.5 for k in S.TERMS}, class_weight=[1.0, 2.0, 0.5, 1.5]).spec
    prm = spec.cparams(4)
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_segloss_workspace_bytes(2, 4, 16, 24, C.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    scalars = torch.full((_lib.seg_nscalars(4),), float("nan"), device=DEV)
    st = _lib.current_stream(z.device)
    assert L.uaps_segloss_fwd(z.data_ptr(), y.data_ptr(), C.byref(prm), 2, 4, 16, 24, scalars.data_ptr(), ws.data_ptr(), n.value, st) == 0
    assert bool(torch.isfinite(scalars).all())
    one = torch.ones((), device=DEV)
    a, b = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    assert L.uaps_segloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(prm), scalars.data_ptr(), one.data_ptr(), 2, 4, 16, 24, a.data_ptr(), st) == 0
    assert L.uaps_segloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(prm), scalars.data_ptr(), None, 2, 4, 16, 24, b.data_ptr(), st) == 0
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and float(a.abs().max()) > 0
    half = torch.full((), 0.5, device=DEV)
    c = torch.full_like(z, float("nan"))
    assert L.uaps_segloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(prm), scalars.data_ptr(), half.data_ptr(), 2, 4, 16, 24, c.data_ptr(), st) == 0
    assert float((c - 0.5 * a).abs().max()) <= 1e-6 * float(a.abs().max())


@pytest.mark.parametrize("B,C,H,W", [(3, 4, 37, 53), (2, 2, 16, 24), (4, 8, 32, 40)])
def test_ce_dice_selection_agrees_with_uaps_sup_loss(B, C, H, W):
    """{dice 0.5, ce 0.5} without weights is uaps_sup_loss((z,), y): both against the float64 restatement at the sweep's bars, so
    they agree with each other to twice those."""
    import uaps_amd
    from uaps_amd import seg_losses as S
    z, y = _small(C, B, H, W, seed=11)
    zd = z.double().requires_grad_(True)
    ref = 0.5 * R.ce_loss(y, zd) + 0.5 * R.dice_loss(y, zd)
    ref.backward()
    scale = float(zd.grad.abs().max())
    za, zb = z.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    a = S.SegLoss({"dice": 0.5, "ce": 0.5})(za, y.to(DEV))
    b = uaps_amd.uaps_sup_loss((zb,), y.to(DEV))
    a.loss.backward()
    b.loss.backward()
    for got, grad in ((a.loss, za.grad), (b.loss, zb.grad)):
        np.testing.assert_allclose(float(got.detach()), float(ref.detach()), rtol=1e-5)
        assert float((grad.cpu().double() - zd.grad).abs().max()) <= 1e-5 * scale
    sa, sb = S.seg_scalars(a.scalars, C), uaps_amd.sup_scalars(b.scalars, 1, C)
    np.testing.assert_allclose(float(sa["ce"]), float(sb["ce"][0]), rtol=2e-5)
    np.testing.assert_allclose(float(sa["dice"]), float(sb["dice"][0]), rtol=2e-5)
    assert float((za.grad - zb.grad).abs().max()) <= 2e-5 * scale


def test_focal_gradient_is_the_detached_form():
    """The reference detaches p_t inside (1 - p_t)^gamma (losses_1.py:85).  The kernel's gradient matches that form at the sweep's bar;
    the full derivative differs from it by far more than the bar on this input, so a wrong derivation cannot pass."""
    from uaps_amd import seg_losses as S
    z, y = _small(C=3, seed=23)
    alpha = [0.4, 0.9, 0.7]
    grads = {}
    for detach in (True, False):
        zd = z.double().requires_grad_(True)
        R.focal_loss(y, zd, 1.5, alpha, True, None, detach_pt=detach).backward()
        grads[detach] = zd.grad
    scale = float(grads[True].abs().max())
    apart = float((grads[True] - grads[False]).abs().max())
    print("detached vs full derivative: max difference", apart, "of max|g|", scale)
    assert apart > 1e-2 * scale
    zg = z.to(DEV).requires_grad_(True)
    S.FocalLoss(gamma=1.5, alpha=alpha)(zg, y.to(DEV)).backward()
    got = zg.grad.cpu().double()
    assert float((got - grads[True]).abs().max()) <= 1e-5 * scale
    assert float((got - grads[False]).abs().max()) > 1e-2 * scale


def test_device_weight_tensor_and_label_layouts():
    from uaps_amd import seg_losses as S
    z, y = _small()
    w = torch.tensor([1.0, 2.0, 0.5, 1.5], device=DEV)
    zg = z.to(DEV)
    a = S.ce_loss(y.to(DEV), zg, w, ignore=255)
    b = S.ce_loss(y.to(DEV).unsqueeze(1), zg, [1.0, 2.0, 0.5, 1.5], ignore=255)
    c = S.ce_loss(y.to(DEV).to(torch.uint8), zg, w.cpu(), ignore=255)
    assert torch.equal(a, b) and torch.equal(a, c)
    ref = torch.nn.functional.cross_entropy(z.double(), y, weight=w.cpu().double())
    np.testing.assert_allclose(float(a), float(ref), rtol=1e-5)


# ---- 4. the trainer ----------------------------------------------------------------------------------------------------------------

def _sd64(model):
    sd = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    for k in sd:
        if k.endswith(".weight") or k.endswith(".bias"):
            sd[k].requires_grad_(True)
    return sd


def test_baseline_trainer_steps_with_a_segloss_vs_float64_steps():
    """Two steps of BaselineTrainer(loss=SegLoss({ce 0.5, tversky 0.5}, class_weight)) at B = 2, 64 x 64; each against a float64 step
    from the same parameters (oracle.uaps_oracle's network, tests/segloss_ref.py's loss).  The bars of
    test_baseline_supervised_step_vs_cpu_oracle: loss and terms rtol 2e-5, every gradient max(5e-3 of its scale, 1e-5), the first
    Adam update of the surely non-zero elements to 0.02 lr."""
    import uaps_amd
    from oracle import uaps_oracle as O
    from uaps_amd import seg_losses as S
    torch.manual_seed(31)
    rng = np.random.default_rng(31)
    B, H, W, C = 2, 64, 64, 4
    cw = [0.5, 2.0, 1.5, 3.0]
    model = uaps_amd.UNet(3, C)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.to(DEV)
    tr = uaps_amd.BaselineTrainer(model, base_lr=1e-3, loss=S.SegLoss({"ce": 0.5, "tversky": 0.5}, class_weight=cw, tversky=(0.3, 0.7)))
    assert tr.log_keys == ("loss", "ce", "tversky")
    checked = 0
    for step in range(2):
        x = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32))
        y = torch.tensor(uaps_amd.data.synthetic_masks(rng, B, C, H, W))
        sd = _sd64(model)
        init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        logits = O.decoder_forward(O.encoder_forward(x.double(), sd, "encoder", True, dropout=[0.0] * 5), sd, "decoder", True)
        ce, tv = R.ce_loss(y, logits, cw), R.tversky_loss(y, logits, 0.3, 0.7)
        loss = 0.5 * ce + 0.5 * tv
        loss.backward()
        captured = {}
        hooks = [p.register_hook(lambda g, n=n: captured.__setitem__(n, g.detach().clone())) for n, p in model.named_parameters()]
        res = tr.train_step(x.to(DEV), y.to(DEV))
        for h in hooks:
            h.remove()
        assert set(res) == {"loss", "ce", "tversky", "bad_labels"} and float(res["bad_labels"]) == 0.0
        for key, ref in (("loss", loss), ("ce", ce), ("tversky", tv)):
            np.testing.assert_allclose(float(res[key]), float(ref.detach()), rtol=2e-5, err_msg=f"step {step} {key}")
        pkeys = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
        grads = {k: sd[k].grad.clone() for k in pkeys}
        if step == 0:
            torch.optim.Adam([sd[k] for k in pkeys], lr=1e-3).step()
        for n, p in model.named_parameters():
            g_ref = grads[n]
            scale = float(g_ref.abs().max())
            err = float((captured[n].cpu().double() - g_ref).abs().max())
            assert err <= max(5e-3 * scale, 1e-5), f"step {step} {n}: max err {err:.3e} vs scale {scale:.3e}"
            if step == 0:
                sure = g_ref.abs() > max(1e-5, 1e-2 * scale)
                delta, delta_ref = p.detach().cpu() - init[n], (sd[n].detach() - init[n].double()).float()
                checked += int(sure.sum())
                if sure.any():
                    assert float((delta[sure] - delta_ref[sure]).abs().max()) <= 0.02 * 1e-3, n
    assert checked > 10000 and tr.iter_num == 2


def test_loss_none_steps_are_bit_identical_to_a_trainer_built_without_the_argument():
    import uaps_amd
    data = uaps_amd.data.SyntheticBatches(2, H=64, W=64, n_batches=2, device=DEV)
    results, weights = [], []
    for kw in ({}, {"loss": None}):
        torch.manual_seed(9)
        tr = uaps_amd.BaselineTrainer(uaps_amd.net_factory("unet", 3, 4).to(DEV), **kw)
        res = [tr.train_step(xl, yl) for xl, yl, _ in data.items]
        assert all(set(r) == {"loss", "ce", "dice"} for r in res)
        results.append([{k: v.clone() for k, v in r.items()} for r in res])
        weights.append([p.detach().clone() for p in tr.model.parameters()])
    for ra, rb in zip(*results):
        for k in ("loss", "ce", "dice"):
            assert torch.equal(ra[k], rb[k]), k
    assert all(torch.equal(p, q) for p, q in zip(*weights))


def test_forward_and_backward_launch_three_kernels_and_no_aten_pass_over_the_logits():
    """In the manner of test_gpu_strided.py's profiler assertion: a SegLoss forward + backward is seg_fwd_kernel, seg_finalize and
    seg_bwd_kernel; the only ATen kernels beside them fill or copy single scalars (the loss scalar's clone, autograd's initial
    gradient) -- no elementwise, softmax, gather or reduce kernel, which is what a pass over [B,C,H,W] would be."""
    from torch.profiler import ProfilerActivity, profile
    from uaps_amd import seg_losses as S
    z, y = _small(C=4, B=2, H=64, W=64)
    y = y.to(DEV)
    crit = S.SegLoss({k: 1.0 for k in S.TERMS}, class_weight=[1.0, 2.0, 0.5, 1.5], focal_gamma=1.5)

    def run():
        zg = z.to(DEV).requires_grad_(True)
        torch.cuda.synchronize()
        return zg

    def step(zg):
        crit(zg, y).loss.backward()
        torch.cuda.synchronize()
    step(run())
    zg = run()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(zg)
    counts = {e.key: e.count for e in prof.key_averages() if "memcpy" not in e.key.lower() and "memset" not in e.key.lower()}
    print(counts)
    assert any("seg_fwd_kernel" in n for n in counts), "the profiler recorded no device kernels of this package"
    for name in ("seg_fwd_kernel", "seg_finalize", "seg_bwd_kernel"):
        assert sum(c for n, c in counts.items() if name in n) == 1, name
    other = {n: c for n, c in counts.items() if "at::" in n}                   # (the rest of the trace: runtime calls)
    assert all(("fill" in n.lower() or "copy" in n.lower()) for n in other), other
    assert sum(other.values()) <= 4, other
