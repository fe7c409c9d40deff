"""Float64 restatements (torch double on the CPU, autograd) of the binary loss family of csrc/loss_binary.hip, written from the
reference's formulas (utilities/losses_2.py: FocalLoss, iou, f_score; utilities/pytorch_losses.py: bce_loss and the num_classes == 1
branches of dice_loss / jaccard_loss / tversky_loss; utilities/losses_1.py: the sigmoid MSE / KL pair), the case table of the GPU sweep
and the entries of the fixture g12_binary.npz through the package.

A label outside {0, 1} enters no term (the defined extension of the kernels).  `planted` switches ONE deliberate mistake on, for the
test that shows the sweep's bars would catch it: "no_pos_weight", "detached_pt", "ineg_without_i", "no_pq"."""
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

TERMS = ("bce", "focal", "jaccard", "fscore", "dice2", "jaccard2", "tversky2")
SUMS = ("n", "P", "G", "I")
PLANTS = ("no_pos_weight", "detached_pt", "ineg_without_i", "no_pq")


def _flat(z, target):
    """(z, g, ok) flat, in z's dtype: the logits, the target in [0, 1] and which elements enter."""
    z = z.reshape(-1)
    t = target.reshape(-1)
    if t.is_floating_point():
        return z, t.to(z.dtype), torch.ones_like(z)
    ok = (t == 0) | (t == 1)
    return z, (t == 1).to(z.dtype), ok.to(z.dtype)


def bin_terms(target, logits, pos_weight=None, focal_alpha=0.8, focal_gamma=2.0, focal_mean=True, beta=1.0, tversky=(0.5, 0.5),
              eps=1e-7, planted: Optional[str] = None):
    """All seven terms by name plus the sums n, P, G, I, in the dtype of `logits`."""
    z, g, ok = _flat(logits, target)
    p = torch.sigmoid(z)
    if planted == "no_pq":                       # a backward without the p (1 - p) factor = a forward whose region sums see z, not p
        p = p.detach() + (z - z.detach())
    n, P, G, I = ok.sum(), (ok * p).sum(), (ok * g).sum(), (ok * g * p).sum()
    pw = None if pos_weight is None or planted == "no_pos_weight" else torch.tensor(float(pos_weight), dtype=z.dtype)
    nd = n.clamp(min=1.0)                        # no label in range: the means are 0 (the kernels' definition)
    out = {"bce": (ok * F.binary_cross_entropy_with_logits(z, g, pos_weight=pw, reduction="none")).sum() / nd}
    l0 = F.binary_cross_entropy_with_logits(z, g, reduction="none")
    pt = torch.exp(-l0)
    if planted == "detached_pt":
        pt = pt.detach()
    f = (ok * focal_alpha * (1 - pt) ** focal_gamma * l0).sum()
    out["focal"] = f / nd if focal_mean else f
    out["jaccard"] = 1 - (I + eps) / (G + P - I + eps)
    b2 = beta ** 2
    out["fscore"] = 1 - ((1 + b2) * I + eps) / ((1 + b2) * I + b2 * (G - I) + (P - I) + eps)
    In = n - P - G + (0 if planted == "ineg_without_i" else I)
    An, Nn = n - P, n - G
    al, be = tversky
    out["dice2"] = 1 - 0.5 * (2 * I / (P + G + eps) + 2 * In / (An + Nn + eps))
    out["jaccard2"] = 1 - 0.5 * (I / (P + G - I + eps) + In / (An + Nn - In + eps))
    out["tversky2"] = 1 - 0.5 * (I / (I + al * (P - I) + be * (G - I) + eps) + In / (In + al * (An - In) + be * (Nn - In) + eps))
    out.update(n=n, P=P, G=G, I=I)
    return out


def sigmoid_mse(a, b):
    return (torch.sigmoid(a) - torch.sigmoid(b)) ** 2


def sigmoid_kl(a, b):
    t = torch.sigmoid(b)
    return (torch.xlogy(t, t) - t * F.logsigmoid(a)).mean()


# ---- the case table of the GPU sweep -------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    shape: tuple                 # (B, H, W)
    target: str                  # "int" | "float" | "zeros" | "ones" | "bad2"
    pos_weight: Optional[float] = None
    gamma: float = 2.0
    scale: float = 2.0           # logits ~ N(0, scale^2), clipped to |z| <= 30
    grad: Optional[float] = None  # None: a NULL gradient pointer (= 1); else the device scalar's value
    offset: int = 0              # floats the logits (and dz) sit behind a 16-byte boundary: 1 = the misaligned scalar form
    seed: int = 0

    @property
    def kernels(self) -> frozenset:
        """The instantiations uaps_binloss_fwd / _bwd launch for the case: SOFT = a float target; the four-element and the scalar
        form are one kernel (`nvec` is an argument), so alignment and size change no name."""
        soft = "true" if self.target == "float" else "false"
        return frozenset({f"bin_fwd_kernel<{soft}>", "bin_finalize", f"bin_bwd_kernel<{soft}>"})


# (1,5,7): 35 elements, the scalar tail alone.  (3,33,19): a count that is no multiple of 4.  (2,96,100): several blocks.
# (3,512,512): 196608 groups of four, more than one pass of 512 blocks x 256 lanes (the kernels' block cap; tests/loss_ref.py has no
# hook to lower a cap, so the smallest shape that takes the second pass stands in).  (1,1,403) at offset 1: one row, misaligned.
SHAPES = ((1, 5, 7), (3, 33, 19), (2, 96, 100))
COEFS = {"bce": 0.6, "focal": 1.3, "jaccard": 0.7, "fscore": 0.4, "dice2": 1.1, "jaccard2": 0.9, "tversky2": 0.5}
TVERSKY, BETA = (0.3, 0.7), 1.5


def cases():
    out = []
    for si, shape in enumerate(SHAPES):
        tag = "x".join(map(str, shape))
        out += [Case(f"{tag}-int", shape, "int", seed=10 * si),
                Case(f"{tag}-float-grad", shape, "float", grad=0.37, seed=10 * si + 1),
                Case(f"{tag}-zeros", shape, "zeros", seed=10 * si + 2),
                Case(f"{tag}-ones", shape, "ones", seed=10 * si + 3),
                Case(f"{tag}-posw", shape, "int", pos_weight=3.0, seed=10 * si + 4),
                Case(f"{tag}-float-posw-g15", shape, "float", pos_weight=0.4, gamma=1.5, seed=10 * si + 5),
                Case(f"{tag}-g15", shape, "int", gamma=1.5, grad=-2.0, seed=10 * si + 6),
                Case(f"{tag}-z30", shape, "int", scale=12.0, seed=10 * si + 7),
                Case(f"{tag}-z30-float-g15", shape, "float", gamma=1.5, scale=12.0, seed=10 * si + 8),
                Case(f"{tag}-bad2", shape, "bad2", pos_weight=2.0, seed=10 * si + 9)]
    out += [Case("1x1x403-off1-int", (1, 1, 403), "int", pos_weight=3.0, offset=1, seed=90),
            Case("1x1x403-off1-float", (1, 1, 403), "float", gamma=1.5, grad=0.5, offset=1, seed=91),
            Case("1x1x403-off1-zeros", (1, 1, 403), "zeros", offset=1, seed=94),
            Case("1x1x403-off1-ones", (1, 1, 403), "ones", grad=0.37, offset=1, seed=95),
            Case("1x1x403-off1-z30", (1, 1, 403), "int", scale=12.0, offset=1, seed=96),
            Case("1x1x403-off1-z30-float-g15", (1, 1, 403), "float", gamma=1.5, scale=12.0, offset=1, seed=97),
            Case("1x1x403-off1-bad2", (1, 1, 403), "bad2", pos_weight=2.0, offset=1, seed=98),
            Case("3x512x512-int", (3, 512, 512), "int", pos_weight=3.0, seed=92),
            Case("3x512x512-float-g15", (3, 512, 512), "float", gamma=1.5, grad=0.25, seed=93)]
    return out


CASES = cases()
# the rest of csrc/loss_binary.hip has no case table: the sigmoid MSE / KL pair (test_sigmoid_mse_and_kl_vs_float64 launches all five)
# and uaps_bin_confusion (test_bin_confusion_is_exact: the zeroing kernel and the counting one), none of them templated
PAIR_KERNELS = frozenset({"sig_mse_fwd_kernel", "sig_mse_bwd_kernel", "sig_kl_fwd_kernel", "sig_kl_finalize", "sig_kl_bwd_kernel"})
CONFUSION_KERNELS = frozenset({"zero4_kernel", "bin_confusion_kernel"})
KERNEL_NAMES = ("bin_fwd_kernel", "bin_finalize", "bin_bwd_kernel", "bin_confusion_kernel", "zero4_kernel") + tuple(sorted(PAIR_KERNELS))


def make_inputs(case: Case):
    """(z float32 [B,1,H,W], target) of a case, host tensors: int64 [B,H,W] labels or a float32 [B,1,H,W] soft target."""
    rng = np.random.default_rng(1000 + case.seed)
    B, H, W = case.shape
    z = np.clip(rng.standard_normal((B, 1, H, W)) * case.scale, -30.0, 30.0).astype(np.float32)
    if case.target == "float":
        t = rng.random((B, 1, H, W)).astype(np.float32)
    elif case.target == "zeros":
        t = np.zeros((B, H, W), dtype=np.int64)
    elif case.target == "ones":
        t = np.ones((B, H, W), dtype=np.int64)
    else:
        t = (rng.random((B, H, W)) < 0.3).astype(np.int64)
        if case.target == "bad2":
            flat = t.reshape(-1)
            flat[3], flat[flat.size - 2] = 7, -1
    return torch.tensor(z), torch.tensor(t)


def reference(case: Case, z, t, dtype=torch.float64, planted=None):
    """{term, sums, loss, dz} of a case in `dtype` (float64: the reference; float32: the floor of the number format)."""
    zz = z.detach().to(dtype, copy=True).requires_grad_(True)          # a copy: at float32 `to` alone would hand back z itself
    tt = t.to(dtype) if t.is_floating_point() else t
    terms = bin_terms(tt, zz, pos_weight=case.pos_weight, focal_gamma=case.gamma, beta=BETA, tversky=TVERSKY, planted=planted)
    loss = sum(COEFS[k] * terms[k] for k in TERMS)
    (loss * (1.0 if case.grad is None else case.grad)).backward()
    out = {k: float(v.detach()) for k, v in terms.items()}
    out["loss"] = float(loss.detach())
    out["dz"] = zz.grad.detach().double().reshape(-1).numpy()
    return out


# Quantities the sweep bars: every term and the loss relative to max(|ref|, 1e-3) -- the terms are O(1) ratios; at an all-zero or
# all-one target some are 0 or 1 to rounding, hence the floor on the denominator --, the sums relative to n (their natural scale:
# each is a sum of n numbers in [0, 1]), dz relative to max|dz_ref|.
QUANTITIES = TERMS + ("loss",) + SUMS + ("dz",)


def errors(got: dict, ref: dict) -> dict:
    out = {}
    for k in TERMS + ("loss",):
        out[k] = abs(got[k] - ref[k]) / max(abs(ref[k]), 1e-3)
    for k in SUMS:
        out[k] = abs(got[k] - ref[k]) / max(ref["n"], 1.0)
    out["dz"] = float(np.abs(np.asarray(got["dz"], dtype=np.float64) - ref["dz"]).max() / max(np.abs(ref["dz"]).max(), 1e-30))
    return out


# The bars: the rule of tests/loss_ref.py -- about 3x the larger of the kernels' measured maximum over the table (MI355X) and the fp32
# floor (this file's reference run in torch.float32 on the CPU), per quantity.  Both columns, the cases that set them and the ratios
# are in profiles/binloss_forms_tau.txt, which tools/binloss_tau.py writes.  The kernels sit at the floor (0.7x to 1.7x of it): block
# sums go through at most 52 fp32 additions and are added in double.  n counts at most 786432 < 2^24 ones per sum: exact.
TAU = {"bce": 4.5e-7, "focal": 6e-7, "jaccard": 3e-7, "fscore": 5e-7, "dice2": 5.5e-7, "jaccard2": 4.5e-7, "tversky2": 6e-7, "loss": 4e-7,
       "n": 0.0, "P": 2.5e-7, "G": 1.5e-7, "I": 7e-8, "dz": 8e-7}
# The sigmoid MSE / KL pair, by the same rule over the shapes of the GPU test (same file, second table): the map absolutely (its values
# lie in [0, 1]), the KL mean relatively, each gradient relative to max|g|.
TAU_PAIR = {"mse_map": 8e-7, "mse_da": 1.5e-6, "kl": 3e-7, "kl_da": 6.5e-7}


# ---- the fixture's entries through the package (shared by the host and the GPU tests) ------------------------------------------------

def fixture_entries(g):
    """(case prefix, entry name) of every recorded loss value of g12_binary.npz."""
    names = ("bce", "bce_pw", "focal", "focal_g15", "jaccard", "dice", "bce_jaccard", "bce_dice", "bce_focal", "dice2", "jaccard2",
             "tversky2", "mse_mean", "kl")
    return [(f"c{i}_", n) for i in range(3) for n in names if f"c{i}_{n}" in g.files]


def fixture_target(g, pre, device="cpu"):
    t = g[pre + "target"]
    return torch.tensor(t.astype(np.int64) if t.dtype == np.uint8 else t, device=device)


def entry_point(name, g, pre, t, z):
    """The fixture entry `name` through the reference-signature entry point of uaps_amd.binary_losses."""
    from uaps_amd import binary_losses as Bn
    if name == "bce":
        return Bn.bce_loss(t, z)
    if name == "bce_pw":
        return Bn.bce_loss(t, z, pos_weight=torch.tensor(3.0))
    if name == "focal":
        return Bn.FocalLoss(logits=True)(z, t)
    if name == "focal_g15":
        return Bn.FocalLoss(alpha=0.6, gamma=1.5, logits=True)(z, t)
    if name == "jaccard":
        return Bn.JaccardLoss()(z, t)
    if name == "dice":
        return Bn.DiceLoss()(z, t)
    if name == "bce_jaccard":
        return Bn.BCEJaccardLoss()(z, t)
    if name == "bce_dice":
        return Bn.BCEDiceLoss()(z, t)
    if name == "bce_focal":
        return Bn.BCEFocalLoss()(z, t)
    if name == "dice2":
        return Bn.dice_loss(t, z)
    if name == "jaccard2":
        return Bn.jaccard_loss(t, z)
    if name == "tversky2":
        return Bn.tversky_loss(t, z, 0.3, 0.7)
    zb = torch.tensor(g[pre + "logits_b"], device=z.device)
    if name == "mse_mean":
        return Bn.sigmoid_mse_loss(z, zb).mean()
    if name == "kl":
        return Bn.sigmoid_kl_loss(z, zb)
    raise KeyError(name)


def check_fixture(g, through_device="cpu", v_rtol=1e-4, g_tol=1e-4):
    """Every recorded quantity of g12 through the package on `through_device` at the project's fixture bar (README "parity"): values
    1e-4 relative, gradients 1e-4 of max|g|.  Returns the number of quantities checked."""
    from uaps_amd import binary_losses as Bn
    checked = 0
    for pre, name in fixture_entries(g):
        z = torch.tensor(g[pre + "logits"], device=through_device).requires_grad_(True)
        t = fixture_target(g, pre, through_device)
        v = entry_point(name, g, pre, t, z)
        assert v.dim() == 0 and v.dtype == torch.float32, (pre, name)
        v.backward()
        print(pre + name, float(v.detach()), float(g[pre + name]))
        np.testing.assert_allclose(float(v.detach()), float(g[pre + name]), rtol=v_rtol, err_msg=pre + name)
        checked += 1
        if pre + "d" + name in g.files:
            ref = g[pre + "d" + name].astype(np.float64)
            err = np.abs(z.grad.detach().cpu().double().numpy() - ref).max()
            print(pre + "d" + name, "max err", err, "max|g|", np.abs(ref).max())
            assert err <= g_tol * np.abs(ref).max(), (pre + name, err, np.abs(ref).max())
            checked += 1
    for i in range(3):
        pre = f"c{i}_"
        z = torch.tensor(g[pre + "logits"], device=through_device)
        t = fixture_target(g, pre, through_device)
        for thr, tag in ((None, "none"), (0.5, "t05")):
            for key, fn in (("iou_", lambda: Bn.iou(z, t, threshold=thr)), ("fscore_", lambda: Bn.f_score(z, t, threshold=thr)),
                            ("fscore_b2_", lambda: Bn.f_score(z, t, beta=2, threshold=thr))):
                np.testing.assert_allclose(float(fn()), float(g[pre + key + tag]), rtol=v_rtol, err_msg=pre + key + tag)
                checked += 1
    z = torch.tensor(g["c0_logits"], device=through_device)
    m = Bn.sigmoid_mse_loss(z, torch.tensor(g["c0_logits_b"], device=through_device))
    ref = g["c0_mse_map"]
    assert float(np.abs(m.cpu().numpy() - ref).max()) <= v_rtol * float(np.abs(ref).max())
    return checked + 1
