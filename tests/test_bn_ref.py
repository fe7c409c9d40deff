"""The BatchNorm reference of tests/bn_ref.py on the CPU: the host Philox against Random123's known answers, the float64 reference
against torch float64 (F.batch_norm + leaky_relu + autograd, nn.BatchNorm2d's running statistics fed group by group), the kink-free
input guarantee, the bars of tests/test_gpu_bn_forms.py rejecting a set of subtle mistakes, and the case table covering every
norm_act kernel of the built code object."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

LLVM = "/opt/rocm/lib/llvm/bin"
_KERNEL = re.compile(r"^(?:void )?\(anonymous namespace\)::(bn_[a-z_]*(?:<[^>]*>)?)\(")


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want


def test_keep_mask_layout():
    """Element e draws word e & 3 of counter offset + (e >> 2), the counter crossing into its high word."""
    n, seed, off = 37, 0x0123456789ABCDEF, 2 ** 32 - 3
    m = R.keep_mask(n, 0.5, seed, off)
    for e in range(n):
        ctr = off + (e >> 2)
        r = int(R.philox4x32_10(ctr & 0xFFFFFFFF, ctr >> 32, R.UAPS_WORD, 0, seed & 0xFFFFFFFF, seed >> 32)[e & 3])
        assert m[e] == ((r >> 8) / 2.0 ** 24 >= 0.5)
    assert 0.2 < m.mean() < 0.8


@pytest.mark.parametrize("B,C,H,W,G,p,res", [(4, 3, 5, 6, 2, 0.0, False), (6, 2, 3, 3, 3, 0.3, False), (2, 3, 4, 4, 1, 0.0, True),
                                             (3, 2, 1, 2, 3, 0.0, False)])
def test_reference_matches_torch_float64(B, C, H, W, G, p, res):
    case = R.Case(f"torch-{B}-{C}-{H}-{W}-{G}-{p}-{res}", R.FWD, B, C, H, W, G, slope=0.1, p=p, residual=res)
    inp = R.inputs(case)
    assert R.min_abs_z(inp["y"], inp["gamma"], inp["beta"], G) >= R.DELTA / 2
    mask = R.keep_mask(B * C * H * W, p, case.seed, case.offset) if p > 0 else None
    ref = R.forward(inp["y"], inp["gamma"], inp["beta"], groups=G, slope=0.1, p=p, mask=mask, conv_bias=inp["conv_bias"], rm=inp["rm"],
                    rv=inp["rv"], nbt=3, momentum=0.1, res=inp.get("res"))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    y = t(inp["y"]).requires_grad_(True)
    gamma, beta = t(inp["gamma"]).requires_grad_(True), t(inp["beta"]).requires_grad_(True)
    bias = t(inp["conv_bias"])
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.running_mean.copy_(t(inp["rm"])); bn.running_var.copy_(t(inp["rv"]))
        bn.momentum = float(np.float32(0.1))
    Bg = B // G
    outs = []
    for g in range(G):                      # the reference's successive forward calls, one per statistics group
        yg = y[g * Bg:(g + 1) * Bg] + bias.view(1, -1, 1, 1)
        z = F.batch_norm(yg, bn.running_mean, bn.running_var, gamma, beta, training=True, momentum=bn.momentum, eps=float(np.float32(R.EPS)))
        outs.append(z)
    z = torch.cat(outs)
    if res:
        out = torch.relu(z + t(inp["res"]))
    else:
        out = F.leaky_relu(z, 0.1)
        if p > 0:
            out = out * t(mask.reshape(B, C, H, W)) / (1.0 - float(np.float32(p)))
    np.testing.assert_allclose(ref["out"], out.detach().numpy(), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(ref["rm"], bn.running_mean.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["rv"], bn.running_var.numpy(), rtol=1e-12, atol=1e-12)
    assert ref["nbt"] == 3 + G
    if res:
        return
    dout = t(inp["dout"])
    out.backward(dout)
    bwd = R.backward(inp["dout"], inp["y"], inp["gamma"], inp["beta"], ref["mean"], ref["invstd"], groups=G, slope=0.1, p=p, mask=mask)
    scale = float(np.abs(bwd["dy"]).max())
    np.testing.assert_allclose(bwd["dy"], y.grad.numpy(), rtol=1e-9, atol=1e-11 * scale)
    np.testing.assert_allclose(bwd["dgamma"], gamma.grad.numpy(), rtol=1e-9, atol=1e-11 * float(bwd["abs_dgamma"].max()))
    np.testing.assert_allclose(bwd["dbeta"], beta.grad.numpy(), rtol=1e-9, atol=1e-11 * float(bwd["abs_dbeta"].max()))


def test_reference_eval_matches_torch_float64():
    case = R.BY_ID["eval"]
    inp = R.inputs(case)
    ref = R.eval_forward(inp["y"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], slope=case.slope, conv_bias=inp["conv_bias"])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    y = t(inp["y"]).requires_grad_(True)
    z = F.batch_norm(y + t(inp["conv_bias"]).view(1, -1, 1, 1), t(inp["rm"]), t(inp["rv"]), t(inp["gamma"]), t(inp["beta"]), training=False,
                     eps=float(np.float32(R.EPS)))
    out = F.leaky_relu(z, case.slope)
    out.backward(t(inp["dout"]))
    np.testing.assert_allclose(ref["out"], out.detach().numpy(), rtol=1e-11, atol=1e-11)
    # (torch's eval-mode input gradient carries the scale through a single-precision step: ~1e-7 relative)
    np.testing.assert_allclose(R.eval_backward(inp["dout"], ref["z"], ref["sc"], case.slope), y.grad.numpy(), rtol=3e-7, atol=0)


@pytest.mark.parametrize("cid", [c.id for c in R.CASES if c.B * c.C * c.HW <= 2 ** 21])
def test_kinkfree_inputs_keep_their_margin(cid):
    case = R.BY_ID[cid]
    inp = R.inputs(case)
    assert R.min_abs_z(inp["y"], inp["gamma"], inp["beta"], case.groups) >= R.DELTA / 2
    assert inp["y"].dtype == np.float32 and np.all(np.isfinite(inp["y"]))


def test_large_mean_channels_are_present():
    inp = R.inputs(R.BY_ID["fwd-large-mean-g4"])
    r = R.forward(inp["y"], inp["gamma"], inp["beta"], groups=4, slope=0.01)
    assert float((np.abs(r["mean"]) * r["invstd"]).max()) > 1e3


def test_case_table_is_consistent():
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        assert c.B % c.groups == 0 and 1 <= c.groups <= R.MAX_GROUPS and c.B * c.C <= 65535, c.id
        assert (c.ppi > 0) == (c.entry in (R.FWD_PARTIALS, R.FINALIZE, R.BWD_FINALIZE)), c.id
        assert not (c.residual and c.p > 0), c.id
    shapes = {(c.B, c.C, c.H, c.W, c.groups) for c in R.CASES}
    for C_, H_ in ((16, 256), (32, 128), (64, 64), (128, 32), (256, 16)):
        assert (32, C_, H_, H_, 2) in shapes
    assert {c.groups for c in R.CASES} >= {1, 2, 3, 4, 5, 8}
    assert {c.HW for c in R.CASES} >= {1, 2, 3, 63, 4097, 65 * 65}
    assert {c.ppi for c in R.CASES} >= {1, 7, 4096} and any(c.ppi % 2048 for c in R.CASES if c.ppi > 2048)
    assert any(c.off % 4 and c.HW % 4 == 0 for c in R.CASES)
    assert any(c.B * c.C == 65535 for c in R.CASES)


# ---- the bars reject subtle mistakes -------------------------------------------------------------------------------------------
def _fwd(case, inp, **kw):
    return R.forward(inp["y"], inp["gamma"], inp["beta"], groups=case.groups, slope=case.slope, p=case.p, mask=kw.pop("mask", inp["mask"]),
                     conv_bias=inp["conv_bias"], rm=inp["rm"], rv=inp["rv"], nbt=inp["nbt"], momentum=0.1, res=inp.get("res"), **kw)


def _bwd(case, inp, **kw):
    return R.backward(inp["dout"], inp["y"], inp["gamma"], inp["beta"], inp["save_mean"], inp["save_invstd"], groups=case.groups,
                      slope=case.slope, p=case.p, mask=kw.pop("mask", inp["mask"]), **kw)


def _f32(d, keys):
    return {k: np.asarray(d[k]).astype(np.float32) for k in keys if k in d}


FWD_KEYS = ("out", "mean", "invstd", "rm", "rv", "xf")


def test_correct_fp32_results_pass_the_bars():
    for cid in ("fwd-hw63", "fwd-hw4097-g5", "fwd-65x65-g8", "fwdp-ppi1-g2", "fwd-residual"):
        case = R.BY_ID[cid]
        inp = R.inputs(case)
        ref = _fwd(case, inp)
        r = R.fwd_ratios(case, inp, ref, _f32(ref, FWD_KEYS))
        assert all(v <= R.TAU[k] for k, v in r.items()), (cid, r)
    for cid in ("bwd-odd-hw3-g3", "bwd-hw4097-g5", "halves-hw63"):
        case = R.BY_ID[cid]
        inp = R.inputs(case)
        ref = _bwd(case, inp)
        got = _f32(ref, ("dy", "dgamma", "dbeta"))
        got["coef"] = R.two_halves_coef(ref, inp["save_mean"], inp["save_invstd"], inp["gamma"], inp["beta"]).astype(np.float32)
        r = R.bwd_ratios(case, ref, got)
        assert all(v <= R.TAU[k] for k, v in r.items()), (cid, r)


@pytest.mark.parametrize("mut,cid,key", [
    ("rv_biased", "fwd-hw2-bg1", "running"),
    ("rm_no_bias", "fwd-hw63", "running"),
    ("eps_outside", "fwd-hw63", "invstd"),
    ("eps_outside", "fwd-hw63", "out"),
    ("group0_stats", "fwd-misaligned", "out"),
    ("drop_chunk", "fwd-hw4097-g5", "mean"),
    ("drop_chunk", "fwd-hw4097-g5", "out"),
    ("mask_ctr", "fwd-hw63", "out"),
    ("mask_word", "fwd-hw63", "out"),
    ("no_drop_scale", "fwd-hw63", "out")])
def test_forward_bars_reject_mutant(mut, cid, key):
    case = R.BY_ID[cid]
    inp = R.inputs(case)
    ref = _fwd(case, inp)
    if mut == "mask_ctr":
        bad = _fwd(case, inp, mask=R.keep_mask(inp["y"].size, case.p, case.seed, case.offset, ctr_shift=1))
    elif mut == "mask_word":
        bad = _fwd(case, inp, mask=R.keep_mask(inp["y"].size, case.p, case.seed, case.offset, word_shift=1))
    else:
        bad = _fwd(case, inp, mut=mut)
    r = R.fwd_ratios(case, inp, ref, _f32(bad, FWD_KEYS))
    assert r[key] > R.TAU[key], (mut, r)


@pytest.mark.parametrize("mut,cid,key", [
    ("no_k2", "bwd-hw4097-g5", "dy"),
    ("no_k3", "bwd-hw4097-g5", "dy"),
    ("no_k2", "bwd-step-256x16", "dy"),
    ("no_k3", "bwd-step-256x16", "dy"),
    ("slope_pos", "bwd-odd-hw3-g3", "dy"),
    ("first_group", "bwd-65x65-g8", "dgamma"),
    ("first_group", "bwd-65x65-g8", "dbeta"),
    ("mask_ctr", "bwd-odd-hw3-g3", "dy"),
    ("mask_word", "bwd-odd-hw3-g3", "dy"),
    ("no_drop_scale", "bwd-odd-hw3-g3", "dy")])
def test_backward_bars_reject_mutant(mut, cid, key):
    case = R.BY_ID[cid]
    inp = R.inputs(case)
    ref = _bwd(case, inp)
    if mut == "mask_ctr":
        bad = _bwd(case, inp, mask=R.keep_mask(inp["y"].size, case.p, case.seed, case.offset, ctr_shift=1))
    elif mut == "mask_word":
        bad = _bwd(case, inp, mask=R.keep_mask(inp["y"].size, case.p, case.seed, case.offset, word_shift=1))
    else:
        bad = _bwd(case, inp, mut=mut)
    r = R.bwd_ratios(case, ref, _f32(bad, ("dy", "dgamma", "dbeta")))
    assert r[key] > R.TAU[key], (mut, r)


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def kernel_pattern(names) -> "re.Pattern":
    """Matches the demangled symbol of a kernel whose base name (template arguments apart) is one of `names`."""
    return re.compile(r"^(?:void )?\(anonymous namespace\)::((?:" + "|".join(map(re.escape, names)) + r")(?:<[^>]*>)?)\(")


def norm_act_kernel_symbols(so_path: str, pattern=_KERNEL) -> set:
    """The kernels whose demangled symbol `pattern` matches (group 1: the name, namespace stripped; by default the norm_act
    kernels) in the gfx950 code objects of so_path (extracted as tests/test_conv_form_table.py does)."""
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
                    m = pattern.match(cols[7].strip())
                    if m:
                        names.add(m.group(1))
        return names
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_cases_cover_every_norm_act_kernel():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    built = norm_act_kernel_symbols(_lib.LIB_PATH)
    assert len(built) == 24, sorted(built)
    named = set().union(*(c.kernels for c in R.CASES))
    assert named == built, (sorted(built - named), sorted(named - built))
