"""The C ABI of the supervised loss family on the GPU (include/uaps_hip.h, uaps_segloss_*): every error return comes back with nothing
launched -- `scalars` and `dz`, pre-filled with a sentinel, are untouched on real device buffers -- and a valid call through the raw
entry points gives what the Python surface gives."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SENTINEL = -12345.0
B, CC, H, W = 2, 4, 16, 24


@pytest.fixture(scope="module")
def env():
    from uaps_amd import _lib, seg_losses as S
    L = _lib.lib()
    gen = torch.Generator().manual_seed(17)
    z = (torch.randn(B, CC, H, W, generator=gen) * 2).to(DEV)
    y = torch.randint(0, CC, (B, H, W), generator=gen).to(DEV)
    n = C.c_size_t()
    assert L.uaps_segloss_workspace_bytes(B, CC, H, W, C.byref(n)) == 0 and n.value > 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    crit = S.SegLoss({"ce": 0.5, "jaccard": 0.25, "dice_sq": 1.5}, class_weight=[1.0, 2.0, 0.5, 1.5])
    return dict(L=L, lib=_lib, S=S, z=z, y=y, ws=ws, wsn=n.value, crit=crit, st=_lib.current_stream(z.device))


def _params(env, terms=None, size=None):
    p = env["lib"].SegLossParams.from_buffer_copy(env["crit"].spec.cparams(CC))      # a copy: the criterion keeps its own
    if terms is not None:
        p.terms = terms
    if size is not None:
        p.struct_size = size
    return p


def test_every_error_return_of_the_forward_writes_nothing(env):
    L, lib, z, y, ws = env["L"], env["lib"], env["z"], env["y"], env["ws"]
    scalars = torch.full((lib.seg_nscalars(CC),), SENTINEL, device=DEV)
    wsn = env["wsn"]
    full = C.sizeof(lib.SegLossParams)

    def fwd(z_=z.data_ptr(), y_=y.data_ptr(), prm="ok", B_=B, C_=CC, H_=H, W_=W, s=scalars.data_ptr(), w=ws.data_ptr(), wb=wsn):
        prm = C.byref(_params(env)) if prm == "ok" else prm
        return L.uaps_segloss_fwd(z_, y_, prm, B_, C_, H_, W_, s, w, wb, env["st"])
    cases = [({"z_": None}, EINVAL), ({"y_": None}, EINVAL), ({"prm": None}, EINVAL), ({"s": None}, EINVAL), ({"B_": 0}, EINVAL),
             ({"H_": -1}, EINVAL), ({"W_": 0}, EINVAL), ({"prm": C.byref(_params(env, terms=0))}, EINVAL),
             ({"prm": C.byref(_params(env, terms=1 << 6))}, EINVAL), ({"prm": C.byref(_params(env, size=full - 8))}, EINVAL),
             ({"prm": C.byref(_params(env, size=8))}, EINVAL), ({"C_": 1}, ERANGE), ({"C_": 9}, ERANGE),
             ({"B_": 64, "C_": 8, "H_": 1024, "W_": 1024}, ERANGE), ({"B_": 256, "C_": 2, "H_": 1024, "W_": 1024}, ERANGE),
             ({"w": None}, EWORKSPACE), ({"wb": wsn - 1}, EWORKSPACE), ({"wb": 0}, EWORKSPACE)]
    for kw, want in cases:
        assert fwd(**kw) == want, kw
    torch.cuda.synchronize()
    assert bool((scalars == SENTINEL).all())
    assert L.uaps_segloss_workspace_bytes(B, CC, H, W, None) == EINVAL
    n = C.c_size_t(77)
    assert L.uaps_segloss_workspace_bytes(B, 9, H, W, C.byref(n)) == ERANGE and n.value == 77
    assert L.uaps_segloss_workspace_bytes(B, CC, 0, W, C.byref(n)) == EINVAL and n.value == 77


def test_every_error_return_of_the_backward_writes_nothing(env):
    L, lib, z, y = env["L"], env["lib"], env["z"], env["y"]
    scalars = env["crit"](z, y).scalars
    dz = torch.full_like(z, SENTINEL)
    full = C.sizeof(lib.SegLossParams)

    def bwd(z_=z.data_ptr(), y_=y.data_ptr(), prm="ok", s=scalars.data_ptr(), B_=B, C_=CC, H_=H, W_=W, d=dz.data_ptr()):
        prm = C.byref(_params(env)) if prm == "ok" else prm
        return L.uaps_segloss_bwd(z_, y_, prm, s, None, B_, C_, H_, W_, d, env["st"])
    cases = [({"z_": None}, EINVAL), ({"y_": None}, EINVAL), ({"prm": None}, EINVAL), ({"s": None}, EINVAL), ({"d": None}, EINVAL),
             ({"B_": -3}, EINVAL), ({"H_": 0}, EINVAL), ({"W_": 0}, EINVAL), ({"prm": C.byref(_params(env, terms=0))}, EINVAL),
             ({"prm": C.byref(_params(env, terms=128))}, EINVAL), ({"prm": C.byref(_params(env, size=full - 1))}, EINVAL),
             ({"C_": 1}, ERANGE), ({"C_": 9}, ERANGE), ({"B_": 64, "C_": 8, "H_": 1024, "W_": 1024}, ERANGE)]
    for kw, want in cases:
        assert bwd(**kw) == want, kw
    torch.cuda.synchronize()
    assert bool((dz == SENTINEL).all())


def test_raw_entry_points_give_what_the_python_surface_gives(env):
    """A larger struct_size (a later header's) is accepted: the fields of this version are read, the rest is not."""
    L, lib, S, z, y, ws = env["L"], env["lib"], env["S"], env["z"], env["y"], env["ws"]
    zg = z.clone().requires_grad_(True)
    out = env["crit"](zg, y)
    out.loss.backward()

    class Later(C.Structure):
        _fields_ = [("base", lib.SegLossParams), ("appended", C.c_double * 4)]
    later = Later()
    later.base = _params(env)
    later.base.struct_size = C.sizeof(Later)
    scalars = torch.full((lib.seg_nscalars(CC),), SENTINEL, device=DEV)
    dz = torch.full_like(z, SENTINEL)
    assert L.uaps_segloss_fwd(z.data_ptr(), y.data_ptr(), C.byref(later), B, CC, H, W, scalars.data_ptr(), ws.data_ptr(), env["wsn"],
                              env["st"]) == 0
    assert L.uaps_segloss_bwd(z.data_ptr(), y.data_ptr(), C.byref(later), scalars.data_ptr(), None, B, CC, H, W, dz.data_ptr(),
                              env["st"]) == 0
    assert torch.equal(scalars, out.scalars) and torch.equal(dz, zg.grad)
    sc = S.seg_scalars(scalars, CC)
    assert float(sc["focal"]) == 0.0 and float(sc["dice"]) == 0.0 and float(sc["tversky"]) == 0.0      # not selected: stored as 0
    assert float(sc["ce"]) > 0 and float(sc["jaccard"]) > 0 and float(sc["dice_sq"]) > 0
