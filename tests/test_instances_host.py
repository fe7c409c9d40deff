"""Defect instances and run-length masks without a GPU: the package's CPU restatement (uaps_amd/instances.py, a two-pass union-find)
against scipy (tests/instances_ref.py), the C ABI's argument checks (they return before any launch), and the run-length format against
the strings the reference's mask2rle produced (tests/golden/g13_rle.npz, written by tools/make_golden_rle.py).  Every comparison is
exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as R
from conftest import GOLDEN, ROOT

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
SHAPES = ((1, 1), (1, 17), (23, 1), (37, 53))


@pytest.mark.parametrize("density", (0.3, 0.6))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("min_area", (1, 5))
@pytest.mark.parametrize("background", (0, None))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_cpu_path_equals_scipy(connectivity, background, min_area, shape, density):
    from uaps_amd import label_instances
    H, W = shape
    m = R.noise(2, H, W, density, seed=H * 7 + W)
    maps = R.random_maps(2, H, W)
    res = label_instances(torch.from_numpy(m), [torch.from_numpy(v) for v in maps], connectivity=connectivity, background=background,
                          min_area=min_area, max_instances=2048)
    R.assert_equal(res, R.label_batch(m, maps, connectivity, background, min_area, 2048))
    assert not bool(res.overflow.any())
    n0 = int(res.count[0])
    mean = res.means()
    assert mean.dtype == torch.float64 and mean.shape == (2, 2048, 2)
    if n0:
        t = res.table[0, 0]
        assert float(mean[0, 0, 0]) == int(t[7]) / 16777216.0 / int(t[1])
    recs = res.records()
    assert [len(r) for r in recs] == res.count.tolist()
    if n0:
        r0 = recs[0][0]
        assert r0["label"] == 1 and r0["cls"] == int(res.table[0, 0, 0]) and r0["bbox"] == tuple(res.table[0, 0, 2:6].tolist())
        assert r0["mean0"] == float(mean[0, 0, 0]) and r0["mean1"] == float(mean[0, 0, 1])


def test_checkerboard_overflow():
    from uaps_amd import label_instances
    m = R.checkerboard(37, 53)
    one = label_instances(torch.from_numpy(m), connectivity=8)
    assert one.count.tolist() == [1] and one.table[0, 0, :7].tolist() == [1, 981, 0, 0, 37, 53, 0]
    many = label_instances(torch.from_numpy(m), connectivity=4, max_instances=256)
    assert many.count.tolist() == [981] and many.overflow.tolist() == [True] and many.table.shape == (1, 256, 9)
    R.assert_equal(many, R.label_batch(m, (), 4, 0, 1, 256))
    assert int(many.labels.max()) == 981 and int((many.labels > 0).sum()) == 981          # complete labels
    assert bool((many.table[0, :, 1] == 1).all())                                          # 256 rows, all filled
    assert len(many.records()[0]) == 256
    one_map = label_instances(torch.from_numpy(m), [torch.ones(1, 37, 53)], connectivity=8)
    assert one_map.records()[0][0]["mean0"] == 1.0 and one_map.records()[0][0]["mean1"] is None


def test_clamp_rule_and_argument_checks():
    from uaps_amd import label_instances
    m = torch.ones(1, 2, 3, dtype=torch.int64)
    v = torch.tensor([[[float("nan"), 1e9, -1e9], [0.5, 2.0 ** -25, 3.0 * 2.0 ** -25]]])
    res = label_instances(m, [v])
    # NaN -> 0, +-1e9 -> +-65536 (cancel), 0.5 -> 2^23, 2^-25 -> rint(0.5) = 0, 3 * 2^-25 -> rint(1.5) = 2
    assert int(res.table[0, 0, 7]) == 2 ** 23 + 2 and int(res.table[0, 0, 8]) == 0
    with pytest.raises(TypeError):
        label_instances(m.int())
    with pytest.raises(ValueError):
        label_instances(m, connectivity=6)
    with pytest.raises(ValueError):
        label_instances(m, max_instances=0)
    with pytest.raises(ValueError):
        label_instances(m, [v, v, v])
    with pytest.raises(TypeError):
        label_instances(m, [v.double()])


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_instances_workspace_bytes", "uaps_label_instances", "uaps_rle_count", "uaps_rle_encode", "uaps_rle_decode"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uaps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    # the ctypes mirrors have the header's layout: the fields named in the header, in its order
    for struct, cname in ((_lib.InstancesCall, "uaps_instances_call"), (_lib.RleCall, "uaps_rle_call")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
        assert names == [f[0] for f in struct._fields_], (cname, names)


def _inst_call(B=1, H=8, W=8, **kw):
    from uaps_amd import _lib
    c = _lib.InstancesCall()
    c.struct_size = C.sizeof(_lib.InstancesCall)
    c.B, c.H, c.W, c.connectivity, c.has_background, c.background, c.min_area, c.max_instances = B, H, W, 8, 1, 0, 1, 16
    c.mask = c.labels = c.count = c.table = c.workspace = 4096           # never dereferenced: every call below returns before a launch
    c.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    assert L.uaps_instances_workspace_bytes(16, 256, 256, C.byref(n)) == 0 and n.value >= 2 * 4 * 16 * 256 * 256
    assert L.uaps_instances_workspace_bytes(1, 1, 1, C.byref(n)) == 0 and n.value > 0
    assert L.uaps_instances_workspace_bytes(0, 8, 8, C.byref(n)) == EINVAL
    assert L.uaps_instances_workspace_bytes(1, 8, 8, None) == EINVAL
    assert L.uaps_instances_workspace_bytes(1, 65536, 32768, C.byref(n)) == ERANGE          # H * W = 2^31
    assert L.uaps_instances_workspace_bytes(64, 2048, 2048, C.byref(n)) == ERANGE           # B * H * W * 8 = 2 GiB
    run = lambda c: L.uaps_label_instances(C.byref(c))
    assert L.uaps_label_instances(None) == EINVAL
    for field in ("mask", "labels", "count", "table", "workspace"):
        assert run(_inst_call(**{field: None})) == EINVAL, field
    assert run(_inst_call(map1=4096)) == EINVAL                                             # map1 without map0
    assert run(_inst_call(connectivity=6)) == EINVAL
    assert run(_inst_call(max_instances=0)) == EINVAL
    assert run(_inst_call(min_area=0)) == EINVAL
    assert run(_inst_call(has_background=2)) == EINVAL
    assert run(_inst_call(struct_size=C.sizeof(_lib.InstancesCall) - 8)) == EINVAL          # a header without `stream`
    assert run(_inst_call(H=0)) == EINVAL
    assert run(_inst_call(workspace_bytes=64)) == EWORKSPACE
    assert run(_inst_call(B=64, H=2048, W=2048)) == ERANGE
    assert run(_inst_call(H=65536, W=32768)) == ERANGE
    assert run(_inst_call(B=4096, max_instances=8192)) == ERANGE                            # a 2 GiB table

    def rle(**kw):
        c = _lib.RleCall()
        c.struct_size = C.sizeof(_lib.RleCall)
        c.B, c.H, c.W, c.n_classes = 1, 8, 8, 2
        c.mask = c.col_offsets = c.pairs = c.offsets = c.out = 4096
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)
    for fn in (L.uaps_rle_count, L.uaps_rle_encode, L.uaps_rle_decode):
        assert fn(None) == EINVAL
        assert fn(rle(struct_size=8)) == EINVAL
        assert fn(rle(W=0)) == EINVAL
        assert fn(rle(n_classes=0)) == ERANGE and fn(rle(n_classes=9)) == ERANGE
        assert fn(rle(B=64, H=2048, W=2048)) == ERANGE
    assert L.uaps_rle_count(rle(mask=None)) == EINVAL and L.uaps_rle_count(rle(col_offsets=None)) == EINVAL
    assert L.uaps_rle_encode(rle(pairs=None)) == EINVAL
    assert L.uaps_rle_decode(rle(out=None)) == EINVAL and L.uaps_rle_decode(rle(offsets=None)) == EINVAL
    assert L.uaps_rle_decode(rle(n_runs=-1)) == EINVAL and L.uaps_rle_decode(rle(n_runs=3, pairs=None)) == EINVAL
    assert L.uaps_rle_decode(rle(out_uint8=2)) == EINVAL


def _golden():
    g = np.load(os.path.join(GOLDEN, "g13_rle.npz"))
    return [(str(n), g["mask_" + str(n)], str(g["rle_" + str(n)])) for n in g["names"]]


def test_rle_format_equals_the_reference_strings():
    from uaps_amd import format_rle, mask_to_rle, parse_rle, rle_to_mask
    cases = _golden()
    assert len(cases) >= 8 and {"blobs200", "empty", "full", "single", "last", "ragged5x7"} <= {c[0] for c in cases}
    for name, mask, text in cases:
        H, W = mask.shape
        if name == "blobs200":
            assert (H, W) == (200, 200)
        if name == "empty":
            assert text == ""
        assert R.rle_string(mask) == text, name                                             # the tests' own numpy form
        rle = mask_to_rle(torch.from_numpy(mask.astype(np.int64))[None], (1,))
        assert rle.pairs.dtype == torch.int32 and rle.offsets.tolist() == [0, rle.pairs.shape[0]]
        assert format_rle(rle.segment(0, 0)) == text, name
        pairs = parse_rle(text, (H, W))
        assert torch.equal(pairs, rle.pairs) and format_rle(pairs) == text                  # parse(format(x)) == x
        back = rle_to_mask(pairs, rle.offsets, (H, W), (1,), dtype=torch.uint8)
        assert back.dtype == torch.uint8 and np.array_equal(back[0].numpy(), mask), name    # decode(encode(mask)) == mask
        assert np.array_equal(R.decode(pairs.numpy(), H, W), mask)


def test_rle_round_trip_with_classes_and_overlap():
    from uaps_amd import mask_to_rle, rle_from_strings, rle_to_mask
    m = R.class_mask(2, 13, 7)
    classes = (1, 2, 3)
    rle = mask_to_rle(torch.from_numpy(m), classes)
    assert rle.offsets.shape == (7,) and rle.shape == (13, 7) and rle.classes == classes
    for b in range(2):
        for k, c in enumerate(classes):
            assert np.array_equal(rle.segment(b, k).numpy(), R.mask2rle_pairs(m[b] == c))
    assert np.array_equal(rle_to_mask(rle.pairs, rle.offsets, (13, 7), classes).numpy(), m)
    assert np.array_equal(mask_to_rle(torch.from_numpy(m.astype(np.uint8)), classes).pairs.numpy(), rle.pairs.numpy())
    # later classes win where annotations overlap; runs need not be sorted
    r = rle_from_strings([["3 4 1 2", "2 3"]], (3, 3), (5, 9))
    flat = np.zeros(9, dtype=np.int64)
    flat[0:2] = 5; flat[2:6] = 5; flat[1:4] = 9
    assert np.array_equal(rle_to_mask(r.pairs, r.offsets, (3, 3), (5, 9)).numpy()[0], flat.reshape(3, 3, order="F"))


def test_runs_outside_the_plane_are_refused_on_the_host():
    from uaps_amd import parse_rle, rle_from_strings, rle_to_mask
    assert parse_rle("34 2", (5, 7)).tolist() == [[34, 2]]                                   # ends at the last pixel: fine
    for bad in ("35 2", "36 1", "0 3", "1 36"):
        with pytest.raises(ValueError):
            parse_rle(bad, (5, 7))
    with pytest.raises(ValueError):
        parse_rle("1 2 3")
    with pytest.raises(ValueError):
        parse_rle("1 x")
    with pytest.raises(ValueError):
        rle_from_strings([["30 9"]], (5, 7), (1,))
    with pytest.raises(ValueError):
        rle_to_mask(torch.tensor([[30, 9]], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), (5, 7), (1,))
    assert parse_rle("").shape == (0, 2)
