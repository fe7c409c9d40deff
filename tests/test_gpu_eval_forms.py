"""-m gpu: every kernel form of the evaluation chain -- uaps_amd/csrc/instances.hip, surface.hip and match.hip -- through the C ABI,
against the references of tests/eval_form_cases.py (scipy and brute force).  Everything is an integer: every comparison is exact.

Every tensor, inputs included, is a view `off` elements into a buffer of sentinels, 64 of them at least on either side.  Outputs are
pre-filled with bytes 0xEE, the workspace is exactly the size the library reports, 256-byte aligned, pre-filled with bytes 0x7F and
followed by sentinels (for the run-length calls: exactly n + 1 words of col_offsets and 2 * total words of pairs).  After a launch every
output equals the reference in every element, every input is bit-identical, every sentinel intact; a second launch into fresh buffers
gives the same bits; a refused call leaves outputs and workspace untouched.

Which case reaches which form (tests/test_eval_form_table.py shows it from the table and the references, without a GPU):
  instances.hip
    scan_segments_kernel, second round (carry += total), partial last quad   label-scan-min1/-min3 (1,029 chunks an image);
                                                                             rle-scan-1025/-2049/-4100; one round: rle-scan-1023/-1024
    flatten_area_kernel / final_kernel, pend_b == b0 at an image boundary    label-carry-9x64-* and label-carry-8x72-* (full, rows2,
                                                                             full_empty_full): 576-pixel images, 1024-pixel waves
    tile_label_kernel / seam_merge_kernel, ragged tiles, every seam relation label-seam-17x31 / 33x16 / 16x17 / 31x18 / 17x33 x spiral, comb,
                                                                             diagonal, corners, links x connectivity 4, 8
    class values as int64 (LDS tiles, seams, background test)                label-wide-bg-m5 / -big / -absent / -none
    number_roots_kernel / final_kernel above max_instances, with maps        label-overflow-1 / -7
    fixed_q: NaN, +-inf, +-1e9 in components through a wave boundary         label-maps-1 / -2 (float views with off % 4 != 0)
    odd int32 offsets, 8-byte-only int64 offsets                             every label case but label-aligned
    rle_walk_kernel: 8 classes / 1 class, negative and > 2^32 class values   rle-scan-1024 / rle-scan-2049, rle-crossing
    H = 1, W = 1, one run through every column edge                          rle-scan-1024 and -2049, rle-w1, rle-crossing
    rle_decode_kernel: odd offsets, no runs, overlap, empty segments, clip   decode-roundtrip / -none / -overlap / -empty / -clip, each
                                                                             for an int64 and a uint8 output
  surface.hip
    col_kernel<C, false>, C = 1 .. 8                                         surf-blobs-C1 .. C8; surf-absent, surf-filled
    col_kernel row segments: nseg 1, 2, 3, 15, 16; last strip full / 1 lane  surf-seg-{16,17,32,33,240,241,256,257}x{2,64,65}
    col_kernel<1, true> for uint8 / int32 / int64 masks                      edt-seg-HxW-d1 / -d4 / -d8 (odd byte and word offsets)
    selection: ranks part in pass 0, 1, 2, not at all; N = 2; frac 0 .. 1    surf-select-0 / -50 / -95 / -100, surf-blobs-q*
    within counts: tol_d2 0, 1, 2^25; has_tolerance 0                        surf-tol-*
    argmax_kernel: C = 1, 5; ties, -0.0 against +0.0, infinities             surf-scores-C1 / -C5
    load_label: nine dtype pairs, labels outside [0, C) and negative         surf-dtype-*
  match.hip
    pair_count_kernel<4>; <1> by either pointer; <1> by H * W % 4            match-v4, match-v1-pred, match-v1-target, match-v1-hw
    a wave over many images (per-lane base)                                  match-images-70x2x2, match-images-50x1x3
    whole waves of one key across images                                     match-carry
    matrix strides, 64-column groups and 32-row rounds of the reductions     match-strides-1x1 / 1x65 / 65x1 / 33x64 / 40x129
    rows_of: count 0, negative, above the table; labels that are no row      match-counts
    ties (lowest number), inter == thr * union at 0.5 and 0.75               match-crafted-0.5 / -0.75
    class test on / off, classes outside [0, num_classes), as int64          match-agnostic-0 / -1, match-nc1, match-nc64, match-wide-classes
    zero_kernel on a stale matrix                                            every case (0x7F workspace); dense, sparse, dense on one"""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_form_cases as E
from test_gpu_ops_forms import DEV, EINVAL, ERANGE, EWORKSPACE, OK, Buf, _stream

pytestmark = pytest.mark.gpu
GUARD = 64                                    # sentinel elements in front of and behind every view
SENT = {torch.float32: -12345.0, torch.uint8: 0xA5, torch.int64: -7, torch.int32: -77777, torch.float64: -12345.0}
OUT_FILL, WS_FILL = 0xEE, 0x7F
TORCH_OF = {E.U8: torch.uint8, E.I32: torch.int32, E.I64: torch.int64}


@pytest.fixture(scope="module")
def L():
    from uaps_amd import _lib
    return _lib.lib()


class View(Buf):
    """Buf with 64 sentinels a side, int32 tensors, and a byte pattern in the view where no data is given.  The view lies `off`
    elements behind a 256-byte boundary of the address space (the buffer is a boundary longer, and the view is moved up to one)."""

    def __init__(self, shape, off: int = 0, data=None, dtype=torch.int32, fill: int = OUT_FILL):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        n = int(np.prod(shape))
        size = torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((GUARD + 256 // size + off + n + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        self.lo, self.n, self.shape, self.dtype = GUARD + (-(self.buf.data_ptr() + GUARD * size) % 256) // size + off, n, shape, dtype
        self.v = self.buf[self.lo:self.lo + n]
        self.data = None
        if data is not None:
            self.data = np.array(data).reshape(-1)      # (a copy: the case's arrays are shared and read-only)
            self.v.copy_(torch.from_numpy(self.data))
        elif n:
            self.v.view(torch.uint8).fill_(fill)

    @property
    def ptr(self):                              # (also of an empty view: the address its first element would have)
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def fetch(self):
        h = self.buf.cpu().numpy()
        s = SENT[self.dtype]
        return h[self.lo:self.lo + self.n].reshape(self.shape).copy(), bool((h[:self.lo] == s).all() and (h[self.lo + self.n:] == s).all())


def _workspace(nbytes):
    ws = View(nbytes, 0, dtype=torch.uint8, fill=WS_FILL)
    assert ws.ptr % 256 == 0
    return ws


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                      # a HIP error is sticky: launch nothing more on a device that has faulted
        if "hip" in str(e).lower():
            pytest.exit(f"the device reports {e}", returncode=3)
        raise


class Launch:
    """One call: the entry point, its struct, and every buffer it may touch."""

    def __init__(self, fn, call, ins, outs, ws=None):
        self.fn, self.call, self.ins, self.outs, self.ws = fn, call, ins, outs, ws

    def fire(self, extra: int = 0):
        self.call.struct_size = C.sizeof(self.call) + extra
        self.call.stream = _stream()
        return self.fn(C.byref(self.call))

    def collect(self):
        """(outputs on the host, failed checks): sentinels of everything, inputs bit-identical."""
        _sync()
        got, bad = {}, []
        for k, b in self.outs.items():
            got[k], ok = b.fetch()
            if not ok:
                bad.append(f"the sentinels around {k} were written")
        for k, b in self.ins.items():
            h, ok = b.fetch()
            if not ok:
                bad.append(f"the sentinels around the input {k} were written")
            if h.tobytes() != b.data.tobytes():
                bad.append(f"the input {k} was changed")
        if self.ws is not None and not self.ws.fetch()[1]:
            bad.append("bytes behind (or in front of) the reported workspace size were written")
        return got, bad

    def snapshot(self):
        bufs = dict(self.outs)
        if self.ws is not None:
            bufs["workspace"] = self.ws
        return {k: b.buf.clone() for k, b in bufs.items()}, bufs


def _size(fn, *dims):
    n = C.c_size_t()
    assert fn(*dims, C.byref(n)) == OK
    return n.value


# ---- one preparation per entry point ----------------------------------------------------------------------------------------------------
def prep_label(L, c, inp):
    from uaps_amd import _lib
    B, H, W = c.shape
    M = c.arg("max_instances", 64)
    ins = {k: View(c.shape, c.off(k), v, torch.int64 if k == "mask" else torch.float32) for k, v in inp.items()}
    outs = dict(labels=View(c.shape, c.off("labels")), count=View(B, c.off("count")), table=View((B, M, 9), c.off("table"), dtype=torch.int64))
    ws = _workspace(_size(L.uaps_instances_workspace_bytes, B, H, W))
    k = _lib.InstancesCall()
    k.B, k.H, k.W, k.connectivity, k.min_area, k.max_instances = B, H, W, c.arg("connectivity", 8), c.arg("min_area", 1), M
    bg = c.arg("background", 0)
    k.has_background, k.background = (0, 0) if bg is None else (1, bg)
    k.mask, k.labels, k.count, k.table = ins["mask"].ptr, outs["labels"].ptr, outs["count"].ptr, outs["table"].ptr
    k.map0, k.map1 = (ins[m].ptr if m in ins else None for m in ("map0", "map1"))
    k.workspace, k.workspace_bytes = ws.ptr, ws.n
    return Launch(L.uaps_label_instances, k, ins, outs, ws)


def _rle_call(c):
    from uaps_amd import _lib
    k = _lib.RleCall()
    classes = c.arg("classes")
    k.B, k.H, k.W, k.n_classes = *c.shape, len(classes)
    for i, v in enumerate(classes):
        k.classes[i] = v
    return k


def prep_rle_count(L, c, inp):
    B, H, W = c.shape
    n = B * len(c.arg("classes")) * W
    ins = dict(mask=View(c.shape, c.off("mask"), inp["mask"], torch.int64))
    outs = dict(col_offsets=View(n + 1, c.off("col_offsets"), fill=WS_FILL))
    k = _rle_call(c)
    k.mask, k.col_offsets = ins["mask"].ptr, outs["col_offsets"].ptr
    return Launch(L.uaps_rle_count, k, ins, outs)


def prep_rle_encode(L, c, inp, col_offsets):
    """col_offsets: what uaps_rle_count wrote (host); the pairs are exactly 2 * total words."""
    ins = dict(mask=View(c.shape, c.off("mask"), inp["mask"], torch.int64), col_offsets=View(len(col_offsets), c.off("col_offsets"), col_offsets))
    outs = dict(pairs=View((int(col_offsets[-1]), 2), c.off("pairs"), fill=WS_FILL))
    k = _rle_call(c)
    k.mask, k.col_offsets, k.pairs = ins["mask"].ptr, ins["col_offsets"].ptr, outs["pairs"].ptr
    return Launch(L.uaps_rle_encode, k, ins, outs)


def prep_decode(L, c, inp):
    u8 = int(c.arg("uint8", 0))
    ins = dict(pairs=View(inp["pairs"].shape, c.off("pairs"), inp["pairs"]), offsets=View(len(inp["offsets"]), c.off("offsets"), inp["offsets"]))
    outs = dict(out=View(c.shape, c.off("out"), dtype=torch.uint8 if u8 else torch.int64))
    k = _rle_call(c)
    k.pairs, k.offsets, k.n_runs, k.out, k.out_uint8 = ins["pairs"].ptr, ins["offsets"].ptr, len(inp["pairs"]), outs["out"].ptr, u8
    return Launch(L.uaps_rle_decode, k, ins, outs)


def prep_edt(L, c, inp):
    from uaps_amd import _lib
    B, H, W = c.shape
    d = c.arg("dtype")
    mask = np.where(inp["mask"], E.EDT_VALUE[d], 0).astype(E.NP_OF[d])
    ins = dict(mask=View(c.shape, c.off("mask"), mask, TORCH_OF[d]))
    outs = dict(out=View(c.shape, c.off("out")))
    ws = _workspace(_size(L.uaps_edt_workspace_bytes, B, H, W))
    k = _lib.EdtCall()
    k.B, k.H, k.W, k.mask_dtype, k.mask, k.out, k.workspace, k.workspace_bytes = B, H, W, d, ins["mask"].ptr, outs["out"].ptr, ws.ptr, ws.n
    return Launch(L.uaps_edt_sq, k, ins, outs, ws)


def prep_surface(L, c, inp):
    from uaps_amd import _lib
    B, H, W = c.shape
    Cc, dp, dt = c.arg("C"), c.arg("pred_dtype", E.I64), c.arg("target_dtype", E.I64)
    ins = dict(target=View(c.shape, c.off("target"), inp["target"].astype(E.NP_OF[dt]), TORCH_OF[dt]))
    k = _lib.SurfaceCall()
    if c.arg("scores"):
        ins["scores"] = View((B, Cc, H, W), c.off("scores"), inp["scores"], torch.float32)
        k.pred, k.pred_scores = None, ins["scores"].ptr
    else:
        ins["pred"] = View(c.shape, c.off("pred"), inp["pred"].astype(E.NP_OF[dp]), TORCH_OF[dp])
        k.pred, k.pred_scores = ins["pred"].ptr, None
    outs = dict(table=View((B, Cc, 12), c.off("table"), dtype=torch.int64))
    ws = _workspace(_size(L.uaps_surface_workspace_bytes, B, Cc, H, W))
    k.B, k.C, k.H, k.W, k.pred_dtype, k.target_dtype, k.target = B, Cc, H, W, dp, dt, ins["target"].ptr
    k.percentile_frac, k.has_tolerance, k.tol_d2 = c.arg("percentile", 95.0) / 100.0, c.arg("has_tolerance", 0), c.arg("tol_d2", 0)
    k.table, k.workspace, k.workspace_bytes = outs["table"].ptr, ws.ptr, ws.n
    return Launch(L.uaps_surface_distances, k, ins, outs, ws)


def prep_match(L, c, inp, ws=None):
    from uaps_amd import _lib
    B, H, W = c.shape
    mp, mg, nc = c.arg("max_pred"), c.arg("max_gt"), c.arg("num_classes", 4)
    ins = {k: View(v.shape, c.off(k), v, torch.int64 if k.endswith("table") else torch.int32) for k, v in inp.items()}
    for name in ("pred_labels", "target_labels"):
        assert ins[name].ptr % 16 == 4 * c.off(name) % 16
    outs = dict(pred_out=View((B, mp, 4), c.off("pred_out"), dtype=torch.int64), target_out=View((B, mg, 4), c.off("target_out"), dtype=torch.int64),
                counts=View((B, nc, 3), c.off("counts"), dtype=torch.int64))
    need = _size(L.uaps_match_workspace_bytes, B, mp, mg)
    ws = ws if ws is not None else _workspace(need)
    k = _lib.MatchCall()
    k.B, k.H, k.W, k.num_classes, k.class_agnostic, k.iou_threshold = B, H, W, nc, c.arg("agnostic", 0), c.arg("thr", 0.5)
    for name, b in ins.items():
        setattr(k, name, b.ptr)
    k.max_pred, k.max_gt, k.pred_out, k.target_out, k.counts = mp, mg, outs["pred_out"].ptr, outs["target_out"].ptr, outs["counts"].ptr
    k.workspace, k.workspace_bytes = ws.ptr, need
    return Launch(L.uaps_match_instances, k, ins, outs, ws)


PREP = dict(label=prep_label, decode=prep_decode, edt=prep_edt, surface=prep_surface, match=prep_match)


def _run_rle(L, c, inp, extra=0):
    """uaps_rle_count into exactly n + 1 words, then uaps_rle_encode into exactly 2 * total words."""
    cnt = prep_rle_count(L, c, inp)
    assert cnt.fire(extra) == OK
    got, bad = cnt.collect()
    total = int(got["col_offsets"][-1])
    if not 0 <= total <= inp["mask"].size:      # (never size a buffer from a number the call under test got wrong)
        return got, bad + [f"total {total}"]
    enc = prep_rle_encode(L, c, inp, got["col_offsets"])
    assert enc.fire(extra) == OK
    got2, bad2 = enc.collect()
    got.update(got2)
    return got, bad + bad2


def _launch(L, c, extra=0):
    """One run of the case on fresh buffers: (outputs on the host, failed checks)."""
    inp = E.inputs(c)
    if c.entry == "rle":
        return _run_rle(L, c, inp, extra)
    la = PREP[c.entry](L, c, inp)
    assert la.fire(extra) == OK
    return la.collect()


def run_case(L, c):
    got, bad = _launch(L, c)
    bad = bad + E.compare(E.reference(c), got)
    again, _ = _launch(L, c)
    return got, bad + [f"a second launch differs in {k}" for k in got if got[k].tobytes() != again[k].tobytes()]


def _check(L, cid):
    got, bad = run_case(L, E.BY_ID[cid])
    assert not bad, bad
    return got


@pytest.mark.parametrize("cid", E.ids("label"))
def test_label_instances(L, cid):
    got = _check(L, cid)
    c = E.BY_ID[cid]
    if "carry-image-boundary" in c.forms and c.pattern != "rows2":      # per image, not the sum of two
        hw = c.shape[1] * c.shape[2]
        assert got["table"][0, 0, 1] == hw and got["table"][2, 0, 1] == hw


@pytest.mark.parametrize("cid", E.ids("rle"))
def test_rle_count_and_encode(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("decode"))
def test_rle_decode(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("edt"))
def test_edt_sq(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("surface"))
def test_surface_distances(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", [i for i in E.ids("match") if i != E.SPARSE_CASE.id])
def test_match_instances(L, cid):
    _check(L, cid)


def test_match_forms_give_the_same_tables(L):
    """V = 4, V = 1 by the prediction's pointer, V = 1 by the target's: one set of data, one set of tables."""
    got = [_launch(L, E.BY_ID[i])[0] for i in ("match-v4", "match-v1-pred", "match-v1-target")]
    for g in got[1:]:
        assert all(g[k].tobytes() == got[0][k].tobytes() for k in got[0])
    assert not E.compare(E.reference(E.BY_ID["match-v4"]), got[0])


def test_match_dense_sparse_dense_on_one_workspace(L):
    cases = [E.BY_ID[i] for i in E.STALE]
    ws = _workspace(max(_size(L.uaps_match_workspace_bytes, c.shape[0], c.arg("max_pred"), c.arg("max_gt")) for c in cases))
    for c in cases:
        la = prep_match(L, c, E.inputs(c), ws)
        assert la.fire() == OK
        got, bad = la.collect()
        assert not bad + E.compare(E.reference(c), got), c.id


# ---- struct_size above this version's: the call runs ------------------------------------------------------------------------------------
LATER = ("label-aligned", "rle-aligned", "decode-overlap-i64", "edt-seg-17x65-d4", "surf-aligned", "match-crafted-0.5")


@pytest.mark.parametrize("cid", LATER)
def test_a_later_headers_struct_size_still_runs(L, cid):
    c = E.BY_ID[cid]
    got, bad = _launch(L, c, extra=64)
    assert not bad + E.compare(E.reference(c), got)


# ---- refusals: nothing launched, nothing written ----------------------------------------------------------------------------------------
# (entry, case, what is wrong, the code tests/test_instances_host.py, test_surface_host.py and test_match_host.py pin for it)
REFUSALS = [
    ("label", "label-aligned", dict(labels=None), EINVAL), ("label", "label-aligned", dict(connectivity=6), EINVAL),
    ("label", "label-aligned", "short", EWORKSPACE), ("label", "label-aligned", "v0", EINVAL),
    ("count", "rle-aligned", dict(col_offsets=None), EINVAL), ("count", "rle-aligned", dict(n_classes=9), ERANGE), ("count", "rle-aligned", "v0", EINVAL),
    ("encode", "rle-aligned", dict(pairs=None), EINVAL), ("encode", "rle-aligned", dict(n_classes=0), ERANGE), ("encode", "rle-aligned", "v0", EINVAL),
    ("decode", "decode-overlap-i64", dict(out=None), EINVAL), ("decode", "decode-overlap-i64", dict(out_uint8=2), EINVAL),
    ("decode", "decode-overlap-i64", dict(n_classes=9), ERANGE), ("decode", "decode-overlap-i64", "v0", EINVAL),
    ("edt", "edt-seg-17x65-d4", dict(out=None), EINVAL), ("edt", "edt-seg-17x65-d4", dict(mask_dtype=2), EINVAL),
    ("edt", "edt-seg-17x65-d4", "short", EWORKSPACE), ("edt", "edt-seg-17x65-d4", "v0", EINVAL),
    ("surface", "surf-aligned", dict(table=None), EINVAL), ("surface", "surf-aligned", dict(pred_dtype=2), EINVAL),
    ("surface", "surf-aligned", dict(C=9), ERANGE), ("surface", "surf-aligned", "short", EWORKSPACE), ("surface", "surf-aligned", "v0", EINVAL),
    ("match", "match-crafted-0.5", dict(counts=None), EINVAL), ("match", "match-crafted-0.5", dict(class_agnostic=2), EINVAL),
    ("match", "match-crafted-0.5", dict(num_classes=65), ERANGE), ("match", "match-crafted-0.5", "short", EINVAL),
    ("match", "match-crafted-0.5", "v0", EINVAL)]


def _refusal_id(r):
    return f"{r[0]}-{r[2] if isinstance(r[2], str) else '-'.join(r[2])}"


@pytest.mark.parametrize("entry,cid,wrong,code", REFUSALS, ids=[_refusal_id(r) for r in REFUSALS])
def test_refusals_write_nothing(L, entry, cid, wrong, code):
    c = E.BY_ID[cid]
    inp = E.inputs(c)
    if entry == "count":
        la = prep_rle_count(L, c, inp)
    elif entry == "encode":
        la = prep_rle_encode(L, c, inp, E.reference(c)["col_offsets"])
    else:
        la = PREP[entry](L, c, inp)
    extra = 0
    if wrong == "short":
        la.call.workspace_bytes -= 1
    elif wrong == "v0":
        extra = -8                                 # a header that ends in front of `stream`
    else:
        for k, v in wrong.items():
            setattr(la.call, k, v)
    before, bufs = la.snapshot()
    rc = la.fire(extra)
    _sync()
    assert rc == code, rc
    wrote = [k for k, b in bufs.items() if not torch.equal(b.buf, before[k])]
    assert not wrote, f"a refused call wrote {wrote}"
