"""-m gpu: every kernel form of the inference side -- uaps_amd/csrc/tta.hip, tiled.hip and curves.hip -- through the C ABI, against the
references of tests/infer_form_cases.py: tests/curves_ref.py (integers, exact; pro_sum bit for bit) and the float64 walks of the two
folds with their derived per-element bars.

Every tensor, inputs included, is a view `off` elements into a buffer of sentinels, 64 of them at least on either side (the View of
tests/test_gpu_eval_forms.py).  Outputs are pre-filled with bytes 0xEE, the curves workspace is exactly the size the library reports,
256-byte aligned, pre-filled with bytes 0x7F and followed by sentinels; every chunk of tiles is a buffer of its own.  After a launch
every output equals the reference (exactly, or within the bar), the mask is the lowest-index arg-max of the launch's own probs and conf
the picked value, every input is bit-identical, every sentinel intact; a second launch into fresh buffers gives the same bits; the tiled
fold gives the same bits under another chunking; a refused call leaves outputs and workspace untouched.

Which case reaches which form: tests/test_infer_form_table.py shows it from the table and the references, without a GPU."""
import dataclasses
import re

import pytest
import torch

import infer_form_cases as E
from test_gpu_eval_forms import L, Launch, View, _size, _sync, _workspace  # noqa: F401  (L: the fixture)
from test_gpu_ops_forms import EINVAL, ERANGE, OK

pytestmark = pytest.mark.gpu
TORCH_OF = {E.U8: torch.uint8, E.I32: torch.int32, E.I64: torch.int64}
F32, I64 = torch.float32, torch.int64


def _in(c, name, data, dtype=F32):
    return View(data.shape, c.off(name), data, dtype)


# ---- one preparation per entry point ----------------------------------------------------------------------------------------------------
def prep_tta_fold(L, c, inp, tpc=None):
    from uaps_amd import _lib
    a = c.arg
    B, Cc, H, W = a("B", 2), a("C"), a("H"), a("W")
    ins = {k: _in(c, k, v) for k, v in inp.items()}
    shapes = dict(probs=((B, Cc, H, W), F32), mask=((B, H, W), I64), conf=((B, H, W), F32))
    outs = {k: View(shapes[k][0], c.off(k), dtype=shapes[k][1]) for k in c.outs}
    k = _lib.TTAFoldCall()
    k.S, k.B, k.C, k.H, k.W, k.flip = len(a("sizes")), B, Cc, H, W, a("flip", 1)
    for s, (h, w) in enumerate(a("sizes")):
        k.logits[s], k.h[s], k.w[s] = ins[f"z{s}"].ptr, h, w
    k.probs_sum, k.mask, k.conf = (outs[n].ptr if n in outs else None for n in ("probs", "mask", "conf"))
    return Launch(L.uaps_tta_fold, k, ins, outs)


def prep_tta_views(L, c, inp, tpc=None):
    from uaps_amd import _lib
    a = c.arg
    B, Cin, flip = a("B", 2), a("Cin"), a("flip", 1)
    ins = dict(x=_in(c, "x", inp["x"]))
    outs = dict(out=View(((2 if flip or a("buf2") else 1) * B, Cin, a("h"), a("w")), c.off("out"), dtype=F32))
    k = _lib.TTAViewsCall()
    k.B, k.Cin, k.H, k.W, k.h, k.w, k.flip, k.x, k.out = B, Cin, a("H"), a("W"), a("h"), a("w"), flip, ins["x"].ptr, outs["out"].ptr
    return Launch(L.uaps_tta_views, k, ins, outs)


def prep_tile_cut(L, c, inp, tpc=None):
    from uaps_amd import _lib
    a = c.arg
    g0, g1 = a("g0", 0), a("g1", None) or E.n_tiles(c)
    ins = dict(x=_in(c, "x", inp["x"]))
    outs = dict(out=View((g1 - g0, a("Cin")) + a("tile"), c.off("out"), dtype=F32))
    k = _lib.TileCutCall()
    k.B, k.Cin, k.H, k.W, (k.th, k.tw), (k.oy, k.ox), k.g0, k.g1 = a("B", 2), a("Cin"), a("H"), a("W"), a("tile"), a("overlap"), g0, g1
    k.x, k.out = ins["x"].ptr, outs["out"].ptr
    return Launch(L.uaps_tile_cut, k, ins, outs)


def prep_tile_fold(L, c, inp, tpc=None):
    """tpc: the tiles of a chunk (the case's own by default); every chunk is a buffer of its own."""
    from uaps_amd import _lib
    a = c.arg
    B, Cc, H, W, n_maps, G = a("B", 2), a("C"), a("H"), a("W"), a("n_maps", 0), E.n_tiles(c)
    tpc = tpc or a("tpc")
    n_chunks = -(-G // tpc)
    ins = dict(wy=_in(c, "wy", inp["wy"]), wx=_in(c, "wx", inp["wx"]))
    k = _lib.TileFoldCall()
    for j in range(n_chunks):
        if Cc:
            ins[f"z.{j}"] = View(inp["z"][j * tpc:(j + 1) * tpc].shape, c.off("z"), inp["z"][j * tpc:(j + 1) * tpc], F32)
            k.logits[j] = ins[f"z.{j}"].ptr
        for m in range(n_maps):
            ins[f"m{m}.{j}"] = View(inp[f"m{m}"][j * tpc:(j + 1) * tpc].shape, c.off(f"m{m}"), inp[f"m{m}"][j * tpc:(j + 1) * tpc], F32)
            k.maps[m][j] = ins[f"m{m}.{j}"].ptr
    shapes = dict(probs=((B, Cc, H, W), F32), mask=((B, H, W), I64), conf=((B, H, W), F32), map0=((B, H, W), F32), map1=((B, H, W), F32))
    outs = {n: View(shapes[n][0], c.off(n), dtype=shapes[n][1]) for n in c.outs}
    k.B, k.C, k.H, k.W, (k.th, k.tw), (k.oy, k.ox) = B, Cc, H, W, a("tile"), a("overlap")
    k.n_chunks, k.tiles_per_chunk, k.n_maps, k.wy, k.wx = n_chunks, tpc, n_maps, ins["wy"].ptr, ins["wx"].ptr
    k.probs, k.mask, k.conf = (outs[n].ptr if n in outs else None for n in ("probs", "mask", "conf"))
    for m in range(n_maps):
        k.map_out[m] = outs[f"map{m}"].ptr
    return Launch(L.uaps_tile_fold, k, ins, outs)


def prep_score(L, c, inp, tpc=None):
    from uaps_amd import _lib
    a = c.arg
    B, Cc, H, W, bins, cls, tdt = a("B", 2), a("C"), a("H"), a("W"), a("bins", 64), a("classes", ()), a("tdt", E.I64)
    R = c.R
    ins = dict(scores=_in(c, "scores", inp["scores"]), target=_in(c, "target", inp["target"], TORCH_OF[tdt]))
    assert ins["scores"].ptr % 16 == 4 * c.off("scores") % 16 and ins["target"].ptr % 16 == tdt * c.off("target") % 16
    outs = dict(hist=View((B, R, 2, bins), c.off("hist"), dtype=I64), nan=View((B, R), c.off("nan"), dtype=I64))
    if a("qsum", 0):
        outs["qsum"] = View((B, R, 2, bins), c.off("qsum"), dtype=I64)
    k = _lib.CurvesCall()
    k.B, k.C, k.H, k.W, k.bins, k.from_logits, k.top_row, k.n_classes = B, Cc, H, W, bins, a("from_logits", 0), a("top", 1), len(cls)
    for i, v in enumerate(cls):
        k.classes[i] = v
    k.target_dtype, k.lo, k.hi, k.scores, k.target = tdt, a("lo", 0.0), a("hi", 1.0), ins["scores"].ptr, ins["target"].ptr
    ws = None
    if a("regions"):
        Mg = inp["rtable"].shape[1]
        ins.update(rl=_in(c, "rl", inp["rl"], torch.int32), rcount=_in(c, "rcount", inp["rcount"], torch.int32),
                   rtable=_in(c, "rtable", inp["rtable"], I64))
        outs.update(pro_sum=View((B, len(cls), bins), c.off("pro_sum"), dtype=torch.float64),
                    n_regions=View((B, len(cls)), c.off("n_regions"), dtype=I64))
        ws = _workspace(_size(L.uaps_curves_workspace_bytes, B, Mg, bins))
        k.region_labels, k.region_count, k.region_table, k.max_regions = ins["rl"].ptr, ins["rcount"].ptr, ins["rtable"].ptr, Mg
        k.pro_sum, k.n_regions, k.workspace, k.workspace_bytes = outs["pro_sum"].ptr, outs["n_regions"].ptr, ws.ptr, ws.n
    k.hist, k.nan, k.qsum = outs["hist"].ptr, outs["nan"].ptr, outs["qsum"].ptr if "qsum" in outs else None
    return Launch(L.uaps_score_curves, k, ins, outs, ws)


def prep_plane(L, c, inp, tpc=None):
    from uaps_amd import _lib
    a = c.arg
    B, H, W, bins, pdt, tdt = a("B", 2), a("H"), a("W"), a("bins", 64), a("pdt", E.I64), a("tdt", E.I64)
    ins = dict(scores=_in(c, "scores", inp["scores"]), pred=_in(c, "pred", inp["pred"], TORCH_OF[pdt]),
               target=_in(c, "target", inp["target"], TORCH_OF[tdt]))
    outs = dict(hist=View((B, 1, 2, bins), c.off("hist"), dtype=I64), nan=View((B, 1), c.off("nan"), dtype=I64))
    if a("qsum", 0):
        outs["qsum"] = View((B, 1, 2, bins), c.off("qsum"), dtype=I64)
    k = _lib.PlaneCurvesCall()
    k.B, k.H, k.W, k.bins, k.from_logits, k.pred_dtype, k.target_dtype, k.lo, k.hi = B, H, W, bins, 0, pdt, tdt, a("lo", 0.0), a("hi", 1.0)
    k.score, k.pred, k.target = ins["scores"].ptr, ins["pred"].ptr, ins["target"].ptr
    k.hist, k.nan, k.qsum = outs["hist"].ptr, outs["nan"].ptr, outs["qsum"].ptr if "qsum" in outs else None
    return Launch(L.uaps_plane_curves, k, ins, outs)


PREP = dict(tta_fold=prep_tta_fold, tta_views=prep_tta_views, tile_cut=prep_tile_cut, tile_fold=prep_tile_fold, score=prep_score,
            plane=prep_plane)


def _launch(L, c, extra=0, tpc=None):
    """One run of the case on fresh buffers: (outputs on the host, failed checks)."""
    la = PREP[c.entry](L, c, E.inputs(c), tpc)
    assert la.fire(extra) == OK
    return la.collect()


def _full(c):
    """The same data with every class output asked for."""
    return dataclasses.replace(c, args=tuple(kv for kv in c.args if kv[0] != "outs"), offs=())


def run_case(L, c):
    """(outputs, failed checks, name -> largest error / bar): two launches on fresh buffers, and for a fold without probs one more that
    asks for every output, whose mask and conf must be the same bits."""
    got, bad = _launch(L, c)
    own = None
    if c.entry in ("tta_fold", "tile_fold") and c.arg("C") and "probs" not in c.outs:
        full, bad_full = _launch(L, _full(c))
        bad = bad + bad_full + [f"{k} differs from the launch with every output" for k in got if got[k].tobytes() != full[k].tobytes()]
        own = full["probs"]
    more, ratios = E.compare(c, got, own)
    again, _ = _launch(L, c)
    bad = bad + more + [f"a second launch differs in {k}" for k in got if got[k].tobytes() != again[k].tobytes()]
    return got, bad, ratios


def _check(L, cid):
    got, bad, ratios = run_case(L, E.BY_ID[cid])
    print(cid, " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))
    assert not bad, bad
    return got


@pytest.mark.parametrize("cid", E.ids("tta_fold"))
def test_tta_fold(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("tta_views"))
def test_tta_views(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("tile_cut"))
def test_tile_cut(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("tile_fold"))
def test_tile_fold(L, cid):
    got = _check(L, cid)
    c = E.BY_ID[cid]
    G = E.n_tiles(c)
    other, bad = _launch(L, c, tpc=G if c.arg("tpc") < G else -(-G // 2))              # another chunking of the same tiles
    assert not bad and all(other[k].tobytes() == got[k].tobytes() for k in got), "two chunkings differ"


@pytest.mark.parametrize("cid", E.ids("score"))
def test_score_curves(L, cid):
    _check(L, cid)


@pytest.mark.parametrize("cid", E.ids("plane"))
def test_plane_curves(L, cid):
    _check(L, cid)


# ---- struct_size above this version's: the call runs and gives the same bits ------------------------------------------------------------
LATER = ("tta-c4-v4", "views-up", "cut-clamp", "fold-c4-maps2", "score-regions-c4-v4", "plane-d4-d8-v4")


@pytest.mark.parametrize("cid", LATER)
def test_a_later_headers_struct_size_still_runs(L, cid):
    c = E.BY_ID[cid]
    got, bad = _launch(L, c, extra=64)
    more, _ = E.compare(c, got)
    plain, _ = _launch(L, c)
    assert not bad + more and all(got[k].tobytes() == plain[k].tobytes() for k in got)


# ---- refusals: nothing launched, nothing written ----------------------------------------------------------------------------------------
# (case, what is wrong, the code the header documents).  "null": no struct at all; "v0": a header that ends in front of `stream`; "short" /
# "shifted": the workspace; "maps1_3": maps[1][3]; TINY_RANGE: hi - lo a denormal, so that inv = bins / (hi - lo) is not finite.
TINY_RANGE = dict(lo=0.0, hi=1e-45)
BIG = dict(H=1 << 15, W=1 << 15)                # 2^30 pixels an image: every tensor over them is 2 GiB or more
NONE3 = dict(probs_sum=None, mask=None, conf=None)
REFUSALS = [
    ("views-up", dict(x=None), EINVAL), ("views-up", dict(out=None), EINVAL), ("views-up", dict(flip=2), EINVAL), ("views-up", dict(B=0), EINVAL),
    ("views-up", dict(h=0), EINVAL), ("views-up", dict(H=65536, W=65536), ERANGE), ("views-up", "v0", EINVAL), ("views-up", "null", EINVAL),
    ("tta-c4-v4", NONE3, EINVAL), ("tta-c4-v4", dict(logits1=None), EINVAL), ("tta-c4-v4", dict(flip=-1), EINVAL), ("tta-c4-v4", dict(H=0), EINVAL),
    ("tta-c4-v4", dict(h0=0), EINVAL), ("tta-c4-v4", dict(C=1), ERANGE), ("tta-c4-v4", dict(C=9), ERANGE), ("tta-c4-v4", dict(S=0), ERANGE),
    ("tta-c4-v4", dict(S=9), ERANGE), ("tta-c4-v4", BIG, ERANGE), ("tta-c4-v4", "v0", EINVAL), ("tta-c4-v4", "null", EINVAL),
    ("cut-clamp", dict(x=None), EINVAL), ("cut-clamp", dict(out=None), EINVAL), ("cut-clamp", dict(Cin=0), EINVAL), ("cut-clamp", dict(oy=-1), EINVAL),
    ("cut-clamp", dict(oy=9), ERANGE), ("cut-clamp", dict(g1=0), EINVAL), ("cut-clamp", dict(g1=33), EINVAL), ("cut-clamp", dict(g0=-1), EINVAL),
    ("cut-clamp", "v0", EINVAL), ("cut-clamp", "null", EINVAL), ("cut-clamp", BIG, ERANGE), ("cut-clamp", dict(g1=1, th=1 << 15, tw=1 << 15), ERANGE),
    ("fold-c4-maps2", dict(wy=None), EINVAL), ("fold-c4-maps2", dict(wx=None), EINVAL), ("fold-c4-maps2", dict(C=0), EINVAL),
    ("fold-c4-maps2", dict(n_maps=-1), EINVAL), ("fold-c4-maps2", dict(C=-1), EINVAL), ("fold-c4-maps2", dict(logits0=None), EINVAL), ("fold-c4-maps2", dict(map_out1=None), EINVAL),
    ("fold-c4-maps2", dict(n_chunks=5), EINVAL), ("fold-c4-maps2", dict(n_chunks=3), EINVAL), ("fold-c4-maps2", dict(tiles_per_chunk=0), EINVAL),
    ("fold-c4-maps2", dict(probs=None, mask=None, conf=None), EINVAL), ("fold-c4-maps2", dict(W=0), EINVAL), ("fold-c4-maps2", dict(C=1), ERANGE),
    ("fold-c4-maps2", dict(C=9), ERANGE), ("fold-c4-maps2", dict(n_maps=3), ERANGE), ("fold-c4-maps2", dict(n_chunks=33), ERANGE),
    ("fold-c4-maps2", dict(ox=5), ERANGE), ("fold-c4-maps2", "v0", EINVAL), ("fold-c4-maps2", "null", EINVAL), ("fold-c4-maps2", dict(maps1_3=None), EINVAL),
    ("fold-c4-maps2", dict(maps0_0=None), EINVAL), ("fold-c4-maps2", dict(logits3=None), EINVAL), ("fold-c4-maps2", BIG, ERANGE),
    ("fold-maps1-v4", BIG, ERANGE), ("fold-maps1-v4", dict(maps0_2=None), EINVAL), ("fold-maps1-v4", dict(map_out0=None), EINVAL),
    ("fold-maps1-v4", dict(n_maps=0), EINVAL),
    ("score-regions-c4-v4", dict(scores=None), EINVAL), ("score-regions-c4-v4", dict(target=None), EINVAL), ("score-regions-c4-v4", dict(hist=None), EINVAL),
    ("score-regions-c4-v4", dict(nan=None), EINVAL), ("score-regions-c4-v4", dict(B=0), EINVAL), ("score-regions-c4-v4", dict(from_logits=2), EINVAL),
    ("score-regions-c4-v4", dict(top_row=2), EINVAL), ("score-regions-c4-v4", dict(target_dtype=2), EINVAL), ("score-regions-c4-v4", dict(n_classes=9), EINVAL),
    ("score-regions-c4-v4", dict(n_classes=0, top_row=0), EINVAL), ("score-regions-c4-v4", dict(classes0=4), EINVAL), ("score-regions-c4-v4", dict(classes1=-1), EINVAL),
    ("score-regions-c4-v4", dict(lo=1.0), EINVAL), ("score-regions-c4-v4", dict(lo=float("nan")), EINVAL), ("score-regions-c4-v4", dict(hi=float("inf")), EINVAL),
    ("score-regions-c4-v4", dict(pro_sum=None), EINVAL), ("score-regions-c4-v4", dict(region_count=None), EINVAL), ("score-regions-c4-v4", dict(max_regions=0), EINVAL),
    ("score-regions-c4-v4", "short", EINVAL), ("score-regions-c4-v4", "shifted", EINVAL), ("score-regions-c4-v4", dict(workspace=None), EINVAL),
    ("score-regions-c4-v4", dict(C=0), ERANGE), ("score-regions-c4-v4", dict(C=9), ERANGE), ("score-regions-c4-v4", dict(bins=1), ERANGE),
    ("score-regions-c4-v4", dict(bins=4097), ERANGE), ("score-regions-c4-v4", dict(H=1 << 16, W=1 << 15), ERANGE), ("score-regions-c4-v4", "v0", EINVAL), ("score-regions-c4-v4", "null", EINVAL),
    ("score-regions-c4-v4", TINY_RANGE, EINVAL), ("score-regions-c4-v4", dict(n_classes=-1), EINVAL), ("score-regions-c4-v4", dict(region_labels=None), EINVAL),
    ("score-regions-c4-v4", dict(region_table=None), EINVAL), ("score-regions-c4-v4", dict(n_regions=None), EINVAL), ("score-regions-c4-v4", BIG, ERANGE),
    ("score-c1-v4-q1", dict(classes0=0), EINVAL),
    ("plane-d4-d8-v4", dict(score=None), EINVAL), ("plane-d4-d8-v4", dict(pred=None), EINVAL), ("plane-d4-d8-v4", dict(target=None), EINVAL),
    ("plane-d4-d8-v4", dict(hist=None), EINVAL), ("plane-d4-d8-v4", dict(nan=None), EINVAL), ("plane-d4-d8-v4", dict(from_logits=1), EINVAL),
    ("plane-d4-d8-v4", dict(pred_dtype=2), EINVAL), ("plane-d4-d8-v4", dict(target_dtype=0), EINVAL), ("plane-d4-d8-v4", dict(W=-1), EINVAL),
    ("plane-d4-d8-v4", dict(hi=-2.5), EINVAL), ("plane-d4-d8-v4", dict(bins=1), ERANGE), ("plane-d4-d8-v4", dict(bins=4097), ERANGE),
    ("plane-d4-d8-v4", "v0", EINVAL), ("plane-d4-d8-v4", "null", EINVAL), ("plane-d4-d8-v4", TINY_RANGE, EINVAL),
    ("plane-d4-d8-v4", dict(H=1 << 16, W=1 << 15), ERANGE), ("plane-d4-d8-v4", BIG, ERANGE)]


def _refusal_id(r):
    return f"{r[0]}-{r[1] if isinstance(r[1], str) else '-'.join(f'{k}={v}' for k, v in r[1].items())}"


def _set(call, name, v):
    """A field, an element of an array field ("logits3") or of a two-dimensional one ("maps1_3")."""
    m = re.fullmatch(r"([a-z_]+?)(\d+)(?:_(\d+))?", name)
    if m and hasattr(call, m.group(1)) and not hasattr(call, name):
        field = getattr(call, m.group(1))
        if m.group(3) is None:
            field[int(m.group(2))] = v
        else:
            field[int(m.group(2))][int(m.group(3))] = v
    else:
        setattr(call, name, v)


@pytest.mark.parametrize("cid,wrong,code", REFUSALS, ids=[_refusal_id(r) for r in REFUSALS])
def test_refusals_write_nothing(L, cid, wrong, code):
    c = E.BY_ID[cid]
    la = PREP[c.entry](L, c, E.inputs(c))
    extra = 0
    if wrong == "short":
        la.call.workspace_bytes -= 1
    elif wrong == "shifted":
        la.call.workspace += 16
    elif wrong == "v0":
        extra = -8
    elif wrong != "null":
        for k, v in wrong.items():
            _set(la.call, k, v)
    before, bufs = la.snapshot()
    rc = la.fn(None) if wrong == "null" else la.fire(extra)
    _sync()
    assert rc == code, rc
    wrote = [k for k, b in bufs.items() if not torch.equal(b.buf, before[k])]
    assert not wrote, f"a refused call wrote {wrote}"
