"""GPU parity of the target encoders (csrc/painter_paint.hip through the C ABI of include/painter_paint.h and through
painter_amd/painter_engine.py) against tests/painter_paint_host.py -- the definition -- and against the pictures the unmodified reference
generators produced (tests/golden/painter_paint.npz).

The bar: equal as bytes, no tolerance, no case left out.  Every case of tests/painter_paint_cases.py runs; the instance masks arrive with
every padding bit and every slot past the masks set."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import painter_paint_cases as C
from tests import painter_paint_host as H
from tests.guard_bands import abi_symbols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import check
    from painter_amd.seggpt_engine import _stream
    from tests.test_guard_bands_engines_gpu import Ctx, run_case, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCE_NAMES = [name for name, _, _ in C.instance_cases()]
POSE_NAMES = [name for name, _, _, _ in C.pose_cases()]


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "painter_paint.npz")))


# ---- the host statement, computed once
@functools.lru_cache(maxsize=None)
def semantic_refs():
    return {name: H.semantic(m, H.ade_palette())[0] for name, m in C.semantic_cases()}


@functools.lru_cache(maxsize=None)
def panoptic_refs():
    return {name: H.panoptic_semantic(m, s, C.CATEGORY_INDEX, H.mean_sep_palette(133, 7)) for name, m, s in C.panoptic_cases()}


@functools.lru_cache(maxsize=None)
def instance_ref(name, method="mass_center"):
    masks = instance_masks(name)
    return H.instances(masks, method, C.geo_boxes(masks))


def instance_masks(name):
    return {n: m for n, m, _ in C.instance_cases()}[name]


@functools.lru_cache(maxsize=None)
def pose_ref(name):
    _, joints, visible, size = pose_case(name)
    res = [H.pose(j, v, size) for j, v in zip(joints, visible)]
    return np.stack([p for p, _ in res]), np.stack([w for _, w in res])


def pose_case(name):
    return {c[0]: c for c in C.pose_cases()}[name]


def check_reference(key, got):
    """The fixture's picture of the unmodified reference, where it saved one."""
    g = golden()
    if key in g and g[key].size:
        assert got.shape == g[key].shape and got.tobytes() == g[key].tobytes(), key
        return 1
    return 0


# ---- 1. the C ABI, every buffer at its exact size
def _semantic_table(c, jobs_in, palette):
    """One pa_paint_semantic over jobs_in = [(name, map, kind, table rows)] -> {name: picture}, bad."""
    pal = c.dev(palette, "palette")
    srcs = [c.dev(m, name) for name, m, _, _ in jobs_in]
    tables = [c.dev(np.array(t, np.int32).reshape(-1, 2), "table") if t else None for _, _, _, t in jobs_in]
    outs = [c.buf(m.shape[:2] + (3,), torch.uint8, 0x5A) for _, m, _, _ in jobs_in]
    jobs = (E.PaintJob * len(jobs_in))()
    for k, ((_, m, kind, t), s, tab, o) in enumerate(zip(jobs_in, srcs, tables, outs)):
        jobs[k] = E.PaintJob(s.data_ptr(), o.data_ptr(), None if tab is None else tab.data_ptr(), m.shape[0], m.shape[1], kind, len(t))
    jobs_d = c.dev(np.frombuffer(bytearray(jobs), np.uint8), "jobs")
    bad = c.buf((len(jobs_in),), torch.int32, 77)
    check(c.lib.pa_paint_semantic(jobs_d.data_ptr(), len(jobs_in), max(m.shape[0] * m.shape[1] for _, m, _, _ in jobs_in), pal.data_ptr(),
                                  len(palette), bad.data_ptr(), _stream()), "pa_paint_semantic")
    return {name: o for (name, _, _, _), o in zip(jobs_in, outs)}, bad


def semantic_direct(c):
    """The semantic cases -- 5 x 7, 37 x 53 and 512 x 683, uint8 and int32 -- in ONE job table; the panoptic cases -- int32 and RGB id maps,
    one without a segment -- in a second one with their own palette."""
    sem, bad = _semantic_table(c, [(name, m, E.PAINT_LABELS_U8 if m.dtype == np.uint8 else E.PAINT_LABELS_I32, []) for name, m in C.semantic_cases()],
                               H.ade_palette())
    pan, bad2 = _semantic_table(c, [(name, m, E.PAINT_IDS_RGB if m.ndim == 3 else E.PAINT_IDS_I32, [(s, C.CATEGORY_INDEX[cat]) for s, cat in seg])
                                    for name, m, seg in C.panoptic_cases()], H.mean_sep_palette(133, 7))
    return dict(bad=bad, bad2=bad2, semantic=sem, panoptic=pan)


def instances_direct(c, name, method="mass_center"):
    masks = instance_masks(name)
    n, h, w = masks.shape
    bits = c.dev(H.pack_bits(masks, poison=True, slots=n + 3).view(np.int32), "bits")
    pal = c.dev(E.location_palette().astype(np.uint8), "palette")
    cells_in = None if method == "mass_center" else c.dev(instance_ref(name, method)[1].reshape(-1, 2)[:max(n, 0)] if n else np.zeros((1, 2), np.int32), "cells")
    nbytes = c.lib.pa_paint_instances_workspace_bytes(n)
    ws = c.buf((nbytes,), torch.uint8)
    c.holds("pa_paint_instances's workspace", ws, nbytes)
    pic = c.buf((h, w, 3), torch.uint8, 0x5A)
    cells, empty = c.buf((max(n, 1), 2), torch.int32), c.buf((1,), torch.int32)
    check(c.lib.pa_paint_instances(bits.data_ptr(), n, h, w, pal.data_ptr(), None if cells_in is None else cells_in.data_ptr(), ws.data_ptr(),
                                   pic.data_ptr(), cells.data_ptr(), empty.data_ptr(), _stream()), "pa_paint_instances")
    return dict(picture=pic, cells=cells[:n], empty=empty)


def pose_direct(c, name):
    _, joints, visible, (W, H_) = pose_case(name)
    B, K = joints.shape[:2]
    rc, _ = E.msra_rectangles(joints, visible, (W, H_), 1.5)
    rk, _ = E.msra_rectangles(joints, visible, (W, H_), 3)
    table, _, centre = E.msra_table(3)
    rects = c.dev(np.stack([rc, rk], 1).astype(np.int32), "rects")
    colours, tab = c.dev(H.pose_colours()[:K], "colours"), c.dev(table, "table")
    out = c.buf((B, H_, W, 3), torch.uint8, 0x5A)
    check(c.lib.pa_paint_pose(rects.data_ptr(), B, K, H_, W, centre, colours.data_ptr(), tab.data_ptr(), len(table), out.data_ptr(), _stream()),
          "pa_paint_pose")
    return dict(pictures=out)


def test_semantic_and_panoptic_cases_in_one_job_table():
    got = semantic_direct(Ctx())
    assert not got["bad"].cpu().numpy().any() and not got["bad2"].cpu().numpy().any()
    seen = 0
    for kind, refs in (("semantic", semantic_refs()), ("panoptic", panoptic_refs())):
        for name, ref in refs.items():
            pic = got[kind][name].cpu().numpy()
            assert pic.shape == ref.shape and pic.tobytes() == ref.tobytes(), (kind, name)
            seen += check_reference("%s.%s" % (kind, name), pic)
    assert seen == 9                                                  # every picture the reference saved
    same_bytes("second run", got, semantic_direct(Ctx()))


@pytest.mark.parametrize("name", INSTANCE_NAMES)
def test_instance_case(name):
    got = instances_direct(Ctx(), name)
    pic, cells, empty = instance_ref(name)
    assert got["picture"].cpu().numpy().tobytes() == pic.tobytes(), name
    assert np.array_equal(got["cells"].cpu().numpy(), cells) and bool(got["empty"].item()) == empty
    check_reference("instances.mass_center." + name, got["picture"].cpu().numpy())
    assert ("instances.mass_center." + name in golden()) == (not name.startswith("overlap"))
    same_bytes("second run", got, instances_direct(Ctx(), name))


@pytest.mark.parametrize("name", [n for n in INSTANCE_NAMES if n.endswith("37x53")])
def test_instance_case_geo_center(name):
    got = instances_direct(Ctx(), name, "geo_center")
    pic, cells, empty = instance_ref(name, "geo_center")
    assert got["picture"].cpu().numpy().tobytes() == pic.tobytes() and np.array_equal(got["cells"].cpu().numpy(), cells)
    assert bool(got["empty"].item()) == empty
    check_reference("instances.geo_center." + name, got["picture"].cpu().numpy())


@pytest.mark.parametrize("name", POSE_NAMES)
def test_pose_case(name):
    got = pose_direct(Ctx(), name)["pictures"].cpu().numpy()
    ref, _ = pose_ref(name)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
    assert check_reference("pose." + name, got) == (1 if name.endswith("256x192") else 0)
    same_bytes("second run", got, pose_direct(Ctx(), name)["pictures"].cpu().numpy())


def test_refused_arguments():
    c = Ctx()
    a = c.buf((64,), torch.uint8, 0)
    p = a.data_ptr()
    bad = 1                                                           # hipErrorInvalidValue
    assert c.lib.pa_paint_semantic(None, 1, 35, p, 150, p, _stream()) == bad
    assert c.lib.pa_paint_semantic(p, 0, 35, p, 150, p, _stream()) == bad
    assert c.lib.pa_paint_semantic(p, 1, 35, p, 1025, p, _stream()) == bad
    assert c.lib.pa_paint_semantic(p, 1, 1 << 31, p, 150, p, _stream()) == bad
    assert c.lib.pa_paint_semantic(p + 4, 1, 35, p, 150, p, _stream()) == bad
    assert c.lib.pa_paint_instances_workspace_bytes(-1) == -1 and c.lib.pa_paint_instances_workspace_bytes(4097) == -1
    assert c.lib.pa_paint_instances_workspace_bytes(0) == 48 and c.lib.pa_paint_instances_workspace_bytes(100) == 2400 + 400
    assert c.lib.pa_paint_instances(p, 4097, 5, 7, p, None, p, p, p, p, _stream()) == bad
    assert c.lib.pa_paint_instances(p, 1, 0, 7, p, None, p, p, p, p, _stream()) == bad
    assert c.lib.pa_paint_instances(p, 1, 65536, 65536, p, None, p, p, p, p, _stream()) == bad
    assert c.lib.pa_paint_instances(p, 1, 5, 7, p, None, p, p + 4, p, p, _stream()) == bad
    assert c.lib.pa_paint_instances(p, 1, 5, 7, None, None, p, p, p, p, _stream()) == bad
    assert c.lib.pa_paint_pose(p, 1, 33, 5, 7, 9, p, p, 163, p, _stream()) == bad
    assert c.lib.pa_paint_pose(p, 0, 17, 5, 7, 9, p, p, 163, p, _stream()) == bad
    assert c.lib.pa_paint_pose(p, 1, 17, 5, 7, 9, p, p, 1025, p, _stream()) == bad
    assert c.lib.pa_paint_pose(p, 1, 17, 5, 7, 9, p, p, 163, None, _stream()) == bad
    torch.cuda.synchronize()
    assert not a.cpu().numpy().any()                                  # nothing was launched


# ---- 2. through painter_engine
def engine_semantic(c=None):
    c = c or Ctx()
    names = [name for name, _ in C.semantic_cases()]
    maps = [m for _, m in C.semantic_cases()]
    outs = E.paint_semantic([c.dev(m) if k % 2 else m for k, m in enumerate(maps)])          # numpy and device maps in one call
    for name, o in zip(names, outs):
        assert o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and o.cpu().numpy().tobytes() == semantic_refs()[name].tobytes(), name
    one = E.paint_semantic(maps[0])
    assert torch.equal(one, outs[0])
    pnames = [name for name, _, _ in C.panoptic_cases()]
    pouts = E.paint_panoptic_semantic([c.dev(m) if k % 2 else m for k, (_, m, _) in enumerate(C.panoptic_cases())],
                                      [[dict(id=s, category_id=cat) for s, cat in seg] if k % 2 else seg for k, (_, _, seg) in enumerate(C.panoptic_cases())],
                                      C.CATEGORY_INDEX)
    for name, o in zip(pnames, pouts):
        assert o.cpu().numpy().tobytes() == panoptic_refs()[name].tobytes(), name
    return dict(semantic=outs, panoptic=pouts)


def test_paint_semantic_and_paint_panoptic_semantic():
    engine_semantic()
    with pytest.raises(ValueError, match=r"picture 1 has 2 pixel\(s\) with a label above the palette's 150 colours; 1 of 2"):
        E.paint_semantic(C.semantic_bad_case())
    with pytest.raises(ValueError, match="picture 0"):               # the same labels over a palette of 100 colours
        E.paint_semantic(C.semantic_cases()[0][1], palette=H.ade_palette()[:100])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.paint_semantic(torch.zeros((5, 7), dtype=torch.uint8))


def engine_instances(c=None):
    c = c or Ctx()
    r = {}
    for name in ("n11_37x53", "n100_5x7", "overlap_37x53", "n0_64x33", "allblack_37x53"):
        masks = instance_masks(name)
        n, h, w = masks.shape
        pic, cells, empty = instance_ref(name)
        routes = [("bool", masks, None), ("u8 tensor", c.dev(masks.view(np.uint8)), None)]
        if n:                                                         # (bit masks cannot say "no mask": their first dimension is at least 1)
            routes.append(("bits", c.dev(H.pack_bits(masks, poison=True).view(np.int32)), (h, w)))
        for tag, arg, size in routes:
            got = E.paint_instances(arg, size=size)
            assert got[0].is_cuda and got[0].cpu().numpy().tobytes() == pic.tobytes(), (name, tag)
            assert np.array_equal(got[1], cells) and got[1].dtype == np.int32 and got[2] is empty, (name, tag)
        r[name] = got[0]
        if name.endswith("37x53"):
            geo = E.paint_instances(masks, method="geo_center", boxes=C.geo_boxes(masks))
            want = instance_ref(name, "geo_center")
            assert geo[0].cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(geo[1], want[1]) and geo[2] is want[2], name
            r[name + " geo"] = geo[0]
    masks = instance_masks("n11_37x53")
    rles = E.rle_encode(masks)[0]
    assert torch.equal(E.paint_instances(rles)[0], r["n11_37x53"])
    return r


def test_paint_instances():
    engine_instances()


def engine_pose(c=None):
    r = {}
    for name in POSE_NAMES:
        _, joints, visible, size = pose_case(name)
        pics, weights = E.paint_pose(joints, visible, heatmap_size=size)
        ref, w = pose_ref(name)
        assert pics.is_cuda and pics.dtype == torch.uint8 and tuple(pics.shape) == ref.shape and pics.cpu().numpy().tobytes() == ref.tobytes(), name
        assert weights.dtype == np.float32 and np.array_equal(weights, w[:, 1])
        r[name] = pics
    _, joints, visible, size = pose_case("b5_64x48")
    odd = E.paint_pose(joints[:, :5, :2] * 0.7, visible[:, :5, 0], heatmap_size=(37, 53), image_size=(74, 106))[0]       # 37 * 53 * 3 bytes per box: no multiple of 4
    want = np.stack([H.pose(j, v, (37, 53), image_size=(74, 106))[0] for j, v in zip(joints[:, :5, :2] * 0.7, visible[:, :5, :1])])
    assert odd.cpu().numpy().tobytes() == want.tobytes() and want.any()
    r["odd"] = odd
    return r


def test_paint_pose():
    engine_pose()


# ---- 3. round trips on the device
def test_round_trip_semantic():
    for name, labels in C.semantic_cases()[:2]:
        got = E.class_map(E.paint_semantic(labels), H.ade_palette())
        assert np.array_equal(got[labels > 0], labels[labels > 0].astype(np.int64) - 1) and (labels > 0).any(), name


def test_round_trip_instances():
    from tests.test_painter_paint_cpu import round_trip_rows
    masks = C.roundtrip_masks()
    rows = round_trip_rows(masks)
    pic, cells, empty = E.paint_instances(masks)
    out = E.instances(pic, dist_thr=4.0)                              # neighbouring cells' colours are 13 apart: 13 / 3 > 4
    assert not empty and len(out["masks"]) == len(masks) and sorted(out["candidates"].tolist()) == sorted(rows)
    for cand, got in zip(out["candidates"], out["masks"]):
        assert np.array_equal(got, masks[rows.index(int(cand))])


@pytest.mark.parametrize("size", C.POSE_SIZES)
def test_round_trip_pose(size):
    from tests.test_painter_paint_cpu import pose_round_trip_set
    joints, visible = C.pose_boxes(*size)
    pics, _ = E.paint_pose(joints, visible, heatmap_size=size)
    kp = E.keypoints(pics)
    chosen = pose_round_trip_set(pose_ref("b5_%dx%d" % (size[1], size[0]))[0], joints, visible, size)
    assert len(chosen) >= 8
    for b, k, mx, my in chosen:
        assert kp["preds"][b, k].tolist() == [mx, my] and kp["maxvals"][b, k] == 1, (b, k)


# ---- 4. where the pictures go
def test_painter_engine_takes_a_device_prompt_target():
    from tests import painter_eval_cases as PC
    img, _ = PC.prompt_pair()
    tgt = E.paint_instances(C.roundtrip_masks())[0]
    a = E.PainterEngine(PC.StandInModel(), "cuda", "coco_pano_inst", img, tgt, input_size=PC.RES, batch_size=2)
    b = E.PainterEngine(PC.StandInModel(), "cuda", "coco_pano_inst", torch.from_numpy(img).cuda(), tgt.cpu().numpy(), input_size=PC.RES, batch_size=2)
    assert torch.equal(a.prompt_tgt, b.prompt_tgt) and torch.equal(a.prompt, b.prompt) and a.prompt_tgt.any()
    queries = torch.from_numpy(np.stack([PC.picture(5, PC.RES, PC.RES), PC.picture(6, PC.RES, PC.RES)])).cuda()
    for x, y in zip(a.stitch(queries), b.stitch(queries)):
        assert torch.equal(x, y)
    with pytest.raises(AssertionError):
        E.PainterEngine(PC.StandInModel(), "cuda", "coco_pano_inst", img, tgt.to(torch.int32), input_size=PC.RES)


def pair_device_route(c=None):
    """PairSpec.image / .target as device tensors: the crop jobs read the tensors in place (`src`, `src_row_bytes`)."""
    from painter_amd import pair_pipeline as PP
    from tests.seggpt_io_cases import picture
    c = c or Ctx()
    pipe = PP.DevicePairPipeline("cuda", input_size=(64, 32))
    img = picture(97, 37, 53)
    tgt = H.instances(instance_masks("n11_37x53"))[0]
    boxes = [(1, 0, 36, 53), (2, 3, 7, 50), (0, 0, 37, 53), (36, 52, 1, 1), (5, 7, 32, 32), (3, 1, 32, 20)]
    jobs = [(box, near) for box in boxes for near in (False, True)]
    r = {}
    for tag, pics in (("numpy", [img, tgt]), ("device", [c.dev(img, "image"), c.dev(tgt, "target")])):
        out = c.buf((2 * len(jobs), 32, 32, 3), torch.uint8, 0)
        pipe.resized_crop_batch([pics[k % 2] for k in range(2 * len(jobs))], [b for b, _ in jobs] * 2, [n for _, n in jobs] * 2, out)
        r[tag] = out
    assert torch.equal(r["numpy"], r["device"]) and r["numpy"].any()
    mixed = c.buf((4, 32, 32, 3), torch.uint8, 0)
    pipe.resized_crop_batch([img, c.dev(tgt), c.dev(img), tgt], [boxes[1]] * 4, [False, True, False, True], mixed)
    plain = c.buf((4, 32, 32, 3), torch.uint8, 0)
    pipe.resized_crop_batch([img, tgt, img, tgt], [boxes[1]] * 4, [False, True, False, True], plain)
    assert torch.equal(mixed, plain)
    samples = lambda a, b: [PP.SampleSpec([PP.PairSpec(a, b, boxes[k], flip=bool(k)), PP.PairSpec(a, b, boxes[k + 1])], "coco_image2panoptic_inst")
                            for k in range(2)]
    host_batch = pipe.build_batch(samples(img, tgt))
    dev_batch = pipe.build_batch(samples(c.dev(img), c.dev(tgt)))
    for x, y in zip(host_batch, dev_batch):
        assert torch.equal(x, y)
    r["mixed"], r["batch"] = mixed, list(dev_batch)
    return r


def test_pair_spec_device_tensors_equal_the_numpy_route():
    pair_device_route()


# ---- 5. guard bands: exact-size buffers between 4 MiB of 0xFF, results byte-identical to the ordinary run
def _guard_instances(c):
    return {name: instances_direct(c, name) for name in ("n100_37x53", "n11_5x7", "n0_64x33", "n11_64x33", "overlap_37x53")}


def _guard_instances_geo(c):
    return instances_direct(c, "n11_37x53", "geo_center")


def _guard_pose(c):
    return {name: pose_direct(c, name) for name in ("b5_64x48", "b1_256x192")}


GUARD_CASES = [
    ("semantic-one-job-table", semantic_direct, [], ("pa_paint_semantic",)),
    ("instances-exact-buffers-poisoned-bits", _guard_instances, [], ("pa_paint_instances", "pa_paint_instances_workspace_bytes")),
    ("instances-geo-center", _guard_instances_geo, [], ("pa_paint_instances", "pa_paint_instances_workspace_bytes")),
    ("pose", _guard_pose, [], ("pa_paint_pose",)),
    ("engine-paint_semantic", engine_semantic, ["painter_engine"], ("pa_paint_semantic",)),
    ("engine-paint_instances", engine_instances, ["painter_engine"], ("pa_paint_instances", "pa_paint_instances_workspace_bytes", "pa_pack_mask_bits")),
    ("engine-paint_pose", engine_pose, ["painter_engine"], ("pa_paint_pose",)),
    ("pair-device-tensors", pair_device_route, ["pair_pipeline"], ("pa_resized_crop_u8_batch",)),
]


@pytest.mark.parametrize("fn,modules,symbols", [pytest.param(f, m, s, id=i) for i, f, m, s in GUARD_CASES])
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, tuple(modules), tuple(symbols), monkeypatch)


def test_every_symbol_of_the_paint_header_is_guarded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_paint.h")).read())
    assert abi == {"pa_paint_semantic", "pa_paint_instances_workspace_bytes", "pa_paint_instances", "pa_paint_pose"}
    claimed = set()
    for _, _, _, symbols in GUARD_CASES:
        claimed |= {s for s in symbols if s.startswith("pa_paint_")}
    helpers = {s for s in abi if s.endswith("_workspace_bytes")}      # host only: their cases allocate exactly what they return
    assert abi - claimed == set() and helpers <= claimed
