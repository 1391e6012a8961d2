"""CPU side of the panoptic merge: tests/painter_pano_host.py (the definition the GPU tests hold the device to) is pinned against what
the unmodified evaluators produced (tests/golden/painter_pano.npz) and, where a reference checkout is present, against the live
reference; `semantic_palette` against the reference's colour rule; the C ABI against the header.

The bars: semantic map, classes, panoptic map, segment list and areas equal.  The host statement's own instance scores differ from the
reference's float32 ones in the last bits (bounded by tests/golden/painter_inst.npz's `deviation`); the merge decisions must not."""
import os

import numpy as np
import pytest
import torch

from tests import painter_pano_cases as C
from tests import painter_pano_host as H

_inst = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_pano.npz"))


@pytest.fixture(scope="module")
def score_bar(golden_dir):
    return 2 * float(np.load(os.path.join(golden_dir, "painter_inst.npz"))["deviation"])


def _segments(golden, name):
    """The fixture's segment list as the reference's dicts."""
    out = []
    for (sid, isthing, cat, inst, area), score in zip(golden[name + ".segments"].tolist(), golden[name + ".segment_scores"].tolist()):
        out.append(dict(id=sid, isthing=True, score=score, category_id=cat, instance_id=inst) if isthing else
                   dict(id=sid, isthing=False, category_id=cat, area=area))
    return out


def _host(golden, name):
    """The host statement of a fixture case from its two pictures (the instance decode shared between cases on the same pictures)."""
    from painter_amd.painter_engine import location_palette
    seed, h, w, thr, merge, _ = C.FIXTURE[name]
    key = (seed, h, w, tuple(thr))
    sem, inst = golden[name + ".semseg"], golden[name + ".inst"]
    out = H.decode(sem, inst, golden["palette"], location_palette(), thr, inst=_inst.get(key), overlap_threshold=merge[0],
                   stuff_area_thresh=merge[1], instances_score_thresh=merge[2])
    _inst[key] = out["instances"]
    return out


def test_fixture_holds_the_required_cases(golden):
    names = list(C.FIXTURE)
    assert [C.FIXTURE[n][1:5] for n in names] == [(96, 128, [19.0], (0.5, 256, 0.55)), (96, 128, [19.0], (0.5, 256, 0.2)),
                                                  (61, 83, [19.0], (0.1, 128, 0.2)), (72, 96, [10.0, 19.0], (0.1, 256, 0.0))]
    assert np.array_equal(golden["defaults.semseg"], golden["long_paste.semseg"]) and np.array_equal(golden["defaults.inst"], golden["long_paste.inst"])
    classes = set()
    for n in names:
        sem, inst = C.fixture_pair(n)
        assert np.array_equal(sem, golden[n + ".semseg"]) and np.array_equal(inst, golden[n + ".inst"])          # the generator is pinned
        assert sem.shape[:2] == C.FIXTURE[n][1:3] and tuple(golden[n + ".merge"]) == C.FIXTURE[n][4]
        assert [float(t) for t in golden[n + ".thresholds"]] == C.FIXTURE[n][3] and len(golden[n + ".scores"]) == 100
        table = golden[n + ".segments"]
        stuff = table[table[:, 1] == 0]
        present = set(np.unique(golden[n + ".semmap"]).tolist())
        assert len(stuff) >= 1 and len({l for l in present if l >= 80} - set(stuff[:, 2].tolist())) >= 1          # kept and dropped stuff
        classes |= set(golden[n + ".classes"].tolist())
    assert len(classes) >= 20 and max(classes) < 80
    assert 61 * 83 % 32 != 0


@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_host_statement_matches_the_unmodified_reference(golden, score_bar, name):
    host = _host(golden, name)
    ref = _segments(golden, name)
    assert np.array_equal(H.IH.pack_bits(host["masks"].reshape(100, -1)), golden[name + ".masks"])
    assert np.array_equal(host["semmap"], golden[name + ".semmap"]) and np.array_equal(host["classes"], golden[name + ".classes"])
    assert np.array_equal(host["panoptic"], golden[name + ".panoptic"])
    assert len(host["segments"]) == len(ref) and np.array_equal(host["areas"], golden[name + ".areas"])
    for s, r in zip(host["segments"], ref):
        assert set(s) == set(r) and all(s[k] == r[k] for k in r if k != "score"), (s, r)
        assert abs(s.get("score", 0.0) - r.get("score", 0.0)) <= score_bar
    for s, a in zip(host["segments"], host["areas"]):
        assert s["isthing"] or s["area"] == a
    print("%s: %d things, %d stuff, %d rejected for overlap, %d trimmed" % (name, sum(s["isthing"] for s in ref),
          sum(not s["isthing"] for s in ref), host["rejected"], host["trimmed"]))
    if name == "defaults":
        assert 0 < sum(s["isthing"] for s in ref) < 30
    if name in ("long_paste", "odd_size", "two_thr"):
        assert host["rejected"] >= 5 and host["trimmed"] >= 5


def test_host_statement_details():
    pal = np.array([[10, 10, 10], [10, 10, 20], [200, 0, 0], [100, 100, 100]], np.float32)
    pic = np.array([[[10, 10, 15], [10, 10, 16], [100, 100, 98], [190, 0, 0]]], np.uint8)
    assert H.semantic_map(pic, pal).tolist() == [[0, 1, 3, 2]]                          # 5 = 5: the first minimum
    assert H.distances(pic, pal, "square", 2).tolist() == [[25, 36, 8100 * 2 + 88 * 88, 180 * 180 + 200], [25, 16, 8100 * 2 + 78 * 78, 180 * 180 + 100 + 400]]
    assert np.array_equal(H.distances(pic, pal, "mean"), H.distances(pic, pal, "abs") + H.distances(pic, pal, "square"))
    masks = np.array([[[1, 0, 0, 0]], [[1, 1, 0, 0]], [[0, 0, 0, 0]]], bool)
    s, cl = H.vote(pic, pal, masks, n_things=2)
    assert s.tolist() == [[5, 5], [11, 9], [0, 0]] and cl.tolist() == [0, 1, 0]          # a tie and an empty mask: the lower class
    assert H.visiting_order([0.5, 0.9, 0.5, np.nan, 0.9]).tolist() == [1, 4, 0, 2, 3]
    # paste: instance 1 (score 0.9) first; instance 0 overlaps it by exactly 1 / 2 -- not > 0.5, so it is kept and trimmed; instance 2
    # is empty; instance 3 (score 0.1) ends the loop.  Stuff: label 2 keeps its one pixel, label 3's only pixel is taken.
    semmap = np.array([[0, 1, 3, 2]], np.int32)
    masks = np.array([[[1, 0, 1, 0]], [[1, 1, 0, 0]], [[0, 0, 0, 0]], [[0, 0, 0, 1]]], bool)
    out = H.merge(semmap, masks, [0.8, 0.9, 0.85, 0.1], [1, 0, 0, 1], n_things=2, n_colours=4, overlap_threshold=0.5, stuff_area_thresh=1,
                  instances_score_thresh=0.55)
    assert out["panoptic"].tolist() == [[1, 1, 2, 3]] and out["areas"].tolist() == [2, 1, 1] and (out["rejected"], out["trimmed"]) == (0, 1)
    assert out["segments"] == [dict(id=1, isthing=True, score=float(np.float32(0.9)), category_id=0, instance_id=1),
                               dict(id=2, isthing=True, score=float(np.float32(0.8)), category_id=1, instance_id=0),
                               dict(id=3, isthing=False, category_id=2, area=1)]
    out = H.merge(semmap, masks, [0.8, 0.9, 0.85, 0.1], [1, 0, 0, 1], n_things=2, n_colours=4, overlap_threshold=0.49, stuff_area_thresh=2,
                  instances_score_thresh=0.0)
    assert out["panoptic"].tolist() == [[1, 1, 0, 2]] and out["rejected"] == 1 and [s["instance_id"] for s in out["segments"]] == [1, 3]


def test_id2rgb_round_trips():
    from painter_amd.painter_engine import id2rgb
    ids = np.array([[0, 1, 255, 256], [257, 65535, 65536, 70000]], np.int32)
    rgb = id2rgb(ids)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 4, 3) and np.array_equal(H.rgb2id(rgb), ids)
    assert rgb[1, 3].tolist() == [70000 % 256, 70000 // 256 % 256, 1]


def test_semantic_palette_is_the_reference_colour_rule(golden):
    from painter_amd.painter_engine import semantic_palette
    pal = semantic_palette()
    assert pal.dtype == np.float32 and pal.shape == (C.K, 3) and np.array_equal(pal, golden["palette"]) and not pal.flags.writeable
    assert tuple(pal[0]) == (255, 255, 255) and tuple(pal[1]) == (255, 255, 219) and tuple(pal[7]) == (255, 219, 255)
    assert tuple(pal[49]) == (219, 255, 255) and semantic_palette(27, 3).shape == (27, 3) and tuple(semantic_palette(27, 3)[26]) == (85, 85, 85)
    if _reference():
        from tests.golden import make_golden_painter_pano as G
        assert np.array_equal(G.load_palette(), pal)


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_pano_workspace_bytes", "pa_pack_mask_bits", "pa_pano_vote", "pa_pano_merge", "pa_pano_decode"):
        assert name in protos
        assert getattr(lib, name) is not None
    assert len(protos["pa_pano_decode"][1]) == 22 and len(protos["pa_pano_merge"][1]) == 19
    for h, w, k, t, m in ((480, 640, 133, 80, 100), (61, 83, 133, 80, 100), (120, 160, 133, 133, 1), (4096, 4096, 1024, 2, 1024)):
        budget = m * t * 8 + h * w * (4 + 1 / 8) + 8 * k + 4 * m + 64          # vote sums, semantic map, union bits; two tables per colour, one per instance
        got = lib.pa_pano_workspace_bytes(h, w, k, t, m)                      # host only: no GPU needed
        assert budget <= got <= 2 * budget, (h, w, k, t, m, got, budget)
    for bad in ((0, 8, 133, 80, 100), (4097, 4096, 133, 80, 100), (8, 8, 1025, 80, 100), (8, 8, 133, 1, 100), (8, 8, 133, 134, 100),
                (8, 8, 133, 80, 0), (8, 8, 133, 80, 1025)):
        assert lib.pa_pano_workspace_bytes(*bad) == -1, bad
    assert lib.pa_abi_version() == 9


def test_panoptic_refuses_a_cpu_device():
    import torch
    from painter_amd import painter_engine as E
    pic = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.panoptic(pic, pic, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.panoptic(torch.zeros((4, 4, 3), dtype=torch.uint8), pic)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.classify_instances(pic, np.zeros((1, 4, 4), bool), device="cpu")
    # a mask tensor on the host must never reach a kernel as an address, whatever the picture's device: the device of the masks is
    # checked before anything is uploaded or launched (no GPU is needed to see the refusal)
    host_masks = torch.zeros((1, 4, 4), dtype=torch.bool)
    for device in ("cuda", "cuda:0"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E._bit_masks(host_masks, 4, 4, torch.device(device))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E._bit_masks(torch.zeros((1, 1), dtype=torch.int32), 4, 4, torch.device(device))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the picture is a numpy array bound for the GPU: the masks refuse
        E.classify_instances(pic, host_masks)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.panoptic(pic, instances=dict(masks=host_masks, scores=[0.5]))


def test_arguments_are_refused_before_anything_is_enqueued():
    """run_panoptic checks its keyword arguments before the first forward: engines that would fail on any use prove nothing ran."""
    import types
    from painter_amd import painter_engine as E

    def never(*a, **k):
        raise AssertionError("a forward was enqueued")
    sem = types.SimpleNamespace(task="coco_pano_semseg", _run=never, _launch_batch=never, batch_size=2, model=None)
    inst = types.SimpleNamespace(task="coco_pano_inst", _run=never, _launch_batch=never, batch_size=2, model=None)
    with pytest.raises(TypeError, match="nms_iou"):
        E.run_panoptic(sem, inst, [], nms_iou=0.5)
    with pytest.raises(NotImplementedError):
        E.run_panoptic(sem, inst, [], dist_type="cosine")
    with pytest.raises(NotImplementedError):
        E.run_panoptic(sem, inst, [], kernel="cubic")
    with pytest.raises(ValueError):
        E.run_panoptic(inst, inst, [])
    assert E._host_array(torch.tensor([0.25, 0.5]), np.float32).tolist() == [0.25, 0.5] and E._host_array([3, 4], np.int32).dtype == np.int32


def test_run_instances_and_run_pose_refuse_arguments_before_anything_is_enqueued():
    """The same stand-ins for the two other engine routes: an unknown keyword and an unsupported NMS kernel never reach a forward."""
    import types
    from painter_amd import painter_engine as E

    def never(*a, **k):
        raise AssertionError("a forward was enqueued")
    pictures = [np.zeros((4, 4, 3), np.uint8)]
    inst = types.SimpleNamespace(task="coco_pano_inst", _run=never, _launch_batch=never, batch_size=2, model=None)
    pose = types.SimpleNamespace(task="coco_pose", _run=never, _launch_batch=never, batch_size=2, model=None)
    with pytest.raises(TypeError, match="nms_iou"):
        E.PainterEngine.run_instances(inst, pictures, nms_iou=0.5)
    with pytest.raises(TypeError, match="dist_thr"):
        E.PainterEngine.run_pose(pose, pictures, None, dist_thr=3.0)
    with pytest.raises(NotImplementedError, match="cubic"):
        E.PainterEngine.run_instances(inst, pictures, kernel="cubic")


def test_out_bytes_is_the_closed_formula_and_signatures_repeat_the_default_tables():
    """The section list of PanopticDecode gives the byte count its buffer has always had.  The keyword defaults are written once, in the
    tables; every public signature that repeats one for its readers agrees with them."""
    import inspect
    from painter_amd import painter_engine as E
    for h, w, k, n_things, max_inst in ((480, 640, 133, 80, 100), (61, 83, 133, 80, 100), (4, 4, 2, 2, 1)):
        assert E.PanopticDecode.out_bytes(h, w, k, n_things, max_inst) == \
            16 + E.SEGMENT.itemsize * (max_inst + k - n_things) + 4 * max_inst + 7 * h * w
    assert E.SEGMENT.itemsize == 24

    def defaults(fn, rename={}):
        return {rename.get(k, k): v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    for fn, table, rename in ((E.instances, E.INSTANCE_DEFAULTS, {}), (E.panoptic, E.MERGE_DEFAULTS, {}),
                              (E.PanopticDecode.__init__, E.MERGE_DEFAULTS, {"palette": "semseg_palette"}),
                              (E.classify_instances, dict(E.MERGE_DEFAULTS), {"palette": "semseg_palette"}),
                              (E.keypoints, E.POSE_DEFAULTS, {}), (E.pose_heatmaps, E.POSE_DEFAULTS, {}), (E.PoseDecode.__init__, E.POSE_DEFAULTS, {})):
        have = defaults(fn, rename)
        shared = set(have) & set(table)
        assert shared and all(have[k] == table[k] for k in shared), (fn.__qualname__, have)
    assert set(E.INSTANCE_DEFAULTS) <= set(defaults(E.instances)) and set(E.MERGE_DEFAULTS) <= set(defaults(E.panoptic))
    assert set(E.POSE_DEFAULTS) <= set(defaults(E.keypoints))
    # the tables are passed on by position: their order is the constructors'
    assert list(inspect.signature(E.InstanceDecode.__init__).parameters)[2:8] == \
        ["palette", "thresholds", "nms_pre", "max_num", "kernel", "sigma"] and list(E.INSTANCE_DEFAULTS)[1] == "dist_thr"
    assert list(inspect.signature(E.PoseDecode.__init__).parameters)[3:6] == list(E.POSE_DEFAULTS)


# ---- with a reference checkout: the live reference
def _reference():
    from oracle import ref_import
    return os.path.isfile(os.path.join(ref_import.PAINTER_DIR, "eval", "coco_panoptic", "COCOPanoEvaluatorCustom.py"))


@pytest.mark.skipif(not _reference(), reason="needs the reference's Painter/eval/coco_panoptic evaluators")
def test_live_reference_matches_fixture_and_host_statement(golden, tmp_path):
    from tests.golden import make_golden_painter_pano as G
    name = "odd_size"
    rec, cover, why = G.examine(golden[name + ".semseg"], golden[name + ".inst"], C.FIXTURE[name][3], C.FIXTURE[name][4], str(tmp_path))
    assert not why, why
    for k in ("classes", "semmap", "panoptic", "segments", "segment_scores", "masks", "scores", "areas"):
        assert np.array_equal(rec[k], golden["%s.%s" % (name, k)]), k
