"""Generate tests/golden/painter_pano.npz by running the UNMODIFIED reference code on CPU over the synthetic picture pairs of
tests/painter_pano_cases.py saved as PNG files:
  * `SemSegEvaluatorCustom.post_process_segm_output` (Painter/eval/coco_panoptic/COCOPanoSemSegEvaluatorCustom.py:108-136),
  * `COCOEvaluatorCustom.post_process_segm_output_by_threshold` (COCOCAInstSegEvaluatorCustom.py:252-354),
  * `COCOPanopticEvaluatorCustom.merge_inst_semseg_result_to_instseg` and `combine_semantic_and_instance_outputs_custom`
    (COCOPanoEvaluatorCustom.py:259-276, 47-134), and `define_colors_by_mean_sep` (data/coco_semseg/gen_color_coco_panoptic_segm.py).

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_pano.py [--search [case]]

The modules guard their main bodies.  detectron2, pycocotools, tabulate, panopticapi, skimage and tqdm are absent here and are stand-in
modules with the names the import statements ask for (tests/golden/make_golden_painter_inst.py); `data.register_coco_panoptic_annos_semseg`
registers datasets on import and is a stand-in too.  The evaluators' constructors need CUDA and detectron2's catalogue, so the objects are
made with `object.__new__` and given the attributes the methods read.

The reference votes in float32 and exact ties between classes do occur (seen on masks of 1 - 46 pixels), so equality with the host
statement (tests/painter_pano_host.py) is a condition on the chosen inputs, not a tolerance.  A case enters the fixture only after this
script has ASSERTED, here, that
  * the reference's kept masks equal the host statement's, in the same order (the rule of the instance fixture),
  * its semantic map and every instance class equal the host statement's,
  * its panoptic map and segment list equal the host statement's,
and over the set: a case with >= 5 instances rejected for overlap, a case with >= 5 trimmed, a kept and a dropped stuff label in every
case, >= 20 distinct classes voted.  `--search` tries further seeds for every slot (or the one named) and prints which qualify."""
import os
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import                                                    # noqa: E402
from tests import painter_inst_host as IH                                        # noqa: E402
from tests import painter_pano_cases as C                                        # noqa: E402
from tests import painter_pano_host as H                                         # noqa: E402
from tests.golden import make_golden_painter_inst as GI                          # noqa: E402
from tests.golden.make_golden_painter_eval_io import _stub, save_npz             # noqa: E402

N_THINGS = 80                          # the literal of COCOPanoEvaluatorCustom.py:116 and :270
COCO_DIR = os.path.join(ref_import.PAINTER_DIR, "eval", "coco_panoptic")


def _load(private_name, path):
    saved = list(sys.path)
    try:
        return ref_import._load(private_name, path, ref_import.PAINTER_DIR)
    finally:
        sys.path[:] = saved                            # the modules insert './' into sys.path


def load_modules():
    """-> (semantic evaluator module, panoptic evaluator module, colour module)."""
    GI.install_evaluator_stubs()
    for name in ("tabulate", "panopticapi", "skimage", "skimage.segmentation", "detectron2.data", "data",
                 "data.register_coco_panoptic_annos_semseg"):
        _stub(name)
    sys.modules["tabulate"].__dict__.setdefault("tabulate", None)
    sys.modules["detectron2.data"].__dict__.setdefault("MetadataCatalog", None)
    sys.modules["detectron2.utils"].__dict__.setdefault("comm", None)
    sys.modules["detectron2.evaluation"].__dict__.setdefault("SemSegEvaluator", object)
    sys.modules["detectron2.evaluation"].__dict__.setdefault("COCOPanopticEvaluator", object)
    sys.modules["skimage.segmentation"].__dict__.setdefault("find_boundaries", None)
    _stub("panopticapi.utils", rgb2id=None, IdGenerator=None, id2rgb=None)
    return (_load("ref_coco_pano_semseg_evaluator", os.path.join(COCO_DIR, "COCOPanoSemSegEvaluatorCustom.py")),
            _load("ref_coco_pano_evaluator", os.path.join(COCO_DIR, "COCOPanoEvaluatorCustom.py")),
            _load("ref_gen_color_coco_panoptic_segm", os.path.join(ref_import.PAINTER_DIR, "data", "coco_semseg", "gen_color_coco_panoptic_segm.py")))


def load_palette():
    """-> float32 [133][3]: define_colors_by_mean_sep() in its own order."""
    return np.array([v for _, v in load_modules()[2].define_colors_by_mean_sep().items()], dtype=np.float32)


def run_reference(sem_pic, inst_pic, thresholds, merge, tmp):
    """-> dict of what the unmodified methods produced for the pair saved as PNG files."""
    import torch
    sem_mod, pano_mod, _ = load_modules()
    inst_mod = GI.load_evaluator_module()
    ev_inst = object.__new__(inst_mod.COCOEvaluatorCustom)
    ev_inst.palette = torch.tensor([tuple(c) for c in GI.load_palette().tolist()] + [(0, 0, 0)], dtype=torch.float)
    ev_inst.topk, ev_inst.dist_thr_list = GI.MAX_NUM, list(thresholds)
    ev_sem = object.__new__(sem_mod.SemSegEvaluatorCustom)
    ev_sem.palette = torch.tensor([tuple(c) for c in load_palette().tolist()], dtype=torch.float)
    ev_sem.dist_type = "abs"
    ev_pano = object.__new__(pano_mod.COCOPanopticEvaluatorCustom)
    sem_path, inst_path = os.path.join(tmp, "sem.png"), os.path.join(tmp, "inst.png")
    Image.fromarray(sem_pic).save(sem_path)
    Image.fromarray(inst_pic).save(inst_path)
    with torch.no_grad():
        semseg_map, dist = ev_sem.post_process_segm_output(np.array(Image.open(sem_path)))
        inst = ev_inst.post_process_segm_output_by_threshold(inst_path, dist_thr_list=list(thresholds))["instances"]
        inst = ev_pano.merge_inst_semseg_result_to_instseg(semseg_map, dist, inst)
        pan, segments = pano_mod.combine_semantic_and_instance_outputs_custom(
            instance_results=inst, semantic_results=torch.from_numpy(semseg_map).to(inst.pred_classes.device),
            overlap_threshold=merge[0], stuff_area_thresh=merge[1], instances_score_thresh=merge[2])
    return dict(semmap=np.asarray(semseg_map), scores=inst.scores.numpy().astype(np.float32), masks=inst.pred_masks.numpy() > 0,
                classes=inst.pred_classes.numpy(), panoptic=pan.numpy(), segments=segments)


def same_segments(ref, host):
    """The reference's list against the host statement's: the same dicts, the score as the float the reference got from `.item()`."""
    return len(ref) == len(host) and all(set(r) == set(s) and all(r[k] == s[k] for k in r) for r, s in zip(ref, host))


def segment_table(segments):
    """-> int64 [n][5] (id, isthing, category_id, instance_id or -1, area or -1), float64 [n] scores (0 for stuff)."""
    t = np.array([[s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", -1)] for s in segments], np.int64)
    return t.reshape(-1, 5), np.array([s.get("score", 0.0) for s in segments], np.float64)


def examine(sem_pic, inst_pic, thresholds, merge, tmp):
    """-> (dict of what the fixture stores, coverage numbers, list of reasons the case does not qualify)."""
    ref = run_reference(sem_pic, inst_pic, thresholds, merge, tmp)
    kw = dict(overlap_threshold=merge[0], stuff_area_thresh=merge[1], instances_score_thresh=merge[2])
    inst = IH.decode(inst_pic, GI.load_palette(), thresholds, GI.NMS_PRE, GI.MAX_NUM)
    if inst["empty"]:
        return None, None, ["no candidate"]
    # the merge of the host statement runs on the REFERENCE's float32 scores: the host statement's own scores differ from them in the
    # last bits (tests/golden/make_golden_painter_inst.py), which the instance fixture bounds and this one must not depend on
    why = []
    if ref["masks"].shape != inst["masks"].shape or not np.array_equal(ref["masks"], inst["masks"]):
        return None, None, ["the reference's kept masks differ from the host statement's (set or order)"]
    host = H.panoptic(sem_pic, load_palette(), inst["masks"], ref["scores"], None, N_THINGS, "abs", **kw)
    own = H.panoptic(sem_pic, load_palette(), inst["masks"], inst["scores"].astype(np.float32), host["classes"], N_THINGS, "abs", **kw)
    if not np.array_equal(ref["semmap"], host["semmap"]):
        why.append("semantic maps differ")
    if not np.array_equal(ref["classes"], host["classes"]):
        why.append("%d instance classes differ (float32 vote)" % int((ref["classes"] != host["classes"]).sum()))
    if not np.array_equal(ref["panoptic"], host["panoptic"]) or not same_segments(ref["segments"], host["segments"]):
        why.append("panoptic map or segment list differ")
    # ... and the host statement's own float32 scores must lead to the same decisions (they decide the same unless a score sits within
    # a float32 ulp of the threshold)
    if not np.array_equal(own["panoptic"], host["panoptic"]) or [s["id"] for s in own["segments"]] != [s["id"] for s in host["segments"]]:
        why.append("a score within rounding of instances_score_thresh")
    table, seg_scores = segment_table(ref["segments"])
    cover = dict(rejected=host["rejected"], trimmed=host["trimmed"], kept_stuff=len(host["kept_stuff"]),
                 dropped_stuff=len(host["dropped_stuff"]), classes=set(host["classes"].tolist()), instances=len(ref["scores"]),
                 things=int(table[:, 1].sum()))
    rec = dict(semseg=sem_pic, inst=inst_pic, thresholds=np.array(thresholds, np.float32), merge=np.array(merge, np.float64),
               scores=ref["scores"], masks=IH.pack_bits(ref["masks"].reshape(len(ref["masks"]), -1)),
               classes=ref["classes"].astype(np.int32), semmap=ref["semmap"].astype(np.uint8), panoptic=ref["panoptic"].astype(np.uint8),
               segments=table, segment_scores=seg_scores, areas=host["areas"])
    assert ref["panoptic"].max() < 256 and ref["semmap"].max() < 256
    return rec, cover, why


def main():
    out = {"palette": load_palette()}
    covers = {}
    with tempfile.TemporaryDirectory() as tmp:
        if "--search" in sys.argv:
            for name, (seed, h, w, thr, merge, kw) in C.FIXTURE.items():
                if sys.argv[-1] not in ("--search", name):
                    continue
                tries = [(s, kw.get("sem_seed", 0)) for s in range(seed, seed + 100, 10)] + [(seed, t) for t in range(1, 10)]
                for s, t in tries:                     # other instance pictures, then other semantic pictures for the slot's own
                    rec, cover, why = examine(*C.picture_pair(s, h, w, **dict(kw, sem_seed=t)), thr, merge, tmp)
                    print(name, "seed", s, "sem_seed", t,
                          None if cover is None else {k: (len(v) if isinstance(v, set) else v) for k, v in cover.items()},
                          "OK" if not why else why, flush=True)
            return
        for name, (seed, h, w, thr, merge, _) in C.FIXTURE.items():
            rec, cover, why = examine(*C.fixture_pair(name), thr, merge, tmp)
            assert not why, (name, why)
            for k, v in rec.items():
                out["%s.%s" % (name, k)] = v
            covers[name] = cover
            print(name, "%dx%d" % (h, w), thr, merge, {k: (len(v) if isinstance(v, set) else v) for k, v in cover.items()})
    assert max(c["rejected"] for c in covers.values()) >= 5 and max(c["trimmed"] for c in covers.values()) >= 5, covers
    assert all(c["kept_stuff"] >= 1 and c["dropped_stuff"] >= 1 for c in covers.values()), covers
    assert len(set().union(*(c["classes"] for c in covers.values()))) >= 20
    path = os.path.join(HERE, "painter_pano.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
