"""Generate tests/golden/painter_inst.npz by running the UNMODIFIED reference code on CPU:
`COCOEvaluatorCustom.post_process_segm_output_by_threshold` of Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py (which calls
util/matrix_nms.mask_matrix_nms) and that module's `define_colors_per_location_r_gb`, over the synthetic painted pictures of
tests/painter_inst_cases.py saved as PNG files.

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_inst.py [--search]

The module guards its main body, so importing it defines its functions and classes and nothing else.  detectron2, pycocotools, tqdm and
matplotlib are absent here and are empty stand-in modules with the handful of names the import statements ask for; `Instances` and
`Boxes` are attribute bags.  The evaluator's constructor needs CUDA and detectron2's dataset catalogue, so the object is made with
`object.__new__` and given the three attributes the method reads (palette on the CPU, topk, dist_thr_list).

The reference's result is defined only up to float32 rounding and an unspecified sort among tied masknesses (the tests' host statement,
tests/painter_inst_host.py, defines them).  A case enters the fixture only after this script has ASSERTED, here, that
  * the reference's kept masks equal the host statement's, in the same order,
  * the maskness gap at the nms_pre cut is >= 1e-6 relative, and the score gap at the max_num cut is >= 1e-6,
so that the fixture pins the device path to the reference exactly where the reference is well defined.  Stored: the palette, per case
the picture, the thresholds, the reference's scores (float32) and bit-packed masks, the candidate counts, and the reference's own
largest score deviation from the host statement.  `--search` tries further seeds for every slot and prints which qualify."""
import os
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import                                            # noqa: E402
from tests import painter_inst_cases as C                                # noqa: E402
from tests import painter_inst_host as H                                 # noqa: E402
from tests.golden.make_golden_painter_eval_io import _stub, save_npz     # noqa: E402

NMS_PRE, MAX_NUM = 2000, 100              # the literals of COCOCAInstSegEvaluatorCustom.py:318 and :332
GAP = 1e-6


class _Bag:
    def __init__(self, *a, **k):
        self.args = a


def install_evaluator_stubs():
    ref_import.install_stubs()
    for name in ("matplotlib", "matplotlib.pyplot", "tqdm", "pycocotools", "pycocotools.mask", "detectron2.utils"):
        _stub(name)
    _stub("pycocotools.coco", COCO=None)
    _stub("pycocotools.cocoeval", COCOeval=None)
    _stub("detectron2.utils.file_io", PathManager=None)
    _stub("detectron2.structures", Boxes=_Bag, BoxMode=None, Instances=_Bag, BitMasks=None, pairwise_iou=None)
    _stub("detectron2.evaluation", COCOEvaluator=object)
    _stub("detectron2.evaluation.coco_evaluation", instances_to_coco_json=None)


def load_evaluator_module():
    install_evaluator_stubs()
    path = os.path.join(ref_import.PAINTER_DIR, "eval", "coco_panoptic", "COCOCAInstSegEvaluatorCustom.py")
    saved = list(sys.path)
    try:
        return ref_import._load("ref_coco_ca_inst_evaluator", path, ref_import.PAINTER_DIR)
    finally:
        sys.path[:] = saved                            # the module inserts './' into sys.path


def load_palette():
    """-> float32 [6400][3]: define_colors_per_location_r_gb() in its own order, without the background row the evaluator appends."""
    d = load_evaluator_module().define_colors_per_location_r_gb()
    return np.array([v for _, v in d.items()], dtype=np.float32)


def run_reference(picture, thresholds, tmp):
    """-> (scores float32 [n], masks bool [n][H][W]) of the unmodified method for the picture saved as a PNG file."""
    import torch
    mod = load_evaluator_module()
    ev = object.__new__(mod.COCOEvaluatorCustom)
    ev.palette = torch.tensor([tuple(c) for c in load_palette().tolist()] + [(0, 0, 0)], dtype=torch.float)
    ev.topk, ev.dist_thr_list = MAX_NUM, list(thresholds)
    path = os.path.join(tmp, "picture.png")
    Image.fromarray(picture).save(path)
    with torch.no_grad():
        inst = ev.post_process_segm_output_by_threshold(path, dist_thr_list=list(thresholds))["instances"]
    return inst.scores.numpy().astype(np.float32), inst.pred_masks.numpy() > 0


def examine(picture, thresholds, tmp):
    """-> (dict of what the fixture stores, list of reasons the case does not qualify)."""
    pal = load_palette()
    ref_scores, ref_masks = run_reference(picture, thresholds, tmp)
    host = H.decode(picture, pal, thresholds, NMS_PRE, MAX_NUM)
    why = []
    if host["empty"]:
        return None, ["no candidate"]
    if ref_masks.shape != host["masks"].shape or not np.array_equal(ref_masks, host["masks"]):
        why.append("the reference's kept masks differ from the host statement's (set or order)")
    m, live = host["maskness"], host["live"]
    if live > NMS_PRE:
        n, s = host["n"], host["s"]
        rest = np.setdiff1d(np.flatnonzero(n > 0), host["survivors"])
        nxt = (s[rest] / (3.0 * n[rest])).min()
        if not nxt - m[-1] >= GAP * nxt:
            why.append("maskness gap at the nms_pre cut %.3e" % (nxt - m[-1]))
    full = H.matrix_nms(host["survivor_masks"], host["survivor_scores"], inter=host["inter"], max_num=len(m))[0]
    if len(full) > MAX_NUM and not full[MAX_NUM - 1] - full[MAX_NUM] >= GAP:
        why.append("score gap at the max_num cut %.3e" % (full[MAX_NUM - 1] - full[MAX_NUM]))
    dev = float(np.abs(ref_scores.astype(np.float64) - host["scores"]).max()) if ref_scores.shape == host["scores"].shape else float("nan")
    return dict(picture=picture, thresholds=np.array(thresholds, np.float32), scores=ref_scores,
                masks=H.pack_bits(ref_masks.reshape(len(ref_masks), -1)), live=np.int64(live), deviation=np.float64(dev)), why


def main():
    out = {"palette": load_palette()}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        if "--search" in sys.argv:
            for name, (seed, h, w, thr, kw) in C.FIXTURE.items():
                for s in range(seed, seed + 100, 10):
                    rec, why = examine(C.painted_picture(s, h, w, **kw), thr, tmp)
                    print(name, "seed", s, "live", None if rec is None else int(rec["live"]), "deviation",
                          None if rec is None else float(rec["deviation"]), "OK" if not why else why, flush=True)
            return
        for name, (seed, h, w, thr, _) in C.FIXTURE.items():
            rec, why = examine(C.fixture_picture(name), thr, tmp)
            assert not why, (name, why)
            for k, v in rec.items():
                out["%s.%s" % (name, k)] = v
            worst = max(worst, float(rec["deviation"]))
            print(name, "%dx%d" % (h, w), thr, "live", int(rec["live"]), "kept", len(rec["scores"]), "deviation %.3e" % rec["deviation"])
    lives = {n: int(out[n + ".live"]) for n in C.FIXTURE}
    assert lives["many"] > NMS_PRE and lives["few"] < NMS_PRE, lives
    assert sum(1 for n, c in C.FIXTURE.items() if c[3] == [19.0]) >= 3 and any(len(c[3]) == 2 for c in C.FIXTURE.values())
    out["deviation"] = np.float64(worst)
    path = os.path.join(HERE, "painter_inst.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes; largest reference deviation %.3e" % worst)
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
