"""Generate tests/golden/painter_minmax.npz by running the UNMODIFIED reference code on CPU:
`COCOEvaluatorCustom.post_process_segm_output_by_minmax` of Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py (:172-250) and that
module's `define_colors_per_location_r_gb`, over the synthetic painted pictures of tests/painter_minmax_cases.py saved as PNG files.

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_minmax.py

The evaluator module is loaded as tests/golden/make_golden_painter_inst.py loads it (stand-in modules for detectron2 etc.); the object is
made with `object.__new__` and given the two attributes the method reads: `palette` (6400 colours + black, on the CPU) and
`num_windows = 4`, the constructor's default.

A case enters the fixture only after this script has ASSERTED, here, that
  * the reference equals the host statement (tests/painter_minmax_host.py) in every stored array -- pred_map, dist_map, the instance
    colours and their order, the classes, every mask -- and its float32 scores bit for bit,
  * its largest S_c is below 2^24: up to there the reference's float32 sums are exact integers whatever their order,
so the fixture pins the device path to the reference without a tolerance.  At least one stored case has a pixel with a tied minimum.
Stored per case: the picture, the reference's pred_map (uint16), dist_map (uint16), scores (float32), classes (int32), the number of pixels
with a tied minimum and the largest S_c; once: the palette without the background row."""
import os
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import painter_minmax_cases as C                                              # noqa: E402
from tests import painter_minmax_host as H                                               # noqa: E402
from tests.golden.make_golden_painter_eval_io import save_npz                            # noqa: E402
from tests.golden.make_golden_painter_inst import load_evaluator_module, load_palette   # noqa: E402

NUM_WINDOWS = 4                           # the default of COCOEvaluatorCustom.__init__ (:89)
S_LIMIT = 1 << 24


def run_reference(picture, palette, tmp):
    """-> (pred_map int64 [H][W], dist_map float32 [H][W], scores float32 [n], classes int64 [n], masks bool [n][H][W]) of the unmodified
    method for the picture saved as a PNG file."""
    import torch
    mod = load_evaluator_module()
    ev = object.__new__(mod.COCOEvaluatorCustom)
    ev.palette = torch.tensor([tuple(c) for c in palette.tolist()] + [(0, 0, 0)], dtype=torch.float)
    ev.num_windows = NUM_WINDOWS
    path = os.path.join(tmp, "picture.png")
    Image.fromarray(picture).save(path)
    with torch.no_grad():
        output, dist_map, pred_map = ev.post_process_segm_output_by_minmax(path)
    inst = output["instances"]
    assert inst.scores.dtype == torch.float32 and dist_map.dtype == torch.float32
    return pred_map.numpy(), dist_map.numpy(), inst.scores.numpy(), inst.pred_classes.numpy(), inst.pred_masks.numpy() > 0


def examine(picture, palette, tmp):
    """-> dict of what the fixture stores; asserts what the docstring promises."""
    pred_map, dist_map, scores, classes, masks = run_reference(picture, palette, tmp)
    host = H.decode(picture, H.with_background(palette))
    assert np.array_equal(pred_map, host["label"]) and np.array_equal(dist_map, host["dist"].astype(np.float32))
    assert (dist_map == np.floor(dist_map)).all()
    assert np.array_equal(np.unique(pred_map), host["candidates"]) and np.array_equal(classes, host["classes"])
    assert masks.shape == (host["count"],) + picture.shape[:2] and np.array_equal(masks, H.masks_of(host["label"], host["slot"]))
    assert scores.dtype == np.float32 and scores.tobytes() == host["scores"].tobytes(), "the scores differ in some bit"
    largest = int(host["S"].max())
    assert largest < S_LIMIT, largest
    return dict(picture=picture, pred_map=pred_map.astype(np.uint16), dist_map=dist_map.astype(np.uint16), scores=scores,
                classes=classes.astype(np.int32), ties=np.int64(host["ties"]), largest_sum=np.int64(largest))


def main():
    palette = load_palette()
    out = {"palette": palette}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (_, h, w, _) in C.FIXTURE.items():
            rec = examine(C.fixture_picture(name), palette, tmp)
            for k, v in rec.items():
                out["%s.%s" % (name, k)] = v
            print(name, "%dx%d" % (h, w), "instances", len(rec["scores"]), "tied pixels", int(rec["ties"]), "largest S", int(rec["largest_sum"]))
    assert any(int(out[n + ".ties"]) > 0 for n in C.FIXTURE), "no stored case has a pixel with a tied minimum"
    assert {"thr19_a", "thr19_c", "few"} <= set(C.FIXTURE)
    path = os.path.join(HERE, "painter_minmax.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
