"""Generate tests/golden/painter_score.npz by running the UNMODIFIED reference code on CPU over the cases of tests/painter_score_cases.py:
  * `SemSegEvaluatorCustom.process` of Painter/eval/ade20k_semantic/ADE20kSemSegEvaluatorCustom.py (:75-112) and of
    eval/coco_panoptic/COCOPanoSemSegEvaluatorCustom.py (:67-106), over PNG files of the painted pictures and their label maps,
  * `eval` and `compute_errors` of Painter/eval/nyuv2_depth/eval_with_pngs.py (:148-217, :50-71).

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_score.py

The evaluator modules guard their main bodies; detectron2, tqdm and the other absent packages are the stand-in modules of
tests/golden/make_golden_painter_pano.load_modules, `tqdm.tqdm` an identity.  The evaluators' constructors need CUDA and detectron2's
catalogue, so the objects are made with `object.__new__` and given what `process` reads: the palette (CPU), dist_type, _num_classes,
_ignore_label, a zero _conf_matrix, _compute_boundary_iou = False, a PIL `sem_seg_loading_fn`, the file mapping and a no-op
`encode_json_sem_seg`.  eval_with_pngs.py parses its command line on import and reads the PNG files with cv2, which is absent: it is
loaded with `sys.argv` set and a stand-in cv2, its globals `gt_depths` / `missing_ids` are set as its `test()` would (the two
`astype(np.float32) / 1000.0` lines, :100 and :136), and its `eval()` is called.

Stored: per semantic case and dist_type the reference's matrix as (non-zero bin index, count) pairs; per depth case the nine float32
numbers of `eval`, the host statement's ten sums and, for the six numbers that the reference sums in float32, the relative deviation
|statement - reference| / |reference| as `depth.<case>.ref_dev`.  No pictures: the cases are seeded.  A case enters the fixture only
after this script has ASSERTED that the host statement's matrix (tests/painter_score_host.py) equals the reference's exactly and that the
statement's n and counts reproduce the reference's d1 .. d3 after rounding to float32; over the set: >= 20 non-zero off-diagonal bins, a
non-empty ignore column, and a depth case whose predictions are clamped at both ends."""
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import                                                    # noqa: E402
from tests import painter_score_cases as C                                       # noqa: E402
from tests import painter_score_host as H                                        # noqa: E402
from tests.golden import make_golden_painter_pano as GP                          # noqa: E402
from tests.golden.make_golden_painter_eval_io import save_npz                    # noqa: E402

DEPTH_DIR = os.path.join(ref_import.PAINTER_DIR, "eval", "nyuv2_depth")


def load_evaluators():
    """-> {"ade": module of ADE20kSemSegEvaluatorCustom.py, "coco": module of COCOPanoSemSegEvaluatorCustom.py}."""
    coco = GP.load_modules()[0]
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    ade = GP._load("ref_ade20k_semseg_evaluator", os.path.join(ref_import.PAINTER_DIR, "eval", "ade20k_semantic", "ADE20kSemSegEvaluatorCustom.py"))
    return {"ade": ade, "coco": coco}


def _load_png(path, dtype):
    return np.array(Image.open(path)).astype(dtype)


def run_semseg(which, picture, gt, palette, dist_type, tmp):
    """-> int64 [K + 1][K + 1]: what the unmodified `process` added to a zero _conf_matrix for the pair saved as PNG files."""
    import torch
    mod = load_evaluators()[which]
    k = len(palette)
    ev = object.__new__(mod.SemSegEvaluatorCustom)
    ev.palette = torch.tensor([tuple(c) for c in np.asarray(palette).tolist()], dtype=torch.float)
    ev.dist_type, ev._num_classes, ev._ignore_label = dist_type, k, C.IGNORE
    ev._conf_matrix = np.zeros((k + 1, k + 1), dtype=np.int64)
    ev._compute_boundary_iou = False
    ev._predictions = []
    ev.sem_seg_loading_fn = lambda name, dtype: _load_png(name, dtype)
    ev.encode_json_sem_seg = lambda pred, name: []
    pic_path, gt_path = os.path.join(tmp, "picture.png"), os.path.join(tmp, "gt.png")
    Image.fromarray(picture).save(pic_path)
    Image.fromarray(gt).save(gt_path)
    ev.input_file_to_gt_file_custom = {pic_path: gt_path}
    with torch.no_grad():
        ev.process([{"file_name": pic_path}], [{"sem_seg": pic_path}])
    return ev._conf_matrix


def load_depth_eval(argv):
    """-> a fresh module object of eval_with_pngs.py whose `args` are parsed from argv."""
    saved_argv, saved_cv2 = sys.argv, sys.modules.get("cv2")
    sys.argv = ["eval_with_pngs.py", "--pred_path", "unused"] + list(argv)
    if saved_cv2 is None:
        sys.modules["cv2"] = types.ModuleType("cv2")
    name = "ref_eval_with_pngs_" + "_".join(a.strip("-") for a in argv)
    sys.modules.pop(name, None)
    try:
        return ref_import._load(name, os.path.join(DEPTH_DIR, "eval_with_pngs.py"), DEPTH_DIR)
    finally:
        sys.argv = saved_argv
        if saved_cv2 is None:
            del sys.modules["cv2"]


def run_depth(pred, gt, kw):
    """-> float32 [9]: silog, log10, abs_rel, sq_rel, rms, log_rms, d1, d2, d3 of the unmodified `eval` for one picture."""
    argv = []
    if "max_depth" in kw:
        argv += ["--max_depth_eval", repr(kw["max_depth"])]
    if kw.get("crop") == "eigen":
        argv += ["--eigen_crop"]
    mod = load_depth_eval(argv)
    mod.gt_depths = [gt.astype(np.float32) / 1000.0]                   # eval_with_pngs.py:136
    mod.missing_ids = set()
    out = mod.eval([pred.astype(np.float32) / 1000.0])                 # :100
    assert all(o.dtype == np.float32 and o.shape == (1,) for o in out)
    return np.array([o[0] for o in out], np.float32)


def main():
    out, off_diagonal, ignored, clamped = {}, 0, 0, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (which, seed, h, w, dist_types) in C.SEMSEG.items():
            pic, gt, pal = C.semseg_fixture_case(name)
            k = len(pal)
            for dist_type in dist_types:
                ref = run_semseg(which, pic, gt, pal, dist_type, tmp)
                host, invalid = H.confusion([pic], [gt], pal, dist_type, C.IGNORE)
                assert invalid == 0 and ref.dtype == np.int64 and np.array_equal(ref, host), (name, dist_type)
                assert ref.sum() == h * w
                idx = np.flatnonzero(ref.reshape(-1))
                out["semseg.%s.%s.bins" % (name, dist_type)] = idx.astype(np.int32)
                out["semseg.%s.%s.counts" % (name, dist_type)] = ref.reshape(-1)[idx]
                off = int(((idx // (k + 1)) != (idx % (k + 1))).sum())
                off_diagonal, ignored = off_diagonal + off, ignored + int(ref[:, k].sum())
                print(name, dist_type, "K", k, "bins", len(idx), "off-diagonal", off, "ignored pixels", int(ref[:, k].sum()))
    for name, (seed, h, w, kw) in C.DEPTH.items():
        pred, gt = C.depth_fixture_case(name)
        ref = run_depth(pred.copy(), gt.copy(), kw)
        sums, abs_log, clamp = H.depth_sums(pred, gt, **kw)
        host = H.depth_metrics(sums)
        n = sums[0]
        assert n > 0 and np.array_equal(np.float32(sums[1:4] / n), ref[6:9]), (name, sums[:4], ref[6:9])
        dev = np.abs(host[:6] - ref[:6].astype(np.float64)) / np.abs(ref[:6].astype(np.float64))
        out["depth.%s.reference" % name] = ref
        out["depth.%s.sums" % name] = sums
        out["depth.%s.ref_dev" % name] = dev
        clamped.append(clamp)
        print(name, "n", int(n), "clamped", clamp, "reference", ref, "ref_dev", dev)
    assert off_diagonal >= 20 and ignored > 0, (off_diagonal, ignored)
    assert any(c["low"] > 0 and c["high"] > 0 for c in clamped), clamped
    path = os.path.join(HERE, "painter_score.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
