"""Generate tests/golden/painter_paint.npz by running the UNMODIFIED reference generators on the CPU over tests/painter_paint_cases.py:

  colorEncode, PALETTE                       Painter/data/ade20k/gen_color_ade20k_sem.py (imported; its main body is guarded)
  the paint loop, define_colors_by_mean_sep  data/coco_semseg/gen_color_coco_panoptic_segm.py.  The loop is the script's main body, so the
                                             script is RUN as __main__ in a temporary directory that holds the files it opens: the
                                             annotations JSON, the id PNGs and data/panoptic_coco_categories.json (this file's own
                                             133 categories), and the PNGs it saves are read back
  SaveDataPairCustom.__call__                data/mmdet_custom/data/pipelines/transforms.py, saving into a temporary directory
  encode_target_to_image                     data/mmpose_custom/data/pipelines/custom_transform.py, saving into a temporary directory

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_paint.py

Stand-in modules with the names the import statements ask for: cv2, mmcv, mmdet.datasets.builder.PIPELINES (a pass-through
`register_module`), tqdm (its `tqdm` returns its argument), skimage.segmentation.find_boundaries, matplotlib, and
panopticapi.utils whose `rgb2id` is this file's restatement of panopticapi's published one (r + 256 g + 65536 b).  mmpose is absent, and
`_msra_generate_target` is not in the reference tree: the heat maps handed to encode_target_to_image come from
tests/painter_paint_host.msra_target, restated from mmpose's published source and UNVERIFIED against mmpose.  The reference's pose
buffer is fixed at 17 x 256 x 192, so the 64 x 48 pose cases are pinned by the host statement alone; so are the instance cases with
overlapping masks, which the reference's assertion refuses.

Before writing, the script ASSERTS that the host statement equals the reference byte for byte on every case it can run; no case may be
dropped.  Stored: the reference's pictures (a case the reference does not save -- a pure black label, an annotation without segments --
stores an empty array), its palettes, and a digest of the inputs.  No reference program text."""
import json
import os
import runpy
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import                                            # noqa: E402
from tests import painter_paint_cases as C                               # noqa: E402
from tests import painter_paint_host as H                                # noqa: E402
from tests.golden.make_golden_painter_eval_io import _stub, save_npz     # noqa: E402

DATA_DIR = os.path.join(ref_import.PAINTER_DIR, "data")
NOT_SAVED = np.zeros((0, 0, 3), np.uint8)


def _rgb2id(color):
    """Stand-in for panopticapi.utils.rgb2id on an array."""
    color = color.astype(np.int32)
    return color[:, :, 0] + 256 * color[:, :, 1] + 256 * 256 * color[:, :, 2]


def install_stubs():
    ref_import.install_stubs()
    identity = lambda *a, **k: (lambda f: f)
    for name in ("cv2", "mmcv", "mmdet", "mmdet.datasets", "mmdet.datasets.builder", "tqdm", "skimage", "skimage.segmentation", "matplotlib",
                 "matplotlib.pyplot", "panopticapi", "panopticapi.utils"):
        _stub(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = type("Registry", (), {"register_module": staticmethod(identity)})
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    if not hasattr(sys.modules["skimage.segmentation"], "find_boundaries"):
        sys.modules["skimage.segmentation"].find_boundaries = None
    if not hasattr(sys.modules["panopticapi.utils"], "rgb2id"):
        sys.modules["panopticapi.utils"].rgb2id = _rgb2id
        sys.modules["panopticapi.utils"].IdGenerator = None


def _load(name, *path):
    install_stubs()
    full = os.path.join(DATA_DIR, *path)
    saved = list(sys.path)
    try:
        return ref_import._load(name, full, os.path.dirname(full))
    finally:
        sys.path[:] = saved


def run_semantic(out):
    mod = _load("ref_gen_color_ade20k_sem", "ade20k", "gen_color_ade20k_sem.py")
    pal = np.array(mod.PALETTE, np.uint8)
    assert np.array_equal(pal, H.ade_palette())
    out["semantic.palette"] = pal
    for name, labels in C.semantic_cases():
        ref = mod.colorEncode(labelmap=labels.copy(), colors=mod.PALETTE).astype(np.uint8)
        host, bad = H.semantic(labels, pal)
        assert bad == 0 and ref.shape == host.shape and ref.tobytes() == host.tobytes(), (name, "the host statement differs from the reference")
        out["semantic.%s" % name] = ref
        print("semantic", name, ref.shape)


def run_panoptic(out, tmp):
    install_stubs()
    cases = C.panoptic_cases()
    root = os.path.join(tmp, "pano")
    seg_dir = os.path.join(root, "datasets", "coco", "annotations", "panoptic_val2017")
    os.makedirs(seg_dir), os.makedirs(os.path.join(root, "data"))
    with open(os.path.join(root, "data", "panoptic_coco_categories.json"), "w") as f:
        json.dump([{"id": c, "name": "c%d" % c} for c in C.CATEGORY_IDS], f)
    anns = []
    for name, ids, segments in cases:
        png = ids if ids.ndim == 3 else C.id2rgb(ids)
        Image.fromarray(png).save(os.path.join(seg_dir, name + ".png"))
        anns.append({"file_name": name + ".png", "segments_info": [{"id": int(s), "category_id": int(c), "bbox": [0, 0, 1, 1]} for s, c in segments]})
    with open(os.path.join(root, "datasets", "coco", "annotations", "panoptic_val2017.json"), "w") as f:
        json.dump({"annotations": anns}, f)
    script = os.path.join(DATA_DIR, "coco_semseg", "gen_color_coco_panoptic_segm.py")
    cwd, argv, path = os.getcwd(), list(sys.argv), list(sys.path)
    os.chdir(root)
    sys.argv = [script, "--split", "val2017", "--output_dir", os.path.join(root, "out")]
    try:
        ns = runpy.run_path(script, run_name="__main__")
    finally:
        os.chdir(cwd)
        sys.argv[:], sys.path[:] = argv, path
    pal = np.array([ns["color_dict"][k] for k in range(len(C.CATEGORY_IDS))], np.uint8)
    assert np.array_equal(pal, H.mean_sep_palette(133, 7))
    out["panoptic.palette"] = pal
    for name, ids, segments in cases:
        saved = os.path.join(root, "out", "panoptic_segm_val2017_with_color", name + ".png")
        host = H.panoptic_semantic(ids, segments, C.CATEGORY_INDEX, pal)
        if not segments:
            assert not os.path.exists(saved) and not host.any()          # the script skips it; the host statement paints black
            out["panoptic.%s" % name] = NOT_SAVED
        else:
            ref = np.array(Image.open(saved))
            assert ref.shape == host.shape and ref.tobytes() == host.tobytes(), (name, "the host statement differs from the reference")
            out["panoptic.%s" % name] = ref
        print("panoptic", name, host.shape)


class _Masks:
    def __init__(self, masks):
        self.masks = masks


def run_instances(out, tmp):
    mod = _load("ref_mmdet_transforms", "mmdet_custom", "data", "pipelines", "transforms.py")
    for method in ("mass_center", "geo_center"):
        for name, masks, disjoint in C.instance_cases():
            if method == "geo_center" and not name.endswith("37x53"):
                continue
            boxes = C.geo_boxes(masks)
            host, cells, empty = H.instances(masks, method, boxes)
            key = "instances.%s.%s" % (method, name)
            if not disjoint:
                print("instances", method, name, "overlapping masks: host statement only")
                continue
            n, h, w = masks.shape
            target = os.path.join(tmp, "inst_%s_%s" % (method, name))
            saver = mod.SaveDataPairCustom(dir_name="d", target_path=target, method=method)
            results = dict(img=np.zeros((h, w, 3), np.uint8), gt_bboxes=boxes, gt_labels=np.zeros(n, np.int64),
                           gt_masks=_Masks(masks.astype(np.uint8)), img_info=dict(file_name="x.jpg"))
            saver(results)
            saved = os.path.join(target, "d", "x_label_d.png")
            if empty:
                assert not os.path.exists(saved), (name, "the reference saved a picture the host statement calls empty")
                out[key] = NOT_SAVED
            else:
                ref = np.array(Image.open(saved))
                assert ref.shape == host.shape and ref.tobytes() == host.tobytes(), (name, method, "the host statement differs from the reference")
                for m in range(n):
                    assert np.array_equal(saver.color_dict[tuple(int(c) for c in cells[m])], H.location_colour(*[int(c) for c in cells[m]]))
                out[key] = ref
            print("instances", method, name, masks.shape, "empty" if empty else "")


def run_pose(out, tmp):
    mod = _load("ref_pose_custom_transform", "mmpose_custom", "data", "pipelines", "custom_transform.py")
    colours = np.array([mod.color_dict[k] for k in range(17)], np.uint8)
    assert np.array_equal(colours, H.pose_colours())
    out["pose.colours"] = colours
    for sigma in (1.5, 3):
        table, f, c = H.d2_table(sigma)
        g, c2 = H.msra_patch(sigma)
        assert c == c2 and (np.diff(f) < 0).all()
        for y in range(g.shape[0]):
            for x in range(g.shape[1]):
                assert g[y, x] == f[(x - c) ** 2 + (y - c) ** 2]
    for name, joints, visible, (W, H_) in C.pose_cases():
        pics = []
        for b in range(len(joints)):
            host, weights = H.pose(joints[b], visible[b], (W, H_))
            dense, weights2 = H.pose_fast(joints[b], visible[b], (W, H_))
            assert host.tobytes() == dense.tobytes() and np.array_equal(weights, weights2), (name, b)
            if (W, H_) == (192, 256):
                tc, wc, _ = H.msra_target(joints[b], visible[b], (W, H_), 1.5)
                tk, wk, _ = H.msra_target(joints[b], visible[b], (W, H_), 3)
                target_dir = os.path.join(tmp, "pose_%s_%d" % (name, b))
                os.makedirs(target_dir)
                metas = dict(joints_3d_visible=visible[b], image_file="p.jpg", bbox_id=b, img=np.zeros((H_, W, 3), np.uint8))
                mod.encode_target_to_image(np.stack([tc, tk]), np.stack([wc, wk]), target_dir=target_dir, metas=metas)
                ref = np.array(Image.open(os.path.join(target_dir, "p_box%d_label.png" % b)))
                assert ref.shape == host.shape and ref.tobytes() == host.tobytes(), (name, b, "the host statement differs from the reference")
                pics.append(ref)
        if pics:
            out["pose.%s" % name] = np.stack(pics)
        print("pose", name, joints.shape, "reference" if pics else "host statement only")


def build():
    out = {"inputs.digest": np.array(C.input_digest())}
    with tempfile.TemporaryDirectory() as tmp:
        run_semantic(out)
        run_panoptic(out, tmp)
        run_instances(out, tmp)
        run_pose(out, tmp)
    return out


def main():
    out = build()
    path = os.path.join(HERE, "painter_paint.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
