"""Generate tests/golden/painter_pose.npz by running the UNMODIFIED reference code on CPU:
`TopDownCustom.forward_pseudo_test(..., return_heatmap=True)` of Painter/eval/mmpose_custom/model/top_down.py (:163-258) and
`define_colors_gb_mean_sep` (data/pipelines/custom_transform.py:10-33), over the pictures of tests/painter_pose_cases.py saved as PNG
files in a temporary directory and its `_flip` twin.

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_pose.py

mmcv and mmpose are absent here and are stand-in modules with the names the import statements ask for; cv2 is one already.  The class
body of TopDownCustom builds its colour table with `device="cuda"`: `torch.tensor` is wrapped for the duration of the import so that the
table lands on the CPU.  The stand-in base class `TopDown` carries `colors` (the method reads `TopDown.colors`), and the object is made
with `object.__new__` and given what the method reads: `test_cfg`, `with_keypoint`, and a `keypoint_head` with `target_type` and a `decode`
that returns {} -- the head's decode is mmpose's keypoints_from_heatmaps, which is absent, so the fixture pins the reference up to and
including `output_heatmap`, and tests/painter_pose_host.py is the definition of the peak rule.

`flip_back` is mmpose's and absent as well: this script supplies its own (`_flip_back` below: swap the channels of every pair, mirror the
last axis), restated from mmpose's published source for heat-map targets.

The arithmetic is exact and the tie rule is CPU torch's first minimum, so before writing the script ASSERTS that the host statement's heat
maps equal the reference's bit for bit on every case, with the flip test (shift on) and without; no case may be dropped.  Stored: the
palette, the pictures, the reference's heat maps (small cases: the whole float32 array; the 256 x 192 box: per channel the maximum, the
first argmax and the four neighbour values), and the host statement's preds / maxvals."""
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
from tests import painter_pose_cases as C                                # noqa: E402
from tests import painter_pose_host as H                                 # noqa: E402
from tests.golden.make_golden_painter_eval_io import _stub, save_npz     # noqa: E402

POSE_DIR = os.path.join(ref_import.PAINTER_DIR, "eval", "mmpose_custom")


def _flip_back(output_flipped, flip_pairs, target_type="GaussianHeatmap"):
    """Stand-in for mmpose.core.post_processing.flip_back on [n][K][H][W] heat maps: swap the channels of every pair, mirror the last axis."""
    assert output_flipped.ndim == 4 and target_type == "GaussianHeatmap"
    back = output_flipped.copy()
    for left, right in flip_pairs:
        back[:, left], back[:, right] = output_flipped[:, right], output_flipped[:, left]
    return back[..., ::-1]


class _TopDown:
    colors = None


def load_module():
    import torch
    if "ref_pose_top_down" in sys.modules:
        return sys.modules["ref_pose_top_down"]
    ref_import.install_stubs()
    identity = lambda *a, **k: (lambda f: f)
    for name in ("mmcv", "mmcv.image", "mmcv.utils", "mmcv.utils.misc", "mmcv.visualization", "mmcv.visualization.image", "mmcv.runner",
                 "mmpose", "mmpose.core", "mmpose.models", "mmpose.models.builder", "mmpose.models.detectors", "mmpose.core.post_processing"):
        _stub(name)
    sys.modules["mmcv.image"].imwrite = None
    sys.modules["mmcv.utils.misc"].deprecated_api_warning = identity
    sys.modules["mmcv.visualization.image"].imshow = None
    sys.modules["mmcv.runner"].auto_fp16 = identity
    sys.modules["mmpose.core"].imshow_bboxes = sys.modules["mmpose.core"].imshow_keypoints = None
    sys.modules["mmpose.models"].builder = sys.modules["mmpose.models.builder"]
    sys.modules["mmpose.models.builder"].POSENETS = type("Registry", (), {"register_module": staticmethod(identity)})
    sys.modules["mmpose.models.detectors"].TopDown = _TopDown
    sys.modules["mmpose.core.post_processing"].flip_back = _flip_back
    real, saved = torch.tensor, list(sys.path)
    torch.tensor = lambda *a, **k: real(*a, **dict(k, device="cpu"))
    try:
        mod = ref_import._load("ref_pose_top_down", os.path.join(POSE_DIR, "model", "top_down.py"), POSE_DIR)
    finally:
        torch.tensor = real
        sys.path[:] = saved
        for k in [k for k in sys.modules if k == "data" or k.startswith("data.")]:          # the reference's namespace package `data`
            sys.modules["_ref_pose." + k] = sys.modules.pop(k)
    _TopDown.colors = mod.TopDownCustom.colors
    return mod


def load_palette():
    """-> int32 [18][2]: the rows of TopDownCustom.colors (define_colors_gb_mean_sep() in its own order, then (0, 0))."""
    return load_module().TopDownCustom.colors.numpy().astype(np.int32)


class _Head:
    target_type = "GaussianHeatmap"

    def decode(self, img_metas, output, **kwargs):
        return {}


def run_reference(pictures, flipped, tmp, flip_test):
    """-> `output_heatmap` float32 [n][17][H][W] of the unmodified method for the pictures saved as PNG files."""
    import torch
    mod = load_module()
    net = object.__new__(mod.TopDownCustom)
    net.test_cfg = dict(flip_test=flip_test, shift_heatmap=True)
    net.with_keypoint, net.keypoint_head = True, _Head()
    plain, twin = os.path.join(tmp, "pose"), os.path.join(tmp, "pose_flip")
    os.makedirs(plain, exist_ok=True), os.makedirs(twin, exist_ok=True)
    metas, loaded = [], []
    for i, (p, q) in enumerate(zip(pictures, flipped)):
        name = "%04d.png" % i
        Image.fromarray(p).save(os.path.join(plain, name))
        Image.fromarray(q).save(os.path.join(twin, name))
        metas.append(dict(image_file=os.path.join(plain, name), bbox_id=i, flip_pairs=C.FLIP_PAIRS))
        loaded.append(torch.from_numpy(np.array(Image.open(os.path.join(plain, name)))))
    with torch.no_grad():
        res = net.forward_pseudo_test(torch.stack(loaded), metas, return_heatmap=True)
    out = np.asarray(res["output_heatmap"])
    assert out.dtype == np.float32, out.dtype
    return out


def summary(maps):
    """[n][K][H][W] -> (max float32 [n][K], first argmax int64 [n][K], neighbours float32 [n][K][4] = left, right, up, down; 0 outside)."""
    n, k, h, w = maps.shape
    flat = maps.reshape(n, k, -1)
    idx = flat.argmax(2)
    pad = np.pad(maps, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y, x = idx // w + 1, idx % w + 1
    b, c = np.mgrid[0:n, 0:k]
    nb = np.stack([pad[b, c, y, x - 1], pad[b, c, y, x + 1], pad[b, c, y - 1, x], pad[b, c, y + 1, x]], -1)
    return flat.max(2), idx, nb


def main():
    pal = load_palette()
    assert np.array_equal(pal, H.pose_palette()) and np.array_equal(pal, C.PALETTE)
    out = {"palette": pal}
    cases = {name: C.shape_pair(name) for name in C.FIXTURE}
    cases["hand"] = C.hand_boxes()[:2]
    cases["full"] = C.full_pair()
    with tempfile.TemporaryDirectory() as tmp:
        for name, (p, q) in cases.items():
            for mode, flip in (("flip", True), ("plain", False)):
                ref = run_reference(p, q, os.path.join(tmp, name + mode), flip)
                host = H.heatmaps(p, q if flip else None, pal, C.PAIR, shift=True)
                assert ref.shape == host.shape and ref.tobytes() == host.tobytes(), (name, mode, "the host statement differs from the reference")
                kp = H.peaks(host)
                if name == "full":
                    out["full.%s.max" % mode], out["full.%s.argmax" % mode], out["full.%s.neighbours" % mode] = summary(ref)
                else:
                    out["%s.%s.heatmaps" % (name, mode)] = ref
                out["%s.%s.preds" % (name, mode)], out["%s.%s.maxvals" % (name, mode)] = kp
                print(name, mode, ref.shape, "channels with a peak: %d of %d" % (int((kp[1] > 0).sum()), kp[1].size))
            out[name + ".pictures"], out[name + ".flipped"] = p, q
    path = os.path.join(HERE, "painter_pose.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
