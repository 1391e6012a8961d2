"""Painter task inference with the pre- and post-processing on the MI355X, batched.

The reference's eight task scripts (Painter/eval/*/painter_inference_*.py) run one picture at a time and do everything around the
forward on the host: `PIL.resize`, `/ 255.`, `np.concatenate`, `- mean`, `/ std` in float64 on two 896 x 448 x 3 canvases, three
4.8 MB uploads, and after the forward `unpatchify`, `.cpu()` of the whole canvas, de-normalise / clip in float64 and
`F.interpolate` (bilinear, nearest or bicubic) on the CPU to the picture's own size.  Here a picture crosses PCIe once in each
direction (uint8 in; uint8 / int32 / float64 at its own size out) and every array operation in between is a kernel of
csrc/painter_io.hip (resize: csrc/seggpt_io.hip):

    upload uint8 -> Pillow-exact resize -> stitch with the prompt pair -> ONE forward of up to `batch_size` pictures ->
    ONE decode launch over a job table (pictures of different sizes included) -> ONE copy back

The uint8 / int32 outputs are the bytes the scripts write (tests/test_painter_eval_gpu.py, against tests/painter_eval_host.py and
the digests the unmodified scripts produced); the float64 output of the three restoration tasks agrees with CPU torch's bicubic to
~1e-13 (torch's own operation order is not reproduced there).

`instances` / `PainterEngine.run_instances` decode a painted `coco_pano_inst` picture into class-agnostic instances on the device
(csrc/painter_inst.hip): the evaluator's threshold route and its Matrix NMS (COCOCAInstSegEvaluatorCustom.py:252-354,
util/matrix_nms.py) on exact integers and bit masks, ties defined (tests/painter_inst_host.py is the definition).
`instances_minmax` / `run_instances(..., post_type="minmax")` are the evaluator's other route (:172-250, csrc/painter_minmax.hip,
include/painter_minmax.h): every pixel goes to the nearest of the 6401 colours, every colour that wins a pixel is an instance, its score
comes from the mean distance of its pixels -- no NMS, no top-k (tests/painter_minmax_host.py is the definition).

`classify_instances`, `panoptic` and `run_panoptic` finish what COCO panoptic evaluation needs (csrc/painter_pano.hip): every instance
gets the thing class its pixels vote for in the painted `coco_pano_semseg` picture, and instances and semantic picture are combined into
a panoptic map with its segment list (COCOPanoEvaluatorCustom.py:47-134, 203-276; COCOInstSegEvaluatorCustom.py:169-194) -- chained
behind the instance decode on the device, one copy back (tests/painter_pano_host.py is the definition).

`keypoints`, `pose_heatmaps` and `PainterEngine.run_pose` turn painted `coco_pose` pictures into keypoints (csrc/painter_pose.hip):
TopDownCustom.forward_pseudo_test with its flip test (mmpose_custom/model/top_down.py:163-258) and mmpose's heat-map peak rule, straight
from the bytes of the two pictures -- no heat map in memory, 51 floats per box back (tests/painter_pose_host.py is the definition).

`SemsegScore`, `depth_errors`, `PainterEngine.run_semseg_score` and `run_depth_errors` score painted pictures against ground-truth maps
(csrc/painter_score.hip): the confusion matrix of SemSegEvaluatorCustom.process (ADE20kSemSegEvaluatorCustom.py:75-112,
COCOPanoSemSegEvaluatorCustom.py:67-106) accumulated on the device over a whole data set -- one launch per batch, nothing copied back
until `matrix()` -- and per picture the ten sums behind the nine numbers of nyuv2_depth/eval_with_pngs.py:50-71, 148-217
(tests/painter_score_host.py is the definition).  `SemsegBoundaryScore` adds the evaluators' boundary-IoU branch (:103-110 / :97-104,
detectron2's `_compute_boundary_iou`): both label maps eroded on the device by a separable window minimum and a second joint histogram
beside the first, from one evaluation of the classes; `label_boundary` is the erosion alone (tests/painter_boundary_host.py is the
definition; restated from detectron2's published source and unverified against detectron2 / cv2).

`restoration_scores`, `RestorationScores` and `PainterEngine.run_restoration_scores` score restored pictures (csrc/painter_restore.hip):
PSNR and SSIM as painter_inference_lol.py:166-169 asks them of skimage (metric "skimage") or as derain's evaluate_PSNR_SSIM.m computes
them from the saved PNGs (metric "matlab_y"), from the decode's device-resident float64 / saved uint8 output -- a float64 window stencil
over a job table, eight doubles per picture back (tests/painter_restore_host.py is the definition; both metrics are restated from
published sources and unverified against skimage / MATLAB).

`PanopticQuality` and `run_panoptic_quality` score panoptic maps against COCO panoptic annotations (csrc/painter_pq.hip): the joint
histogram of (ground-truth segment, predicted segment) per picture, the match at IoU > 0.5 and the false-negative / false-positive rules
of panopticapi's pq_compute_single_core, read from the panoptic decode's device-resident map, segment table and count -- four numbers
per category back for a whole data set (tests/painter_pq_host.py is the definition; restated from panopticapi's published source and
unverified against panopticapi).

`InstanceAP` and `run_instance_ap` score decoded instances against COCO instance annotations (csrc/painter_ap.hip): COCOeval's mask
IoUs and its greedy matching per (mode, area range, threshold) on bit masks, read from the instance decode's device-resident masks,
scores and count and the panoptic decode's classes -- 48 bytes per detection back; accumulate / summarize run on the host
(`instance_ap_metrics`; tests/painter_ap_host.py is the definition; restated from pycocotools' published source and unverified against
pycocotools).

`KeypointAP` and `PainterEngine.run_pose_ap` carry the keypoint decode to COCO keypoint AP (csrc/painter_kpt.hip): photo coordinates,
rescoring and OKS NMS of TopDownCocoDatasetCustom.evaluate (mmpose_custom/data/topdown_coco_dataset.py:194-315) and COCOeval's computeOks /
evaluateImg per photo, read from the pose decode's device-resident preds and maxvals -- 32 bytes per evaluated detection back; accumulate /
summarize run on the host (`keypoint_ap_metrics`; tests/painter_kpt_host.py is the definition; mmpose's oks_nms and xtcocotools' COCOeval
are restated from their published source and unverified against mmpose / xtcocotools).

`rle_encode`, `rle_decode`, `instance_results` and `run_instance_results` are COCO's run-length encoding on the device
(csrc/painter_rle.hip, include/painter_rle.h): bit masks -> the `{"size", "counts"}` strings, areas and boxes of pycocotools.mask.encode, and
strings or uncompressed counts -> bit masks.  The instance evaluators' whole output is coco_instances_results.json
(COCOCAInstSegEvaluatorCustom.py:119, :147-170): `instance_results` chains the encode behind the instance decode, so scores and strings come
back instead of the bool masks, and every `masks=` argument also takes a list of RLE dicts (a detections JSON, crowd ground truth)
(tests/painter_rle_host.py is the definition; restated from pycocotools' published maskApi.c and unverified against pycocotools).

`paint_semantic`, `paint_panoptic_semantic`, `paint_instances` and `paint_pose` go the other way (csrc/painter_paint.hip,
include/painter_paint.h): annotations -- label maps, panoptic id maps, instance masks, keypoints -- become the painted TARGET pictures the
reference's offline generators write as PNG files (gen_color_ade20k_sem.py, gen_color_coco_panoptic_segm.py, SaveDataPairCustom,
encode_target_to_image), byte for byte, as uint8 CUDA tensors that `PainterEngine(prompt_tgt=...)`, `PairSpec.target` and every decoder
take (tests/painter_paint_host.py is the definition; mmpose's MSRA rule is restated from its published source and unverified against
mmpose).

Stays on the host, by design: file decode / encode; the depth script's one-off prompt-target preparation
(`Image.fromarray(float array).convert("RGB")`, painter_inference_depth.py:134-145: pass its result as `prompt_tgt`); SIDD's
`cv2.resize` of the float query (painter_inference_sidd.py:136: OpenCV's resize is not restated -- use `run_one_image` with the
canvases the script built, or pass an already resized 448 x 448 uint8 query to `run`) and its eval_sidd.m (MATLAB's built-in ssim /
psnr); of the detectron2
evaluators what is left after the colour -> class decode (`class_map`), the confusion count (`SemsegScore`), the instance decode
(`instances`), the panoptic merge (`panoptic`) and the boundary-IoU branch (`SemsegBoundaryScore`): `encode_json_sem_seg`
and its RLE, the final ratios of `evaluate` (`semseg_scores` restates them on the host); of the depth evaluation its KITTI branches
(`do_kb_crop`, `garg_crop`) and the division of the sums;
PNG encoding and COCOeval's box AP (mask AP: `InstanceAP`; RLE: `rle_encode` / `rle_decode`); of the pose route soft_oks_nms, rle_score and the JSON file (keypoint AP: `KeypointAP`).

One host path serves the routes: `_device` / `_pictures` put the inputs of a call on one indexed CUDA device; INSTANCE_DEFAULTS,
MERGE_DEFAULTS, POSE_DEFAULTS and DEPTH_DEFAULTS hold the keyword defaults and `_check_arguments` refuses the rest before a forward is enqueued; an output
buffer is one list of sections (`_layout`): its size, the pointers handed to the library and the slices of `result()` all come from it.
The three scorers with job tables (`PanopticQuality`, `InstanceAP`, `KeypointAP`) stage their tables through one `_Upload` (sections, pinned
host buffer, ONE asynchronous copy), size their workspace through `_workspace` and word a refused picture through `_refuse`; the two AP
scorers parse COCOeval's parameters with `_coco_params`, and `instance_ap_metrics` / `keypoint_ap_metrics` share one `_coco_accumulate`.

There is no CPU fallback: a CPU device or a missing libpainter_hip.so raises.
"""
import contextlib
import ctypes
import functools
import math

import numpy as np
import torch
from PIL import Image

from ._lib import check, lib
from .seggpt_engine import DeviceIO, _stream

# resize = F.interpolate mode after the forward; scale, clip = `torch.clip((y * std + mean) * scale, 0, scale)` or none;
# kind = u8: `.int()` -> uint8 [H][W][3] PNG | depth: `.mean(-1).int()` -> int32 [H][W] PNG | f64: float64 [H][W][3] returned
TASKS = {
    "ade20k_semseg": dict(resize="bilinear", scale=255.0, clip=True, kind="u8"),          # ade20k_semantic/painter_inference_segm.py
    "coco_pano_semseg": dict(resize="bilinear", scale=255.0, clip=True, kind="u8"),       # coco_panoptic/painter_inference_pano_semseg.py
    "coco_pano_inst": dict(resize="nearest", scale=255.0, clip=True, kind="u8"),          # coco_panoptic/painter_inference_pano_inst.py
    "coco_pose": dict(resize="nearest", scale=255.0, clip=True, kind="u8"),               # mmpose_custom/painter_inference_pose.py
    "nyuv2_depth": dict(resize="bilinear", scale=10000.0, clip=True, kind="depth"),       # nyuv2_depth/painter_inference_depth.py
    "derain": dict(resize="bicubic", scale=1.0, clip=False, kind="f64"),                  # derain/painter_inference_derain.py
    "lol": dict(resize="bicubic", scale=1.0, clip=False, kind="f64"),                     # lol/painter_inference_lol.py
    "sidd": dict(resize="bicubic", scale=1.0, clip=False, kind="f64"),                    # sidd/painter_inference_sidd.py
}
DIST_TYPES = {"abs": 0, "square": 1, "mean": 2}
_OUT = {"u8": (torch.uint8, 3), "depth": (torch.int32, 1), "f64": (torch.float64, 3)}       # dtype, channels


class DecodeJob(ctypes.Structure):
    """pa_decode_job of include/painter_hip.h."""
    _fields_ = [("out", ctypes.c_void_p), ("out2", ctypes.c_void_p), ("sample", ctypes.c_int32), ("out_h", ctypes.c_int32),
                ("out_w", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _task(name):
    if name not in TASKS:
        raise KeyError("painter_engine: unknown task %r (one of %s)" % (name, ", ".join(TASKS)))
    return TASKS[name]


def _unwrap(model):
    return model.module if hasattr(model, "module") else model          # the scripts wrap the model in DistributedDataParallel


def _device(inputs=(), device="cuda"):
    """The one device of a call, always with its index: that of the tensors among `inputs` (pictures, masks, lists of them, None), else
    `device`.  CPU is refused first -- a host address must never reach a kernel -- and so are tensors on two devices."""
    tensors = [t for x in inputs for t in (x if isinstance(x, (list, tuple)) else [x]) if torch.is_tensor(t)]
    devices = {t.device for t in tensors} or {torch.device(device)}
    for d in devices:
        if d.type != "cuda":
            raise RuntimeError("painter_amd.painter_engine runs its image kernels on an MI355X only (no CPU fallback); got %s" % d)
    if len(devices) > 1:
        raise RuntimeError("painter_engine: the inputs are on %s" % " and ".join(sorted(str(d) for d in devices)))
    d = devices.pop()
    return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())


def _pictures(x, device, batch=False):
    """A picture [H][W][3] or, with `batch`, [n][H][W][3] / a list of [H][W][3] of one size (numpy or CUDA tensors) -> contiguous uint8
    CUDA tensor on `device` (what `_device` returned)."""
    if batch and isinstance(x, (list, tuple)):
        assert len(x) >= 1 and len({tuple(p.shape) for p in x}) == 1, "painter_engine: the pictures of a batch have one size"
        x = torch.stack(list(x)) if torch.is_tensor(x[0]) else np.stack(x)
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if x.device != device:
        raise RuntimeError("painter_engine: the pictures are on %s, expected %s" % (x.device, device))
    assert x.dtype == torch.uint8 and x.dim() == 3 + batch and x.shape[-1] == 3, (x.dtype, tuple(x.shape))
    return x.contiguous()


def _maps(x, device, dtype):
    """A one-channel map [H][W] (numpy or CUDA tensor) of `dtype` (a torch dtype; uint16 may also arrive as its int16 bits) -> contiguous
    CUDA tensor on `device` (what `_device` returned)."""
    if not torch.is_tensor(x):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(device)
    if x.device != device:
        raise RuntimeError("painter_engine: the maps are on %s, expected %s" % (x.device, device))
    ok = (torch.uint16, torch.int16) if dtype == torch.uint16 else (dtype,)
    assert x.dtype in ok and x.dim() == 2, (x.dtype, tuple(x.shape))
    return x.contiguous()


def _job_table(jobs, device):
    """A ctypes array of job records -> (its pinned host copy, the table on the device).  Pinned + asynchronous: the copy is ordered on the
    stream and the host does not wait for work enqueued earlier."""
    host = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).pin_memory()
    return host, host.to(device, non_blocking=True)


def _rgb_palette(palette, default):
    """[K][3] colours, or None for `default()` -> float32 numpy [K][3], a copy (the default palettes are cached and read-only)."""
    pal = np.array(default() if palette is None else palette, dtype=np.float32, order="C")
    assert pal.ndim == 2 and pal.shape[1] == 3 and (pal == np.floor(pal)).all() and pal.min() >= 0 and pal.max() <= 255, \
        "painter_engine: the palette holds integer colours 0..255"
    return pal


def _check_arguments(who, kw, *tables):
    """What can be refused before anything is enqueued: a keyword no default table has, an unknown `dist_type` or NMS `kernel`."""
    unknown = set(kw).difference(*tables)
    if unknown:
        raise TypeError("%s: unexpected arguments %s" % (who, sorted(unknown)))
    if "dist_type" in kw and kw["dist_type"] not in DIST_TYPES:
        raise NotImplementedError(kw["dist_type"])
    if "kernel" in kw and kw["kernel"] not in NMS_KERNELS:
        raise NotImplementedError("%s kernel is not supported in matrix nms!" % kw["kernel"])


@contextlib.contextmanager
def _eval_mode(model):
    """The model in eval mode; it goes back to the mode it had."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def _layout(sections, base=0):
    """sections = [(name, dtype, count, alignment)] in buffer order, from byte `base` -> ({name: (byte offset, dtype, count)}, end).  An
    empty section takes no room, not even its padding: `end` is where the last section that holds something ends."""
    at, o, end = {}, base, base
    for name, dtype, count, align in sections:
        o, dtype, count = -(-o // align) * align, np.dtype(dtype), int(count)
        at[name] = (o, dtype, count)
        o += dtype.itemsize * count
        end = o if count else end
    return at, end


def _section(host, at, name, count=None):
    """The first `count` elements (default: all) of a section of `_layout` in the buffer's host copy, in the section's dtype."""
    off, dtype, n = at[name]
    return host[off:off + dtype.itemsize * (n if count is None else count)].view(dtype)


class _Upload:
    """The tables of one scoring call, staged as sections (`_layout`; "jobs" is the job table) of a zeroed pinned host buffer with its twin
    on the device: `up.put(name, values)` fills a section (its first len(values) elements) and returns its device address, `up.send(jobs)`
    puts the job records in and enqueues the ONE asynchronous copy.  `host` and `dev` must outlive the launches that read them."""

    def __init__(self, sections, device):
        self.at, size = _layout(sections)
        self.host = torch.zeros(size, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(size, dtype=torch.uint8, device=device)
        self._bytes, self._base = self.host.numpy(), self.dev.data_ptr()          # once: a data set has hundreds of sections

    def put(self, name, values):
        # one call per section and no call below it: KeypointAP stages three sections per photo, hundreds of photos per call
        off, dtype, _ = self.at[name]
        self._bytes[off:off + dtype.itemsize * len(values)].view(dtype)[:] = values
        return self._base + off

    def send(self, jobs):
        at = self.put("jobs", np.frombuffer(bytearray(jobs), np.uint8))
        self.dev.copy_(self.host, non_blocking=True)
        return at


def _workspace(size_of, shape, what, device):
    """The workspace the library asks for at the capacities `shape`; sizes it refuses (-1) fail as `what` would."""
    nbytes = size_of(*shape)
    if nbytes < 0:
        check(1, what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _refuse(who, flags, reasons, k=None, name=lambda i: "picture %d" % i, rest="pictures are refused and emit nothing"):
    """ValueError for the first non-zero word of `flags`, the flag words a scoring kernel left per picture: which picture, its lowest flag
    bit, what that bit means (`reasons`; `k` fills a "%d classes") and how many are refused."""
    bad = np.flatnonzero(flags)
    if len(bad):
        word = int(flags[bad[0]])
        bit = (word & -word).bit_length() - 1
        why = reasons[bit] % k if "%d" in reasons[bit] else reasons[bit]
        raise ValueError("%s: %s is refused (flag bit %d, flags 0x%02x): %s; %d of %d %s"
                         % (who, name(bad[0]), bit, word, why, len(bad), len(flags), rest))


def _coco_params(iou_thrs, area_ranges, max_dets):
    """COCOeval's Params as both AP scorers take them -> (iou_thrs float64 [T], area_ranges float64 [A][2], max_dets tuple, ok): a record's
    words hold one bit per (range, threshold), so T * A <= 64."""
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.array(iou_thrs, np.float64).ravel()
    area_ranges = np.array(area_ranges, np.float64).reshape(-1, 2)
    max_dets = tuple(int(m) for m in max_dets)
    return iou_thrs, area_ranges, max_dets, 1 <= len(iou_thrs) * len(area_ranges) <= 64 and bool(max_dets)


def _forward(model, imgs, tgts):
    """The model call of the scripts' run_one_image (painter_inference_segm.py:76-84): second half of the canvas masked, everything
    valid; eval mode, no_grad.  -> float32 tokens [N][L][p*p*3].  The mask has the RUN-TIME number of tokens (h * w // patch_size ** 2,
    painter_inference_pano_semseg.py:78): an engine at input_size=560 runs the 896 x 448 checkpoint on 70 x 35 tokens."""
    p = int(model.patch_size)
    n = (imgs.shape[2] // p) * (imgs.shape[3] // p)
    masked = torch.zeros(1, n, device=imgs.device)
    masked[:, n // 2:] = 1
    return model(imgs, tgts, masked, torch.ones_like(tgts))[1]


class DecodePlan:
    """Everything a decode launch needs that depends only on the task and the output sizes: the flat output buffer(s), one view
    (offset, shape) per picture and the job table on the device."""

    def __init__(self, task, sizes, device, saved=False, samples=None):
        self.task, self.spec = task, _task(task)
        dtype, ch = _OUT[self.spec["kind"]]
        self.views, total = [], 0
        for (w, h) in sizes:
            w, h = int(w), int(h)
            assert w >= 1 and h >= 1, (w, h)
            self.views.append((total, (h, w, 3) if ch == 3 else (h, w)))
            total += h * w * ch
        self.out = torch.empty(total, dtype=dtype, device=device)
        self.out8 = torch.empty(total, dtype=torch.uint8, device=device) if saved and self.spec["kind"] == "f64" else None
        n = len(self.views)
        jobs = (DecodeJob * n)()
        for i, (off, shape) in enumerate(self.views):
            jobs[i].out = self.out.data_ptr() + off * self.out.element_size()
            jobs[i].out2 = None if self.out8 is None else self.out8.data_ptr() + off
            jobs[i].sample = i if samples is None else int(samples[i])
            jobs[i].out_h, jobs[i].out_w = shape[0], shape[1]
        self._table_host, self.table = _job_table(jobs, device)
        self.n_jobs = n
        self.max_h, self.max_w = max(v[1][0] for v in self.views), max(v[1][1] for v in self.views)

    def launch(self, pred, res_h, res_w, patch):
        """ONE launch over pred = float32 CUDA tokens [N][L][p*p*3]."""
        pred = pred.detach().to(torch.float32).contiguous()
        assert pred.is_cuda and pred.dim() == 3 and \
            tuple(pred.shape[1:]) == ((2 * res_h // patch) * (res_w // patch), patch * patch * 3), tuple(pred.shape)
        args = (pred.data_ptr(), self.table.data_ptr(), self.n_jobs, int(pred.shape[0]), self.max_h, self.max_w, res_h, res_w, patch)
        if self.spec["kind"] == "u8":
            check(lib.pa_painter_decode_u8(*args, 1 if self.spec["resize"] == "nearest" else 0, _stream()), "pa_painter_decode_u8")
        elif self.spec["kind"] == "depth":
            check(lib.pa_painter_decode_depth(*args, _stream()), "pa_painter_decode_depth")
        else:
            check(lib.pa_painter_decode_f64(*args, _stream()), "pa_painter_decode_f64")
        return self

    def picture(self, i):
        """Picture i of the output as a device view [H][W][3] (depth: [H][W])."""
        off, shape = self.views[i]
        return self.out[off:off + int(np.prod(shape))].view(shape)

    def run_of(self, first, count):
        """Pictures first .. first + count, all of one size, as ONE device view [count][H][W][3]."""
        off, shape = self.views[first]
        assert all(v[1] == shape for v in self.views[first:first + count]) and first + count <= self.n_jobs
        return self.out[off:off + count * int(np.prod(shape))].view((count,) + shape)

    def saved_picture(self, i):
        """f64 tasks planned with `saved`: picture i of the uint8 output as a device view [H][W][3]."""
        off, shape = self.views[i]
        return self.out8[off:off + int(np.prod(shape))].view(shape)

    def pictures(self):
        """The copy back (and the one synchronisation) -> one numpy array per picture."""
        return _split(self.out, self.views)

    def saved_pictures(self):
        """f64 tasks planned with `saved`: the uint8 pictures the restoration scripts save, `uint8(clip(out, 0, 1) * 255)`."""
        return _split(self.out8, self.views)


def decode(task, pred, sizes, res_h, res_w, patch, saved=False):
    """Plan and launch in one call: sizes = [(width, height)] per sample of pred, as the scripts pass them.  -> the DecodePlan
    (`.pictures()`, `.saved_pictures()`)."""
    assert len(sizes) == pred.shape[0], (len(sizes), tuple(pred.shape))
    return DecodePlan(task, sizes, pred.device, saved=saved).launch(pred, res_h, res_w, patch)


def _split(flat, views):
    a = flat.cpu().numpy()
    return [a[off:off + int(np.prod(shape))].reshape(shape) for off, shape in views]


def class_map(picture, palette, dist_type="abs", device="cuda"):
    """ADE20kSemSegEvaluatorCustom.post_process_segm_output (:114-141): uint8 [H][W][3] picture (numpy or CUDA tensor), palette
    [K][3] -> int32 [H][W] numpy, the index of the nearest palette colour (first minimum)."""
    device = _device([picture], device)
    _check_arguments("class_map", dict(dist_type=dist_type), MERGE_DEFAULTS)
    img = _pictures(picture, device)
    pal = torch.as_tensor(np.asarray(palette), dtype=torch.float32).to(device).contiguous()
    assert pal.dim() == 2 and pal.shape[1] == 3, tuple(pal.shape)
    h, w = int(img.shape[0]), int(img.shape[1])
    out = torch.empty((h, w), dtype=torch.int32, device=device)
    check(lib.pa_palette_argmin(img.data_ptr(), pal.data_ptr(), out.data_ptr(), h, w, int(pal.shape[0]), DIST_TYPES[dist_type], _stream()),
          "pa_palette_argmin")
    return out.cpu().numpy()


NMS_KERNELS = {"gaussian": 0, "linear": 1}
# The keyword families and their defaults, written once: the run_* entry points read them, the public signatures repeat them for their
# readers (tests/test_painter_pano_cpu.py holds them to it).  INSTANCE_ and POSE_DEFAULTS are in InstanceDecode's / PoseDecode's order.
INSTANCE_DEFAULTS = dict(palette=None, dist_thr=19.0, nms_pre=2000, max_num=100, kernel="gaussian", sigma=2.0)
MERGE_DEFAULTS = dict(semseg_palette=None, n_things=80, dist_type="abs", overlap_threshold=0.5, stuff_area_thresh=8192,
                      instances_score_thresh=0.55)                                   # get_args_parser_pano_seg (COCOPanoEvaluatorCustom.py:279-297)


@functools.lru_cache(maxsize=4)
def location_palette(num_location_r=16, num_location_gb=20):
    """The colours the `coco_pano_inst` targets are painted with, one per location, as float32 [16 * num_location_gb^2][3] without the
    background row (define_colors_per_location_r_gb, COCOCAInstSegEvaluatorCustom.py:42-67): red steps down by 255 // num_location_r
    per cell of the 4 x 4 global grid (row-major), green by 256 // num_location_gb + 1 per local row, blue by the same per local column."""
    sep_r, sep_gb = 255 // num_location_r, 256 // num_location_gb + 1
    cell, y, x = np.meshgrid(np.arange(16), np.arange(num_location_gb), np.arange(num_location_gb), indexing="ij")
    pal = np.stack([255 - cell * sep_r, 255 - y * sep_gb, 255 - x * sep_gb], -1).reshape(-1, 3)
    assert pal.min() >= 0 and len({tuple(c) for c in pal.tolist()}) == len(pal)
    pal = pal.astype(np.float32)
    pal.setflags(write=False)                  # cached: every caller sees the same array
    return pal


class InstanceDecode:
    """One launched pa_inst_decode: every output sits in ONE device buffer, so `result()` is one copy back and one synchronisation."""

    def __init__(self, picture, palette, thresholds, nms_pre, max_num, kernel, sigma, tail=0):
        """tail: further bytes at the end of the output buffer, from offset `self.tail`, for what a caller chains behind the decode."""
        _check_arguments("InstanceDecode", dict(kernel=kernel), INSTANCE_DEFAULTS)
        dev = picture.device
        self.img = img = _pictures(picture, dev)
        pal = _rgb_palette(palette, location_palette)
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float32))
        self.h, self.w, self.k, self.n_thr = int(img.shape[0]), int(img.shape[1]), int(pal.shape[0]), int(thr.size)
        self.nms_pre, self.max_num = int(nms_pre), int(max_num)
        self.words = (self.h * self.w + 31) // 32
        shape = (self.h, self.w, self.k, self.n_thr, self.nms_pre)
        nbytes = lib.pa_inst_workspace_bytes(*shape)
        if nbytes < 0 or self.max_num < 1 or self.max_num > self.nms_pre:
            check(1, "pa_inst_decode (sizes %s, max_num %d)" % (shape, self.max_num))
        self.shape = shape
        self.params = torch.from_numpy(np.concatenate([pal.ravel(), thr])).to(dev, non_blocking=True)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        m = self.max_num
        # ONE byte buffer, every output a section of it
        self.at, size = _layout([("count", np.int32, 1, 1), ("scores_f64", np.float64, m, 8), ("scores", np.float32, m, 1),
                                 ("candidates", np.int32, m, 1), ("bits", np.uint32, m * self.words, 1), ("masks", np.bool_, m * self.h * self.w, 1),
                                 ("tail", np.uint8, int(tail), 16)])
        self.o32, self.obits, self.obytes, self.tail = (self.at[name][0] for name in ("scores", "bits", "masks", "tail"))
        self.out = torch.zeros(size, dtype=torch.uint8, device=dev)
        ptr = lambda name: self.out.data_ptr() + self.at[name][0]
        check(lib.pa_inst_decode(img.data_ptr(), self.params.data_ptr(), self.params.data_ptr() + 4 * pal.size, self.h, self.w, self.k,
                                 self.n_thr, self.nms_pre, m, float(sigma), NMS_KERNELS[kernel], self.workspace.data_ptr(), ptr("count"),
                                 ptr("scores"), ptr("scores_f64"), ptr("candidates"), ptr("bits"), ptr("masks"), _stream()), "pa_inst_decode")

    def section(self, which, dtype, count):
        """A section of the workspace (pa_inst_workspace_offset) as a numpy array: for tests and tools."""
        off = lib.pa_inst_workspace_offset(*self.shape, which)
        return self.workspace[off:off + count * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)

    def result(self, with_f64=False, with_bits=False, host=None):
        """The copy back (and the one synchronisation).  The bool masks are a view of the bytes the device wrote.  host: the output
        buffer as numpy, if the caller has copied it back already."""
        a = self.out.cpu().numpy() if host is None else host
        n = int(_section(a, self.at, "count")[0])
        if n == 0:              # no candidate: the reference's single all-zero mask with score 0 and label 0 (:302-310)
            res = dict(scores=np.zeros(1, np.float32), labels=np.zeros(1, np.float32), masks=np.zeros((1, self.h, self.w), bool),
                       candidates=np.full(1, -1, np.int32))
            if with_f64:
                res["scores_f64"] = np.zeros(1)
            return res
        res = dict(scores=_section(a, self.at, "scores", n), labels=np.ones(n, np.float32),
                   masks=_section(a, self.at, "masks", n * self.h * self.w).reshape(n, self.h, self.w),
                   candidates=_section(a, self.at, "candidates", n))
        if with_f64:
            res["scores_f64"] = _section(a, self.at, "scores_f64", n)
        if with_bits:
            res["bits"] = _section(a, self.at, "bits", n * self.words).reshape(n, self.words)
        return res


def instances(picture, palette=None, dist_thr=19.0, nms_pre=2000, max_num=100, kernel="gaussian", sigma=2.0, device="cuda"):
    """COCOCAInstSegEvaluatorCustom.post_process_segm_output_by_threshold (:252-354) with mask_matrix_nms (util/matrix_nms.py:5-121):
    uint8 [H][W][3] picture (numpy or CUDA tensor), palette [K][3] (default `location_palette()`), dist_thr a threshold or a list of them
    -> dict(scores float32 [n], labels float32 [n], masks bool [n][H][W], candidates int32 [n] = t * K + c of each instance).
    Ties are defined (include/painter_hip.h): exact integer statistics, rational maskness order, stable sorts, float64 NMS."""
    return InstanceDecode(_pictures(picture, _device([picture], device)), palette, dist_thr, nms_pre, max_num, kernel, sigma).result()


# ---- instance decode by nearest colour, the evaluator's post_type "minmax" (csrc/painter_minmax.hip, include/painter_minmax.h)
POST_TYPES = ("threshold", "minmax")                 # COCOEvaluatorCustom.process (:135-141)
MINMAX_DEFAULTS = dict(palette=None)
MINMAX_RECORD = np.dtype([("colour", np.int32), ("cls", np.int32), ("n", np.uint32), ("reserved", np.uint32), ("S", np.uint64),
                          ("neg", np.float32), ("score", np.float32)])                           # pa_minmax_record


class MinmaxDecode:
    """One launched pa_minmax_decode: label and distance map, statistics, instance records and the colour -> slot table, all in ONE device
    buffer.  The masks are not part of it: their number is the instance count, so `bits()` reads the count back (once) and sizes them by
    it -- any number of instances up to K + 1 comes out, nothing is cut."""

    def __init__(self, picture, palette=None):
        dev = picture.device
        self.img = img = _pictures(picture, dev)
        pal = np.concatenate([_rgb_palette(palette, location_palette), np.zeros((1, 3), np.float32)])      # black appended (:114-115)
        self.h, self.w, self.k = int(img.shape[0]), int(img.shape[1]), int(pal.shape[0])
        self.words = (self.h * self.w + 31) // 32
        self.shape = (self.h, self.w, self.k)
        self.workspace = _workspace(lib.pa_minmax_workspace_bytes, self.shape, "pa_minmax_decode (sizes %s)" % (self.shape,), dev)
        self.params = torch.from_numpy(pal).to(dev, non_blocking=True)
        hw = self.h * self.w
        self.at, size = _layout([("count", np.int32, 1, 4), ("records", MINMAX_RECORD, self.k, 8), ("slot", np.int32, self.k, 4),
                                 ("label", np.uint16, hw, 2), ("dist", np.uint16, hw, 2)])
        self.out = torch.zeros(size, dtype=torch.uint8, device=dev)
        self._n, self._bits, self._bytes = None, None, None
        check(lib.pa_minmax_decode(img.data_ptr(), self.params.data_ptr(), self.h, self.w, self.k, self.workspace.data_ptr(), self.ptr("label"),
                                   self.ptr("dist"), self.ptr("count"), self.ptr("records"), self.ptr("slot"), _stream()), "pa_minmax_decode")

    def ptr(self, name):
        return self.out.data_ptr() + self.at[name][0]

    def count(self):
        """The number of instances: four bytes back and the one synchronisation, once."""
        if self._n is None:
            o = self.at["count"][0]
            self._n = int(self.out[o:o + 4].cpu().numpy().view(np.int32)[0])
        return self._n

    def bits(self, with_bytes=False):
        """-> (bit masks int32 CUDA [n][ceil(H W / 32)] in pa_inst_decode's layout, n): what `masks=` arguments and the RLE encode take.
        with_bytes: -> (bits, bool CUDA [n][H][W], n)."""
        n = self.count()
        if self._bits is None or (with_bytes and self._bytes is None):
            dev = self.out.device
            bits = torch.empty((n, self.words), dtype=torch.int32, device=dev)
            dense = torch.empty((n, self.h, self.w), dtype=torch.bool, device=dev) if with_bytes else None
            check(lib.pa_minmax_masks(self.ptr("label"), self.ptr("slot"), self.h, self.w, self.k, 0, n, bits.data_ptr(),
                                      None if dense is None else dense.data_ptr(), _stream()), "pa_minmax_masks")
            self._bits, self._bytes = bits, dense if dense is not None else self._bytes
        return (self._bits, self._bytes, n) if with_bytes else (self._bits, n)

    def result(self, with_bits=False):
        """The copy back of the buffer, then the masks' launch and copy back."""
        a = self.out.cpu().numpy()
        self._n = n = int(_section(a, self.at, "count")[0])
        rec = _section(a, self.at, "records", n)
        bits, dense, _ = self.bits(with_bytes=True)
        res = dict(scores=rec["score"].copy(), labels=rec["cls"].astype(np.float32), candidates=rec["colour"].copy(),
                   areas=rec["n"].astype(np.int32), pred_map=_section(a, self.at, "label").astype(np.int32).reshape(self.h, self.w),
                   dist_map=_section(a, self.at, "dist").astype(np.float32).reshape(self.h, self.w), masks=dense.cpu().numpy())
        if with_bits:
            res["bits"] = bits.cpu().numpy().view(np.uint32)
        return res


def instances_minmax(picture, palette=None, device="cuda"):
    """COCOCAInstSegEvaluatorCustom.post_process_segm_output_by_minmax (:172-250), the evaluator's `post_type="minmax"`: uint8 [H][W][3]
    picture (numpy or CUDA tensor), palette [K][3] without the background row (default `location_palette()`; black is appended as the
    evaluator's constructor does) -> dict(scores float32 [n], labels float32 [n] (0 for the background instance, otherwise 1), candidates
    int32 [n] (the palette row), areas int32 [n], pred_map int32 [H][W], dist_map float32 [H][W], masks bool [n][H][W]), the instances in
    ascending palette row.  Every pixel goes to its nearest colour in L1, the lowest row on a tie; there is no NMS and no top-k
    (tests/painter_minmax_host.py is the definition)."""
    return MinmaxDecode(_pictures(picture, _device([picture], device)), palette).result()


def _post_type(who, kw, semseg_engine=None):
    """Pops `post_type` (default "threshold") from the keywords of a run_* entry point, before their own check.  "minmax" takes `palette`
    only of the instance keywords and has no class vote behind it; anything else raises as the evaluator does (:141)."""
    post_type = kw.pop("post_type", "threshold")
    if post_type not in POST_TYPES:
        raise NotImplementedError("post_type %r (one of %s)" % (post_type, ", ".join(POST_TYPES)))
    if post_type == "minmax":
        if semseg_engine is not None:
            raise ValueError("%s: post_type=\"minmax\" is not offered together with semseg_engine" % who)
        _check_arguments(who + " (post_type=\"minmax\")", kw, MINMAX_DEFAULTS)
    return post_type


# ---- pose keypoints (csrc/painter_pose.hip)
# configs/_base_/coco.py: the left / right partners (`swap`) of COCO's 17 keypoints
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
POSE_DEFAULTS = dict(palette=None, flip_pairs=COCO_FLIP_PAIRS, shift_heatmap=True)


@functools.lru_cache(maxsize=4)
def pose_palette(num_locations=17):
    """The (G, B) colours the `coco_pose` targets are painted with, one per keypoint, plus the background row (0, 0) LAST, as int32
    [num_locations + 1][2] (define_colors_gb_mean_sep, mmpose_custom/data/pipelines/custom_transform.py:10-33; the row TopDownCustom
    appends, model/top_down.py:28-30): green steps down by 256 // (isqrt(n) + 1) per row of the grid, blue by the same per column."""
    per = int(num_locations ** (1 / 2)) + 1
    sep, k = 256 // per, np.arange(num_locations)
    pal = np.concatenate([np.stack([255 - k // per * sep, 255 - k % per * sep], -1), [[0, 0]]]).astype(np.int32)
    assert pal.min() >= 0 and len({tuple(c) for c in pal.tolist()}) == len(pal)
    pal.setflags(write=False)                  # cached: every caller sees the same array
    return pal


class PoseDecode:
    """One launched pa_pose_keypoints (or pa_pose_heatmaps): preds and maxvals sit in ONE device buffer, so `result()` is one copy back
    and one synchronisation."""

    def __init__(self, pictures, flipped=None, palette=None, flip_pairs=COCO_FLIP_PAIRS, shift_heatmap=True, heatmaps=False):
        self.img, self.flip = img, flip = pictures, flipped
        dev = img.device
        assert flip is None or (flip.device == dev and flip.shape == img.shape), "painter_engine: pictures and flipped pictures differ"
        pal = np.ascontiguousarray(np.asarray(pose_palette() if palette is None else palette)).astype(np.int32)
        assert pal.ndim == 2 and pal.shape[1] == 2 and pal.shape[0] >= 1, "painter_engine: the pose palette is [K + 1][2], background last"
        self.n, self.h, self.w, self.k = int(img.shape[0]), int(img.shape[1]), int(img.shape[2]), int(pal.shape[0]) - 1
        pair = np.arange(max(self.k, 0), dtype=np.int32)
        for a, b in flip_pairs:
            assert 0 <= a < self.k and 0 <= b < self.k and pair[a] == a and pair[b] == b, "painter_engine: flip_pairs are disjoint pairs of channels"
            pair[a], pair[b] = b, a
        shape = (self.n, self.h, self.w, self.k)
        what = "pa_pose_heatmaps" if heatmaps else "pa_pose_keypoints"
        nbytes = lib.pa_pose_workspace_bytes(self.n, self.k)
        if nbytes < 0 or self.h < 1 or self.w < 1:
            check(1, "%s (sizes %s)" % (what, shape))
        self.tables = torch.from_numpy(np.concatenate([pal.ravel(), pair])).to(dev, non_blocking=True)
        args = (img.data_ptr(), None if flip is None else flip.data_ptr(), self.tables.data_ptr(), self.tables.data_ptr() + 4 * pal.size,
                *shape, 1 if shift_heatmap else 0)
        if heatmaps:
            self.out = torch.empty((self.n, self.k, self.h, self.w), dtype=torch.float32, device=dev)
            check(lib.pa_pose_heatmaps(*args, self.out.data_ptr(), _stream()), "%s (sizes %s)" % (what, shape))
        else:
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.out = torch.empty(3 * self.n * self.k, dtype=torch.float32, device=dev)           # preds [n][K][2] | maxvals [n][K]
            check(lib.pa_pose_keypoints(*args, self.workspace.data_ptr(), self.out.data_ptr(), self.out.data_ptr() + 8 * self.n * self.k,
                                        _stream()), "%s (sizes %s)" % (what, shape))

    def result(self):
        """The copy back (and the one synchronisation) -> dict(preds float32 [n][K][2], maxvals float32 [n][K])."""
        a, m = self.out.cpu().numpy(), 2 * self.n * self.k
        return dict(preds=a[:m].reshape(self.n, self.k, 2), maxvals=a[m:].reshape(self.n, self.k))


def _pose_inputs(pictures, flipped, device):
    device = _device([pictures, flipped], device)
    return _pictures(pictures, device, batch=True), None if flipped is None else _pictures(flipped, device, batch=True)


def keypoints(pictures, flipped=None, palette=None, flip_pairs=COCO_FLIP_PAIRS, shift_heatmap=True, device="cuda"):
    """TopDownCustom.forward_pseudo_test (mmpose_custom/model/top_down.py:163-258) and the head's decode, mmpose 0.x
    keypoints_from_heatmaps with post_process='default' and no UDP, for n painted person boxes at once.

    pictures: the painted `coco_pose` pictures, uint8 [n][H][W][3] or a list of [H][W][3] of one size (numpy or CUDA tensors); flipped:
    what the network painted for the mirrored boxes (the reference's `_flip` directory), same shape, or None for no flip test; palette:
    int [K + 1][2] (G, B) colours, background last (default `pose_palette()`); flip_pairs: the channels a mirror swaps; shift_heatmap:
    the one-column shift of the flipped heat maps (`shift_heatmap=True` of configs/coco_256x192_test_offline.py).

    -> dict(preds float32 [n][K][2] = (x, y) in heat-map pixels, maxvals float32 [n][K]): per channel the first maximum of
    (heat + flipped heat) / 2 in row-major order, moved a quarter pixel towards the larger neighbour inside the border; (-1, -1) and 0
    for a channel no pixel shows.  The float32 values are the reference's own (one add of two `R / 255` table values, one halving), so
    ties fall as its argmax lets them.  `to_image` maps preds to the photo."""
    return PoseDecode(*_pose_inputs(pictures, flipped, device), palette, flip_pairs, shift_heatmap).result()


def pose_heatmaps(pictures, flipped=None, palette=None, flip_pairs=COCO_FLIP_PAIRS, shift_heatmap=True, device="cuda"):
    """The `output_heatmap` of forward_pseudo_test(return_heatmap=True) for the arguments of `keypoints` -> float32 numpy [n][K][H][W].
    `keypoints` never builds it."""
    return PoseDecode(*_pose_inputs(pictures, flipped, device), palette, flip_pairs, shift_heatmap, heatmaps=True).out.cpu().numpy()


def to_image(preds, center, scale, heatmap_size):
    """Heat-map pixels -> photo pixels for one box: preds [K][2], center (x, y) and scale (w, h) / 200 of the box as mmpose's
    img_metas carry them, heatmap_size (W, H).  Restates mmpose 0.x `transform_preds(coords, center, scale, output_size, use_udp=False)`
    from its published source; mmpose is not available where this project is tested, so the formula is unverified against it."""
    preds = np.asarray(preds)
    full = np.asarray(scale, dtype=np.float64) * 200.0
    out = np.ones_like(preds)
    out[:, 0] = preds[:, 0] * (full[0] / heatmap_size[0]) + center[0] - full[0] * 0.5
    out[:, 1] = preds[:, 1] * (full[1] / heatmap_size[1]) + center[1] - full[1] * 0.5
    return out


# ---- scoring against ground truth (csrc/painter_score.hip)
DEPTH_DEFAULTS = dict(min_depth=1e-3, max_depth=80.0, crop=None, divisor=1000.0)      # eval_with_pngs.py:43-44, no crop, :100 / :136 (nyu)
EIGEN_CROP = (45, 471, 41, 601)                                                        # eval_with_pngs.py:205, of 480 x 640 pictures


class ScoreJob(ctypes.Structure):
    """pa_score_job of include/painter_hip.h."""
    _fields_ = [("picture", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class BoundaryJob(ctypes.Structure):
    """pa_boundary_job of include/painter_hip.h."""
    _fields_ = [("picture", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("d", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class DepthJob(ctypes.Structure):
    """pa_depth_job of include/painter_hip.h."""
    _fields_ = [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("y1", ctypes.c_int32), ("x0", ctypes.c_int32), ("x1", ctypes.c_int32)]


def _same_sizes(who, pictures, gts):
    if len(pictures) != len(gts):
        raise ValueError("%s: %d pictures, %d ground-truth maps" % (who, len(pictures), len(gts)))
    for i, (p, g) in enumerate(zip(pictures, gts)):
        if tuple(p.shape[:2]) != tuple(g.shape):
            raise ValueError("%s: picture %d is %s, its ground truth %s" % (who, i, tuple(p.shape[:2]), tuple(g.shape)))


def _positive_ratio(who, dilation_ratio):
    ratio = float(dilation_ratio)
    if not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("%s: dilation_ratio is a finite number > 0, not %r" % (who, dilation_ratio))
    return ratio


def boundary_dilation(h, w, dilation_ratio=0.02):
    """The erosion count of detectron2's SemSegEvaluator._mask_to_boundary for a picture of h x w: `int(round(dilation_ratio *
    sqrt(h^2 + w^2)))` in float64 with Python's round (half to even), at least 1."""
    h, w = int(h), int(w)
    return max(1, int(round(_positive_ratio("boundary_dilation", dilation_ratio) * math.sqrt(h * h + w * w))))


def label_boundary(label_map, dilation_ratio=0.02, device="cuda"):
    """What the boundary branch makes of one label map, uint8 [H][W] (numpy or CUDA tensor) -> uint8 numpy [H][W]: the map minus its
    erosion by a 3 x 3 square, `boundary_dilation(H, W, dilation_ratio)` times, behind a ring of zeros (pa_label_boundary: the row and
    column passes of `SemsegBoundaryScore`).  The minimum is over label values, as detectron2 erodes the label map itself; restated from
    detectron2's published source and unverified against detectron2 / cv2."""
    ratio = _positive_ratio("label_boundary", dilation_ratio)
    device = _device([label_map], device)
    m = _maps(label_map, device, torch.uint8)
    h, w = int(m.shape[0]), int(m.shape[1])
    if h < 1 or w < 1:
        return np.zeros((h, w), np.uint8)
    what = "pa_label_boundary (%d x %d)" % (h, w)
    workspace = _workspace(lib.pa_semseg_boundary_workspace_bytes, (h * w,), what, device)
    out = torch.empty((h, w), dtype=torch.uint8, device=device)
    check(lib.pa_label_boundary(m.data_ptr(), h, w, boundary_dilation(h, w, ratio), out.data_ptr(), workspace.data_ptr(), _stream()), what)
    return out.cpu().numpy()


def semseg_scores(matrix, boundary_matrix=None):
    """detectron2's SemSegEvaluator.evaluate (detectron2/evaluation/sem_seg_evaluation.py) from the confusion matrix int64
    [K + 1][K + 1] (rows = predictions, columns = ground truth, the last column = ignored pixels), in float64: -> dict(mIoU, fwIoU, mACC,
    pACC in percent, IoU and ACC float64 [K] in percent, NaN for a class without ground-truth pixels).  A class that the ground truth does
    not show is left out of every mean (the release with the boundary-IoU branch, which the reference's evaluators are written against);
    the ignore column and the (empty) ignore row enter nothing.  With `boundary_matrix` (`SemsegBoundaryScore.boundary_matrix()`) two more
    keys, float64 [K] in percent: BoundaryIoU = diagonal / union of the boundary matrix, NaN where the union is empty (no condition on the
    ground truth here), and minIoU_BIoU, the evaluator's `min(IoU, B-Iou)` with Python's min -- the boundary IoU where it is smaller,
    else the IoU, so a NaN IoU stays NaN and a NaN boundary IoU gives the IoU.
    Restated from detectron2's published source; detectron2 is not available where this project is tested, so the formulas are
    unverified against detectron2."""
    conf = np.asarray(matrix)
    assert conf.ndim == 2 and conf.shape[0] == conf.shape[1] and conf.shape[0] >= 2, conf.shape
    k = conf.shape[0] - 1
    tp = conf.diagonal()[:-1].astype(np.float64)
    pos_gt = conf[:-1, :-1].sum(axis=0).astype(np.float64)
    pos_pred = conf[:-1, :-1].sum(axis=1).astype(np.float64)
    class_weight = pos_gt / pos_gt.sum() if pos_gt.sum() else np.zeros(k)
    acc_valid = pos_gt > 0
    acc = np.full(k, np.nan)
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    union = pos_gt + pos_pred - tp
    iou_valid = acc_valid & (union > 0)
    iou = np.full(k, np.nan)
    iou[iou_valid] = tp[iou_valid] / union[iou_valid]
    macc = acc[acc_valid].sum() / acc_valid.sum() if acc_valid.any() else np.nan
    miou = iou[iou_valid].sum() / iou_valid.sum() if iou_valid.any() else np.nan
    fiou = (iou[iou_valid] * class_weight[iou_valid]).sum()
    pacc = tp.sum() / pos_gt.sum() if pos_gt.sum() else np.nan
    res = dict(mIoU=100 * miou, fwIoU=100 * fiou, mACC=100 * macc, pACC=100 * pacc, IoU=100 * iou, ACC=100 * acc)
    if boundary_matrix is not None:
        b_conf = np.asarray(boundary_matrix)
        assert b_conf.shape == conf.shape, (b_conf.shape, conf.shape)
        b_tp = b_conf.diagonal()[:-1].astype(np.float64)
        b_union = b_conf[:-1, :-1].sum(axis=0).astype(np.float64) + b_conf[:-1, :-1].sum(axis=1).astype(np.float64) - b_tp
        b_iou = np.full(k, np.nan)
        b_iou[b_union > 0] = b_tp[b_union > 0] / b_union[b_union > 0]
        with np.errstate(invalid="ignore"):
            res.update(BoundaryIoU=100 * b_iou, minIoU_BIoU=100 * np.where(b_iou < iou, b_iou, iou))
    return res


class SemsegScore:
    """The confusion matrix of a data set of painted semantic pictures, kept on the device (pa_semseg_confusion):
    SemSegEvaluatorCustom.process (ADE20kSemSegEvaluatorCustom.py:75-112, COCOPanoSemSegEvaluatorCustom.py:67-106) without the distance
    tensor, the copy of the class map and np.bincount.  palette: [K][3] integer colours, K <= 255; a class is `class_map`'s."""

    def __init__(self, palette, dist_type="abs", ignore_label=255, device="cuda"):
        self.device = _device((), device)
        _check_arguments("SemsegScore", dict(dist_type=dist_type), MERGE_DEFAULTS)
        pal = _rgb_palette(palette, None)
        self.k, self.dist_type, self.ignore_label = int(pal.shape[0]), dist_type, int(ignore_label)
        self.bins = 0                                        # pa_semseg_confusion's `bins`: 1 forces the direct form (tools/painter_score_bench.py)
        self.palette = torch.from_numpy(pal).to(self.device)
        self.at, size = _layout(self._sections())
        self.out = torch.zeros(size, dtype=torch.uint8, device=self.device)
        self._last = None

    def _sections(self):
        return [("conf", np.int64, (self.k + 1) ** 2, 8), ("invalid", np.int64, 1, 8)]

    def reset(self):
        self.out.zero_()

    def add(self, pictures, gts):
        """pictures: painted pictures uint8 [H][W][3] of any sizes, gts: their label maps uint8 [H][W] (lists of numpy arrays or CUDA
        tensors).  ONE launch for the list, nothing is copied back."""
        pictures, gts = list(pictures), list(gts)
        if _device([pictures, gts], self.device) != self.device:
            raise RuntimeError("painter_engine: this SemsegScore lives on %s" % self.device)
        _same_sizes("SemsegScore.add", pictures, gts)
        if not pictures:
            return self
        pics = [_pictures(p, self.device) for p in pictures]
        maps = [_maps(g, self.device, torch.uint8) for g in gts]
        self._last = (pics, maps) + tuple(self._launch(pics, maps))          # what the enqueued launches read, until the next call
        return self

    def _launch(self, pics, maps):
        """The call of the library for one list -> what it reads besides the pictures and maps."""
        jobs = (ScoreJob * len(pics))()
        for job, p, g in zip(jobs, pics, maps):
            job.picture, job.gt, job.h, job.w = p.data_ptr(), g.data_ptr(), int(p.shape[0]), int(p.shape[1])
        total = sum(int(p.shape[0]) * int(p.shape[1]) for p in pics)
        host, table = _job_table(jobs, self.device)
        check(lib.pa_semseg_confusion(table.data_ptr(), len(pics), total, self.palette.data_ptr(), self.k, DIST_TYPES[self.dist_type],
                                      self.ignore_label, self.bins, self._ptr("conf"), self._ptr("invalid"), _stream()),
              "pa_semseg_confusion (%d jobs, %d pixels, %d colours)" % (len(pics), total, self.k))
        return host, table

    def _ptr(self, name):
        return self.out.data_ptr() + self.at[name][0]

    def _matrix(self, name):
        a = self.out.cpu().numpy()
        invalid = int(_section(a, self.at, "invalid")[0])
        if invalid > 0:
            raise ValueError("SemsegScore: %d ground-truth pixels hold a label >= %d that is not the ignore label %d"
                             % (invalid, self.k, self.ignore_label))
        return _section(a, self.at, name).reshape(self.k + 1, self.k + 1).copy()

    def matrix(self):
        """The one copy back (and synchronisation) -> int64 numpy [K + 1][K + 1], rows = predicted class, columns = ground truth with
        the ignored pixels in column K.  ValueError if a ground-truth value in [K, 255] other than the ignore label was met."""
        return self._matrix("conf")

    def scores(self):
        """`semseg_scores(self.matrix())`: mIoU, fwIoU, mACC, pACC, IoU and ACC per class, on the host in float64 -- detectron2's
        formulas restated, unverified against detectron2."""
        return semseg_scores(self.matrix())


class SemsegBoundaryScore(SemsegScore):
    """`SemsegScore` with the evaluators' boundary-IoU branch (ADE20kSemSegEvaluatorCustom.py:103-110, COCOPanoSemSegEvaluatorCustom.py:
    97-104): besides the confusion matrix, the joint histogram of `label_boundary` of the class map and of the ground truth (its ignore
    label replaced by K), both kept on the device (pa_semseg_boundary_confusion).  A pixel's class is evaluated once for both; the class
    maps never leave the device.  A picture's erosion count is `boundary_dilation(H, W, dilation_ratio)`.  K <= 254: detectron2 switches
    the branch off from 255 classes.  detectron2's _compute_boundary_iou restated from its published source, unverified against
    detectron2 / cv2 (tests/painter_boundary_host.py is the definition)."""

    def __init__(self, palette, dist_type="abs", ignore_label=255, dilation_ratio=0.02, device="cuda"):
        if len(palette) > 254:
            raise ValueError("SemsegBoundaryScore: %d classes -- detectron2 computes boundary IoU only for fewer than 255 classes (the "
                             "ignore label becomes class K in a uint8 map); use SemsegScore" % len(palette))
        self.dilation_ratio = _positive_ratio("SemsegBoundaryScore", dilation_ratio)
        self.workspace = None
        super().__init__(palette, dist_type, ignore_label, device)

    def _sections(self):
        return super()._sections() + [("bconf", np.int64, (self.k + 1) ** 2, 8)]

    def _launch(self, pics, maps):
        jobs = (BoundaryJob * len(pics))()
        for job, p, g in zip(jobs, pics, maps):
            job.picture, job.gt, job.h, job.w = p.data_ptr(), g.data_ptr(), int(p.shape[0]), int(p.shape[1])
            job.d = boundary_dilation(job.h, job.w, self.dilation_ratio)
        total = sum(int(p.shape[0]) * int(p.shape[1]) for p in pics)
        what = "pa_semseg_boundary_confusion (%d jobs, %d pixels, %d colours)" % (len(pics), total, self.k)
        if self.workspace is None or self.workspace.numel() < lib.pa_semseg_boundary_workspace_bytes(total):
            self.workspace = _workspace(lib.pa_semseg_boundary_workspace_bytes, (total,), what, self.device)
        host, table = _job_table(jobs, self.device)
        check(lib.pa_semseg_boundary_confusion(table.data_ptr(), len(pics), total, self.palette.data_ptr(), self.k,
                                               DIST_TYPES[self.dist_type], self.ignore_label, self.bins, self._ptr("conf"), self._ptr("bconf"),
                                               self._ptr("invalid"), self.workspace.data_ptr(), _stream()), what)
        return host, table

    def boundary_matrix(self):
        """As `matrix()`, of the boundary maps -> int64 numpy [K + 1][K + 1], rows = boundary value of the class map, columns = boundary
        value of the ground truth (0 = not on a boundary).  The same ValueError."""
        return self._matrix("bconf")

    def scores(self):
        """`semseg_scores(self.matrix(), self.boundary_matrix())`: the six numbers of `SemsegScore.scores`, BoundaryIoU and minIoU_BIoU."""
        return semseg_scores(self.matrix(), self.boundary_matrix())


def _crop_box(crop, h, w):
    if crop is None:
        return (0, h, 0, w)
    if isinstance(crop, str):
        if crop != "eigen":
            raise ValueError("painter_engine: crop is None, \"eigen\" or (y0, y1, x0, x1), not %r" % crop)
        if (h, w) != (480, 640):
            raise ValueError("painter_engine: the eigen crop %s belongs to 480 x 640 pictures, not %d x %d" % (EIGEN_CROP, h, w))
        return EIGEN_CROP
    y0, y1, x0, x1 = (int(v) for v in crop)
    if not (0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w):
        raise ValueError("painter_engine: the crop box %s leaves the %d x %d picture" % ((y0, y1, x0, x1), h, w))
    return (y0, y1, x0, x1)


class DepthErrors:
    """One launched pa_depth_errors over a list of (prediction, ground truth) device maps: `result()` is one copy back of ten doubles
    per picture and one synchronisation."""

    def __init__(self, preds, gts, min_depth=1e-3, max_depth=80.0, crop=None, divisor=1000.0):
        _same_sizes("depth_errors", preds, gts)
        self.n = len(preds)
        if not self.n:
            return
        dev = preds[0].device
        self.keep = (preds, gts)
        jobs = (DepthJob * self.n)()
        for job, p, g in zip(jobs, preds, gts):
            h, w = int(p.shape[0]), int(p.shape[1])
            job.pred, job.gt, job.h, job.w = p.data_ptr(), g.data_ptr(), h, w
            job.y0, job.y1, job.x0, job.x1 = _crop_box(crop, h, w)
        self._table_host, self.table = _job_table(jobs, dev)
        self.workspace = torch.empty(max(lib.pa_depth_workspace_bytes(self.n), 8), dtype=torch.uint8, device=dev)
        self.out = torch.empty((self.n, 10), dtype=torch.float64, device=dev)
        check(lib.pa_depth_errors(self.table.data_ptr(), self.n, float(divisor), float(min_depth), float(max_depth), self.out.data_ptr(),
                                  self.workspace.data_ptr(), _stream()),
              "pa_depth_errors (%d jobs, divisor %r, depths %r .. %r)" % (self.n, divisor, min_depth, max_depth))

    def sums(self):
        """The copy back -> float64 [n][10]: n, the three threshold counts, the six sums (include/painter_hip.h)."""
        return self.out.cpu().numpy() if self.n else np.zeros((0, 10))

    def result(self):
        return depth_metrics(self.sums())


def depth_metrics(sums):
    """float64 [n][10] of pa_depth_errors -> (float64 [n][9] in the order of compute_errors (eval_with_pngs.py:71): silog, log10,
    abs_rel, sq_rel, rmse, rmse_log, d1, d2, d3; int64 [n] valid pixels).  A picture without a valid pixel gives nine NaN, as the
    reference's mean of nothing does."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 10)
    n = s[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s[:, 1:] / n[:, None]
        d1, d2, d3, sq, lg2, abs_rel, sq_rel, err, l10 = mean.T
        silog = np.sqrt(lg2 - err ** 2) * 100
        out = np.stack([silog, l10, abs_rel, sq_rel, np.sqrt(sq), np.sqrt(lg2), d1, d2, d3], -1)
    return out, n.astype(np.int64)


def depth_errors(preds, gts, min_depth=1e-3, max_depth=80.0, crop=None, divisor=1000.0, device="cuda"):
    """nyuv2_depth/eval_with_pngs.py:148-217 (`eval`, dataset nyu) with compute_errors (:50-71) for a list of pictures in two launches.
    preds: int32 [H][W] depth pictures as `PainterEngine.run` returns them for `nyuv2_depth`; gts: uint16 [H][W], the values of the
    ground-truth PNG (numpy arrays or CUDA tensors, any sizes).  crop: None, "eigen" (the box 45:471, 41:601 of :205, 480 x 640 pictures
    only) or (y0, y1, x0, x1), half-open.  The float32 steps of the reference are float32, so n and d1 .. d3 are its own; the other six
    numbers come from float64 sums where the reference sums in float32.
    -> (float64 [n][9]: silog, log10, abs_rel, sq_rel, rmse, rmse_log, d1, d2, d3; int64 [n]: valid pixels); nine NaN where n = 0."""
    preds, gts = list(preds), list(gts)
    device = _device([preds, gts], device)
    return DepthErrors([_maps(p, device, torch.int32) for p in preds], [_maps(g, device, torch.uint16) for g in gts],
                       min_depth, max_depth, crop, divisor).result()


# ---- restoration scores (csrc/painter_restore.hip)
RESTORE_METRICS = ("skimage", "matlab_y")
RESTORE_DEFAULT_METRIC = {"lol": "skimage", "derain": "matlab_y", "sidd": None}      # what each task's own evaluation uses; sidd: see below
RESTORE_OUT = 8                                                                       # doubles per picture (include/painter_hip.h)


class RestoreJob(ctypes.Structure):
    """pa_restore_job of include/painter_hip.h."""
    _fields_ = [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


def _restore_setup(metric, data_range=2.0):
    """-> (mode, 1-D window weights float64, cov_norm, C1, C2) of a metric; ValueError for an unknown one.
    skimage: `structural_similarity`'s defaults -- 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance -- with `data_range`;
    matlab_y: SSIM_index of evaluate_PSNR_SSIM.m -- 11 x 11 Gaussian of sigma 1.5, normalised, L = 255 (`data_range` does not enter)."""
    if metric == "skimage":
        r = float(data_range)
        if not (r > 0 and np.isfinite(r)):
            raise ValueError("painter_engine: data_range must be positive and finite, not %r" % (data_range,))
        return 0, np.full(7, 1.0 / 7.0), 49.0 / 48.0, (0.01 * r) ** 2, (0.03 * r) ** 2
    if metric == "matlab_y":
        k = np.arange(11, dtype=np.float64) - 5.0
        g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
        return 1, g / g.sum(), 1.0, (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    raise ValueError("painter_engine: metric is one of %s, not %r" % (", ".join(RESTORE_METRICS), metric))


def _restore_sizes(who, sizes, gts, win):
    """sizes: (h, w) of every prediction; gts: their ground truths.  ValueError for a count or size mismatch, or a picture below the window."""
    if len(sizes) != len(gts):
        raise ValueError("%s: %d pictures, %d ground-truth pictures" % (who, len(sizes), len(gts)))
    for i, ((h, w), g) in enumerate(zip(sizes, gts)):
        if tuple(g.shape) != (h, w, 3):
            raise ValueError("%s: picture %d is %s, its ground truth %s" % (who, i, (h, w, 3), tuple(g.shape)))
        if h < win or w < win:
            raise ValueError("%s: picture %d (%d x %d) is smaller than the %d x %d window" % (who, i, h, w, win, win))


def _f64_pictures(x, device):
    """A float64 picture [H][W][3] (numpy or CUDA tensor) -> contiguous CUDA tensor on `device` (what `_device` returned)."""
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if x.device != device:
        raise RuntimeError("painter_engine: the pictures are on %s, expected %s" % (x.device, device))
    assert x.dtype == torch.float64 and x.dim() == 3 and x.shape[-1] == 3, (x.dtype, tuple(x.shape))
    return x.contiguous()


class RestorationScores:
    """One launched pa_restore_scores over a list of (prediction, ground truth) device pictures of any sizes: `sums()` is the one copy
    back (eight doubles per picture) and the one synchronisation.  preds: float64 [H][W][3] (metric "skimage") or uint8 [H][W][3]
    ("matlab_y") CUDA tensors, contiguous; gts: uint8 [H][W][3] CUDA tensors."""

    def __init__(self, preds, gts, metric, data_range=2.0):
        self.metric = metric
        mode, weights, cov_norm, c1, c2 = _restore_setup(metric, data_range)
        win = len(weights)
        _restore_sizes("restoration_scores", [tuple(p.shape[:2]) for p in preds], gts, win)
        self.n = len(preds)
        if not self.n:
            return
        want = torch.float64 if mode == 0 else torch.uint8
        assert all(p.dtype == want and p.is_cuda and p.is_contiguous() for p in preds), "painter_engine: %s scores %s pictures" % (metric, want)
        assert all(g.dtype == torch.uint8 and g.is_cuda and g.is_contiguous() for g in gts)
        dev = preds[0].device
        self.keep = (preds, gts)
        tile, ch = lib.pa_restore_tile(), 3 if mode == 0 else 1
        jobs = (RestoreJob * self.n)()
        tiles = 0
        for job, p, g in zip(jobs, preds, gts):
            job.pred, job.gt, job.h, job.w = p.data_ptr(), g.data_ptr(), int(p.shape[0]), int(p.shape[1])
            tiles += ch * (-(-(job.h - win + 1) // tile)) * (-(-(job.w - win + 1) // tile))
        nbytes = lib.pa_restore_workspace_bytes(self.n, tiles)
        if nbytes < 0:
            check(1, "pa_restore_scores (%d jobs, %d tiles)" % (self.n, tiles))
        # the library reads the table on the host and copies it on the stream: pinned, and kept until the next synchronisation
        self._table_host = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).pin_memory()
        self._weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty((self.n, RESTORE_OUT), dtype=torch.float64, device=dev)
        check(lib.pa_restore_scores(self._table_host.data_ptr(), self.n, mode, win, self._weights.ctypes.data, cov_norm, c1, c2,
                                    self.out.data_ptr(), self.workspace.data_ptr(), _stream()),
              "pa_restore_scores (%d jobs, %d tiles, metric %s)" % (self.n, tiles, metric))

    def sums(self):
        """The copy back -> float64 [n][8]: element count, squared sum, then (sum of S, windows) per channel (include/painter_hip.h)."""
        return self.out.cpu().numpy() if self.n else np.zeros((0, RESTORE_OUT))

    def result(self):
        return restoration_metrics(self.sums(), self.metric)


def restoration_metrics(sums, metric):
    """float64 [n][8] of pa_restore_scores -> dict(psnr float64 [n], ssim float64 [n]).  skimage: psnr = 10 log10(1 / mse) (data range 1:
    the clipped prediction is >= 0), ssim = the mean of the three channels' mean S; matlab_y: psnr = 20 log10(255 / sqrt(mse)), ssim = the
    mean S of the Y plane.  A perfect prediction gives inf and exactly 1.0."""
    _restore_setup(metric)
    s = np.asarray(sums, dtype=np.float64).reshape(-1, RESTORE_OUT)
    ch = 3 if metric == "skimage" else 1
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = s[:, 1] / s[:, 0]
        psnr = 10 * np.log10(1 / mse) if metric == "skimage" else 20 * np.log10(255 / np.sqrt(mse))
        ssim = sum(s[:, 2 + 2 * c] / s[:, 3 + 2 * c] for c in range(ch)) / ch
    return dict(psnr=psnr, ssim=ssim)


def restoration_scores(preds, gts, metric="skimage", data_range=2.0, device="cuda"):
    """PSNR and SSIM of restored pictures, per picture, in one copy of the job table and two launches for the whole list.

    metric "skimage": what painter_inference_lol.py:166-169 computes -- preds float64 [H][W][3] as `PainterEngine.run` returns them
    (clipped to [0, 1] on the device), gts uint8 [H][W][3] taken as gt / 255.; `peak_signal_noise_ratio` with data range 1 and
    `structural_similarity(multichannel=True)` with its defaults: 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, the map
    cropped by 3 pixels, the mean of the three channel means.  data_range defaults to 2.0: skimage takes it from the float dtype's range
    (-1, 1) when none is passed, and that is the release whose call signature (`multichannel=`) the reference uses; pass 1.0 for
    C1 = 0.01^2, C2 = 0.03^2.
    metric "matlab_y": derain's evaluate_PSNR_SSIM.m -- preds uint8 [H][W][3], the `saved` pictures of `run_restoration`; both pictures
    to Y (rgb2ycbcr's row in exact integers, rounded half up), PSNR of the Y planes at peak 255, SSIM_index with its 11 x 11 Gaussian.
    Both are restated from published sources and unverified against skimage / MATLAB, which are not available where this project is
    tested; tests/painter_restore_host.py is the definition and says what is and is not known.  This is NOT sidd's eval_sidd.m, which
    uses MATLAB's built-in ssim / psnr on single blocks.

    preds, gts: lists of numpy arrays or CUDA tensors, any sizes.  A picture smaller than the window is a ValueError.
    -> dict(psnr float64 [n], ssim float64 [n])."""
    preds, gts = list(preds), list(gts)
    device = _device([preds, gts], device)
    mode = _restore_setup(metric, data_range)[0]
    return RestorationScores([_f64_pictures(p, device) if mode == 0 else _pictures(p, device) for p in preds],
                             [_pictures(g, device) for g in gts], metric, data_range).result()


# ---- panoptic merge (csrc/painter_pano.hip)
SEGMENT = np.dtype([("id", np.int32), ("isthing", np.int32), ("category_id", np.int32), ("instance_id", np.int32), ("area", np.int32),
                    ("score", np.float32)])                                             # pa_pano_segment of include/painter_hip.h


@functools.lru_cache(maxsize=4)
def semantic_palette(num_colors=133, channelsep=7):
    """The colours the `coco_pano_semseg` targets are painted with, float32 [num_colors][3] (define_colors_by_mean_sep,
    data/coco_semseg/gen_color_coco_panoptic_segm.py:31-54): each channel steps down by 256 // channelsep, blue fastest."""
    sep, i = 256 // channelsep, np.arange(num_colors)
    pal = np.stack([255 - sep * (i // channelsep ** 2), 255 - sep * (i % channelsep ** 2 // channelsep), 255 - sep * (i % channelsep)], -1)
    assert pal.min() >= 0 and len({tuple(c) for c in pal.tolist()}) == len(pal)
    pal = pal.astype(np.float32)
    pal.setflags(write=False)                  # cached: every caller sees the same array
    return pal


def id2rgb(id_map):
    """panopticapi.utils.id2rgb for an integer map: [H][W] -> uint8 [H][W][3], r = id % 256, g = id // 256 % 256, b = id // 65536."""
    m = np.asarray(id_map).astype(np.int64)
    return np.stack([m % 256, m // 256 % 256, m // 65536], -1).astype(np.uint8)


def _host_array(values, dtype):
    """Scores / classes of supplied instances (list, numpy or a tensor on any device) -> flat numpy array."""
    return np.asarray(values.detach().cpu() if torch.is_tensor(values) else values).astype(dtype).ravel()


def _bit_masks(masks, h, w, device):
    """bool / uint8 [n][H][W] (numpy or CUDA tensor), bit masks uint32 [n][ceil(H W / 32)] (the `bits` of an InstanceDecode), or a list of
    COCO RLE dicts (size, counts; a detections JSON's segmentations, crowd ground truth: `rle_decode`) -> int32 CUDA tensor
    [max(n, 1)][words] in pa_inst_decode's bit layout, n.  device: what `_device` returned for the call; a mask tensor anywhere else is
    refused."""
    words = (h * w + 31) // 32
    if _is_rles(masks):
        if _rle_size(masks) != (h, w):
            raise ValueError("painter_engine: the RLE masks are %s, the picture %s" % (_rle_size(masks), (h, w)))
        return rle_decode(masks, device), len(masks)
    if torch.is_tensor(masks):
        if _device([masks]) != device:                               # a host or foreign address must never reach a kernel
            raise RuntimeError("painter_engine: the masks are on %s, the picture on %s" % (masks.device, device))
    else:
        masks = np.asarray(masks)
        if masks.dtype == np.uint32:
            assert masks.ndim == 2 and masks.shape[1] == words, masks.shape
            masks = np.ascontiguousarray(masks).view(np.int32)
        else:
            masks = np.ascontiguousarray(masks).view(np.uint8) if masks.dtype == bool else np.ascontiguousarray(masks, dtype=np.uint8)
        masks = torch.from_numpy(masks).to(device)
    n = int(masks.shape[0])
    if masks.dtype == torch.int32:
        assert masks.dim() == 2 and masks.shape[1] == words, tuple(masks.shape)
        return (masks.contiguous() if n else torch.zeros((1, words), dtype=torch.int32, device=device)), n
    assert masks.dtype in (torch.uint8, torch.bool) and tuple(masks.shape[1:]) == (h, w), (masks.dtype, tuple(masks.shape))
    bits = torch.zeros((max(n, 1), words), dtype=torch.int32, device=device)
    if n:
        check(lib.pa_pack_mask_bits(masks.contiguous().data_ptr(), n, h, w, bits.data_ptr(), _stream()), "pa_pack_mask_bits (%d masks)" % n)
    return bits, n


def classify_instances(semseg_picture, masks, palette=None, n_things=80, dist_type="abs", device="cuda"):
    """COCOPanopticEvaluatorCustom.merge_inst_semseg_result_to_instseg (COCOPanoEvaluatorCustom.py:259-276; the softmax of
    COCOInstSegEvaluatorCustom.py:169-186 does not change the argmax): the thing class whose colour the pixels of each mask are nearest
    to in sum, as exact integers, ties to the lower class, class 0 for an empty mask.  semseg_picture: the painted `coco_pano_semseg`
    picture, uint8 [H][W][3] (numpy or CUDA tensor); masks: bool / uint8 [n][H][W] (numpy or CUDA tensor) or the uint32 `bits` of an
    InstanceDecode -> int32 [n] numpy."""
    device = _device([semseg_picture, masks], device)
    _check_arguments("classify_instances", dict(dist_type=dist_type), MERGE_DEFAULTS)
    img = _pictures(semseg_picture, device)
    pal = _rgb_palette(palette, semantic_palette)
    h, w, k = int(img.shape[0]), int(img.shape[1]), int(pal.shape[0])
    bits, n = _bit_masks(masks, h, w, device)
    m = int(bits.shape[0])
    dpal = torch.from_numpy(pal).to(device)
    count = torch.tensor([n], dtype=torch.int32, device=device)
    sums = torch.empty((m, int(n_things)), dtype=torch.int64, device=device)
    classes = torch.empty(m, dtype=torch.int32, device=device)
    check(lib.pa_pano_vote(img.data_ptr(), dpal.data_ptr(), bits.data_ptr(), count.data_ptr(), h, w, k, int(n_things), DIST_TYPES[dist_type], m,
                           sums.data_ptr(), classes.data_ptr(), _stream()), "pa_pano_vote (sizes %s)" % ((h, w, k, n_things, m),))
    return classes.cpu().numpy()[:n]


class PanopticDecode:
    """One launched pa_pano_decode.  Behind an InstanceDecode (built with `tail=PanopticDecode.out_bytes(...)`) it reads the decode's
    count, scores and bit masks where the decode left them and writes into the tail of the decode's output buffer: `result()` is one copy
    back and one synchronisation for both.  With supplied instances (dict(masks=, scores=, classes=None)) it owns its output buffer."""

    @staticmethod
    def sections(h, w, k, n_things, max_inst):
        """The output buffer: count (a 16-byte slot), a segment per instance and stuff class, the instances' classes, the map, its id2rgb."""
        return [("count", np.int32, 1, 1), ("segments", SEGMENT, max_inst + k - n_things, 16), ("classes", np.int32, max_inst, 1),
                ("panoptic", np.int32, h * w, 1), ("rgb", np.uint8, 3 * h * w, 1)]

    @staticmethod
    def out_bytes(h, w, k, n_things, max_inst):
        return _layout(PanopticDecode.sections(h, w, k, n_things, max_inst))[1]

    def __init__(self, semseg_picture, decode=None, supplied=None, palette=None, n_things=80, dist_type="abs", overlap_threshold=0.5,
                 stuff_area_thresh=8192, instances_score_thresh=0.55):
        _check_arguments("PanopticDecode", dict(dist_type=dist_type), MERGE_DEFAULTS)
        assert (decode is None) != (supplied is None)
        dev = semseg_picture.device
        self.img = img = _pictures(semseg_picture, dev)
        pal = _rgb_palette(palette, semantic_palette)
        self.h, self.w, self.k, self.n_things = int(img.shape[0]), int(img.shape[1]), int(pal.shape[0]), int(n_things)
        self.decode, self.supplied = decode, supplied
        given = None
        if decode is not None:
            assert (decode.h, decode.w) == (self.h, self.w), "painter_engine: the two painted pictures differ in size"
            self.max_inst, self.out, self.base = decode.max_num, decode.out, decode.tail
            masks, scores, count = (decode.out.data_ptr() + o for o in (decode.obits, decode.o32, 0))
        else:
            self.bits, n = _bit_masks(supplied["masks"], self.h, self.w, dev)
            self.max_inst, self.base = int(self.bits.shape[0]), 0
            sc = np.zeros(self.max_inst, np.float32)
            sc[:n] = _host_array(supplied["scores"], np.float32)
            self.n, self.scores = n, torch.from_numpy(sc).to(dev)
            self.count = torch.tensor([n], dtype=torch.int32, device=dev)
            if supplied.get("classes") is not None:
                cl = np.zeros(self.max_inst, np.int32)
                cl[:n] = _host_array(supplied["classes"], np.int32)
                self.given = given = torch.from_numpy(cl).to(dev)
            masks, scores, count = self.bits.data_ptr(), self.scores.data_ptr(), self.count.data_ptr()
        shape = (self.h, self.w, self.k, self.n_things, self.max_inst)
        nbytes = lib.pa_pano_workspace_bytes(*shape)
        if nbytes < 0:
            check(1, "pa_pano_decode (sizes %s)" % (shape,))
        self.at, end = _layout(self.sections(*shape), self.base)
        if decode is None:
            self.out = torch.zeros(end, dtype=torch.uint8, device=dev)
        assert self.out.numel() >= end
        self.palette = torch.from_numpy(pal).to(dev, non_blocking=True)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ptr = lambda name: self.out.data_ptr() + self.at[name][0]
        check(lib.pa_pano_decode(img.data_ptr(), self.palette.data_ptr(), masks, scores, count, None if given is None else given.data_ptr(),
                                 *shape[:4], DIST_TYPES[dist_type], self.max_inst, float(overlap_threshold), float(stuff_area_thresh),
                                 float(instances_score_thresh), self.workspace.data_ptr(), ptr("panoptic"), ptr("rgb"), ptr("count"),
                                 ptr("segments"), ptr("classes"), _stream()), "pa_pano_decode")

    def result(self):
        """The copy back (and the one synchronisation) -> the dict `panoptic` documents."""
        a = self.out.cpu().numpy()
        if self.decode is not None:
            inst = self.decode.result(host=a)
            scores, masks, n = inst["scores"], inst["masks"], int(_section(a, self.decode.at, "count")[0])
        else:
            masks = self.supplied["masks"]                          # handed back as they came: no copy of what the caller has
            scores, n = _host_array(self.supplied["scores"], np.float32), self.n
        table = _section(a, self.at, "segments", int(_section(a, self.at, "count")[0]))
        segments = [dict(id=int(s["id"]), isthing=True, score=float(s["score"]), category_id=int(s["category_id"]),
                         instance_id=int(s["instance_id"])) if s["isthing"] else
                    dict(id=int(s["id"]), isthing=False, category_id=int(s["category_id"]), area=int(s["area"])) for s in table]
        classes = _section(a, self.at, "classes", n) if n else np.zeros(len(scores), np.int32)
        return dict(panoptic=_section(a, self.at, "panoptic").reshape(self.h, self.w), segments=segments, classes=classes, scores=scores,
                    masks=masks, rgb=_section(a, self.at, "rgb").reshape(self.h, self.w, 3), areas=table["area"].copy())


def _launch_panoptic(sem, inst, instances, semseg_palette, n_things, merge, instances_kw):
    """sem, inst: uint8 CUDA pictures (inst None with supplied instances) -> the launched PanopticDecode."""
    _check_arguments("panoptic", dict(instances_kw, **merge), INSTANCE_DEFAULTS, MERGE_DEFAULTS)
    if (inst is None) == (instances is None):
        raise TypeError("panoptic: give either the painted coco_pano_inst picture or instances=dict(masks=, scores=, classes=None)")
    dec = None
    if inst is not None:
        a = dict(INSTANCE_DEFAULTS, **instances_kw)
        k = len(_rgb_palette(semseg_palette, semantic_palette))
        tail = PanopticDecode.out_bytes(int(sem.shape[0]), int(sem.shape[1]), k, int(n_things), int(a["max_num"]))
        dec = InstanceDecode(inst, *a.values(), tail=tail)
    elif instances_kw:
        raise TypeError("panoptic: %s belong to the instance decode, which supplied instances skip" % sorted(instances_kw))
    return PanopticDecode(sem, dec, instances, semseg_palette, n_things, **merge)


def panoptic(semseg_picture, inst_picture=None, *, instances=None, semseg_palette=None, n_things=80, dist_type="abs", overlap_threshold=0.5,
             stuff_area_thresh=8192, instances_score_thresh=0.55, device="cuda", **instances_kw):
    """COCOPanopticEvaluatorCustom.merge_inst_semseg_result_to_panoseg (COCOPanoEvaluatorCustom.py:203-257) without its files: the
    semantic map of the painted `coco_pano_semseg` picture (nearest of the `semseg_palette` colours, default `semantic_palette()`), a
    class for every instance by vote (:259-276), then combine_semantic_and_instance_outputs_custom (:47-134).  The defaults are those of
    get_args_parser_pano_seg (:279-297).

    inst_picture: the painted `coco_pano_inst` picture; it is decoded as `instances(inst_picture, **instances_kw)` does and the merge is
    chained behind that decode on the device -- one output buffer, one copy back, one synchronisation.  Or instances = dict(masks= bool /
    uint8 [n][H][W] (numpy or a CUDA tensor on the picture's device) or a list of COCO RLE dicts (a detections JSON's segmentations,
    decoded on the device: `rle_decode`), scores= [n], classes= [n] or None (lists, numpy or tensors; they
    are read on the host)) for pre-computed instances (:229-248); given classes skip the vote.

    -> dict(panoptic int32 [H][W] (0 = unassigned), segments = list of dicts as the reference builds them (things: id, isthing, score,
    category_id, instance_id; stuff: id, isthing, category_id, area), areas int32 per segment (pixels that carry its id), classes int32
    [n], scores float32 [n], masks bool [n][H][W] (supplied masks: the caller's own object), rgb uint8 [H][W][3] = id2rgb(panoptic), what
    the evaluator encodes as PNG).  When the
    instance decode finds no candidate the instances are the reference's single zero mask with score 0 and class 0, which adds nothing."""
    device = _device([semseg_picture, inst_picture, (instances or {}).get("masks")], device)
    sem = _pictures(semseg_picture, device)
    inst = None if inst_picture is None else _pictures(inst_picture, device)
    merge = dict(dist_type=dist_type, overlap_threshold=overlap_threshold, stuff_area_thresh=stuff_area_thresh,
                 instances_score_thresh=instances_score_thresh)
    return _launch_panoptic(sem, inst, instances, semseg_palette, n_things, merge, instances_kw).result()


def run_panoptic(semseg_engine, inst_engine, pictures, sizes=None, **kw):
    """Two PainterEngines, one of task `coco_pano_semseg` and one of `coco_pano_inst`, each with its own prompt pair: forward and decode of
    both as `run`, then `panoptic(semantic picture, instance picture, **kw)` of every pair straight from the decode plans' device-resident
    uint8 outputs; the merges of a batch are all enqueued before the first copy back.  -> one dict per picture, as `panoptic` returns it."""
    if semseg_engine.task != "coco_pano_semseg" or inst_engine.task != "coco_pano_inst":
        raise ValueError("painter_engine: run_panoptic takes a coco_pano_semseg engine and a coco_pano_inst engine, not %r and %r"
                         % (semseg_engine.task, inst_engine.task))
    kw = {k: v for k, v in kw.items() if k != "device"}
    _check_arguments("panoptic", kw, INSTANCE_DEFAULTS, MERGE_DEFAULTS)          # before the first forward is enqueued
    merge = {k: kw.pop(k, v) for k, v in MERGE_DEFAULTS.items()}                 # kw keeps what belongs to the instance decode
    palette, n_things = merge.pop("semseg_palette"), merge.pop("n_things")

    def batch(pics, sizes):
        sem = semseg_engine._launch_batch(pics, sizes, False)
        jobs, step = [], inst_engine.batch_size
        for j in range(0, len(pics), step):
            inst = inst_engine._launch_batch(pics[j:j + step], sizes[j:j + step], False)
            jobs += [_launch_panoptic(sem.picture(j + i), inst.picture(i), None, palette, n_things, merge, kw) for i in range(inst.n_jobs)]
        return [j.result() for j in jobs]

    with _eval_mode(inst_engine.model):
        return [o for b in semseg_engine._run(pictures, sizes, batch) for o in b]


class PqJob(ctypes.Structure):
    """pa_pq_job of include/painter_hip.h."""
    _fields_ = [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("pred_segments", ctypes.c_void_p), ("gt_segments", ctypes.c_void_p),
                ("pred_count", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("gt_rgb", ctypes.c_int32),
                ("n_gt", ctypes.c_int32), ("g_cap", ctypes.c_int32), ("p_cap", ctypes.c_int32)]


GT_SEGMENT = np.dtype([("id", np.int32), ("category", np.int32), ("iscrowd", np.int32), ("area", np.int32), ("rank", np.int32),
                       ("reserved", np.int32)])                                         # pa_pq_gt_segment of include/painter_hip.h
PQ_MAX_GT, PQ_MAX_PRED = 254, 255                                                       # pa_pq_add's capacities
PQ_FLAGS = ("a non-zero predicted id that is not in its segment list", "a listed predicted segment without a pixel",
            "a category outside the %d classes", "union <= 0 (inconsistent annotation areas)",
            "a segment matched more than once (inconsistent annotation areas)", "a repeated or non-positive segment id")


def pq_averages(tp, fp, fn, iou, isthing, labels=None):
    """panopticapi's PQStat.pq_average over all categories, the things and the stuff, in Python floats: over the categories of a group
    with tp + fp + fn > 0, pq = iou / (tp + fp / 2 + fn / 2), sq = iou / tp (0 without a true positive), rq = tp / (tp + fp / 2 + fn / 2),
    the group's numbers their means (nan for a group without such a category, where panopticapi divides by zero).  -> dict with the
    keys detectron2's COCOPanopticEvaluator prints, x 100 (PQ SQ RQ PQ_th SQ_th RQ_th PQ_st SQ_st RQ_st), `per_class` = {label: dict(pq,
    sq, rq)} x 100 and `n` = dict(All, Things, Stuff), the categories averaged.  Restated from panopticapi's published source;
    panopticapi is not available where this project is tested, so the formulas are unverified against panopticapi."""
    k = len(tp)
    labels = list(range(k)) if labels is None else list(labels)
    rows = []
    for c in range(k):
        t, p, f, s = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        rows.append(None if t + p + f == 0 else (s / (t + 0.5 * p + 0.5 * f), s / t if t != 0 else 0, t / (t + 0.5 * p + 0.5 * f)))
    res = {}
    counts = {}
    for suffix, name, want in (("", "All", None), ("_th", "Things", True), ("_st", "Stuff", False)):
        pq = sq = rq = 0.0
        n = 0
        for c in range(k):
            if rows[c] is None or (want is not None and bool(isthing[c]) != want):
                continue
            n += 1
            pq, sq, rq = pq + rows[c][0], sq + rows[c][1], rq + rows[c][2]
        counts[name] = n
        for key, v in (("PQ", pq), ("SQ", sq), ("RQ", rq)):
            res[key + suffix] = 100 * (v / n) if n else float("nan")
    zero = (0.0, 0.0, 0.0)
    res["per_class"] = {labels[c]: dict(zip(("pq", "sq", "rq"), (100 * v for v in (rows[c] or zero)))) for c in range(k)}
    res["n"] = counts
    return res


class PanopticQuality:
    """PQ of a data set, kept on the device (pa_pq_add, csrc/painter_pq.hip): panopticapi's pq_compute_single_core per picture -- the
    joint histogram of (ground-truth segment, predicted segment), the match at IoU > 0.5, false negatives, false positives with the
    VOID / crowd rule -- and the sums of PQStat.  Per `add` three launches for the whole list; nothing is copied back before `counts()` /
    `result()`: 4 x n_classes numbers and a flag word per picture.  tests/painter_pq_host.py is the definition; it is restated from
    panopticapi's published source and unverified against panopticapi.

    Categories are indices 0 .. n_classes - 1, things first (isthing = index < n_things), which is what `panoptic` reports.  categories=
    [dict(id=, isthing=), ...] instead names the data set's own ids: `category_id`s of `add` are then mapped through it on the host
    (an id it does not hold refuses the picture) and `per_class` is keyed by them; the segments of `add_decodes` come from the device
    and stay indices into that list.  RLE / COCOeval, splitting over cores and PNG / JSON I/O are not here."""

    def __init__(self, n_classes=133, n_things=80, device="cuda", categories=None):
        self.device = _device((), device)
        if categories is not None:
            n_classes = len(categories)
            self.labels = [c["id"] for c in categories]
            self.isthing = [bool(c["isthing"]) for c in categories]
            self.index = {label: i for i, label in enumerate(self.labels)}
            assert len(self.index) == n_classes, "PanopticQuality: a category id is listed twice"
        else:
            self.labels, self.index = list(range(int(n_classes))), None
            self.isthing = [c < int(n_things) for c in range(int(n_classes))]
        self.k = int(n_classes)
        if not 1 <= self.k <= 1024:
            raise ValueError("PanopticQuality: %d classes (1 .. 1024)" % self.k)
        self.bins = 0                                        # pa_pq_add's `bins`: 1 forces the direct form (tools/painter_pq_bench.py)
        self.min_caps = (1, 1)                               # capacities (G_cap, P_cap) a call has at least (tests, measurements)
        self.at, size = _layout([("tp", np.int64, self.k, 8), ("fp", np.int64, self.k, 8), ("fn", np.int64, self.k, 8),
                                 ("iou", np.float64, self.k, 8)])
        self.out = torch.zeros(size, dtype=torch.uint8, device=self.device)
        self._flags, self._last = [], None

    def reset(self):
        self.out.zero_()
        self._flags, self._last = [], None

    def _category(self, c):
        return int(c) if self.index is None else self.index.get(c, -1)

    def _gt_table(self, segments):
        """dicts(id, category_id, iscrowd, area) -> GT_SEGMENT records in ascending id order; rank = position in the list."""
        t = np.zeros(len(segments), GT_SEGMENT)
        for rank, s in enumerate(segments):
            area = s.get("area")
            t[rank] = (int(s["id"]), self._category(s["category_id"]), int(bool(s.get("iscrowd", 0))), -1 if area is None else int(area), rank, 0)
        return t[np.argsort(t["id"], kind="stable")]

    def _pred_table(self, segments):
        t = np.zeros(len(segments), SEGMENT)
        for i, s in enumerate(segments):
            t[i]["id"], t[i]["category_id"] = int(s["id"]), self._category(s["category_id"])
        return t[np.argsort(t["id"], kind="stable")]

    def _add(self, preds, gts, gt_segments, keep):
        """preds: per picture (address of the int32 map, h, w, predicted table as SEGMENT records or its device address, address of the
        device count or None, capacity of the table).  Tables, counts and the job table go up in ONE pinned copy."""
        n = len(preds)
        if not (n == len(gts) == len(gt_segments)):
            raise ValueError("PanopticQuality: %d predictions, %d ground-truth maps, %d ground-truth segment lists" % (n, len(gts), len(gt_segments)))
        if n == 0:
            return self
        if _device([[g for g in gts]], self.device) != self.device:
            raise RuntimeError("painter_engine: this PanopticQuality lives on %s" % self.device)
        maps = [_pictures(g, self.device) if g.ndim == 3 else _maps(g if torch.is_tensor(g) else np.ascontiguousarray(g, dtype=np.int32),
                                                                     self.device, torch.int32) for g in gts]
        for i, (p, g) in enumerate(zip(preds, maps)):
            if (p[1], p[2]) != tuple(g.shape[:2]):
                raise ValueError("PanopticQuality: prediction %d is %s, its ground truth %s" % (i, (p[1], p[2]), tuple(g.shape[:2])))
        gtabs = [self._gt_table(s) for s in gt_segments]
        g_cap = max([self.min_caps[0]] + [len(t) for t in gtabs])
        p_cap = max([self.min_caps[1]] + [p[5] for p in preds])
        if g_cap > PQ_MAX_GT or p_cap > PQ_MAX_PRED:
            raise ValueError("PanopticQuality: %d ground-truth / %d predicted segments in a picture (at most %d / %d)"
                             % (g_cap, p_cap, PQ_MAX_GT, PQ_MAX_PRED))
        sections = [("jobs", np.uint8, ctypes.sizeof(PqJob) * n, 16)]
        for i, (p, t) in enumerate(zip(preds, gtabs)):
            sections += [("gt%d" % i, GT_SEGMENT, len(t), 8), ("pred%d" % i, SEGMENT, 0 if p[4] is not None else len(p[3]), 8),
                         ("count%d" % i, np.int32, 0 if p[4] is not None else 1, 4)]
        up = _Upload(sections, self.device)
        jobs = (PqJob * n)()
        for i, (job, p, g, t) in enumerate(zip(jobs, preds, maps, gtabs)):
            job.pred, job.h, job.w, job.gt, job.gt_rgb = p[0], p[1], p[2], g.data_ptr(), int(g.dim() == 3)
            job.gt_segments, job.n_gt, job.g_cap, job.p_cap = up.put("gt%d" % i, t), len(t), len(t), p[5]
            if p[4] is not None:
                job.pred_segments, job.pred_count = p[3], p[4]
            else:
                job.pred_segments, job.pred_count = up.put("pred%d" % i, p[3]), up.put("count%d" % i, [len(p[3])])
        shape = (n, g_cap, p_cap, self.k)
        what = "pa_pq_add (sizes %s)" % (shape,)
        sent = up.send(jobs)
        workspace = _workspace(lib.pa_pq_workspace_bytes, shape, what, self.device)
        flags = torch.empty(n, dtype=torch.int32, device=self.device)
        ptr = lambda name: self.out.data_ptr() + self.at[name][0]
        check(lib.pa_pq_add(sent, n, max(p[1] * p[2] for p in preds), g_cap, p_cap, self.k, self.bins, ptr("tp"), ptr("fp"), ptr("fn"),
                            ptr("iou"), flags.data_ptr(), workspace.data_ptr(), _stream()), what)
        self._flags.append(flags)
        self._last = (keep, maps, up.host, up.dev, workspace)      # what the enqueued launches read, until the next call
        return self

    def add(self, preds, pred_segments, gts, gt_segments):
        """preds: panoptic maps int32 [H][W] of any sizes, 0 = VOID (numpy arrays or CUDA tensors); pred_segments: per picture the list of
        dicts `panoptic` returns (id and category_id are read); gts: the annotation PNGs as uint8 [H][W][3] or as int32 [H][W] = r + 256 g +
        65536 b; gt_segments: per picture the annotation's `segments_info` (id, category_id, iscrowd, area; area None = count it from
        the map).  Nothing is copied back.  -> self."""
        preds, pred_segments = list(preds), list(pred_segments)
        if len(preds) != len(pred_segments):
            raise ValueError("PanopticQuality.add: %d maps, %d segment lists" % (len(preds), len(pred_segments)))
        if _device([preds], self.device) != self.device:
            raise RuntimeError("painter_engine: this PanopticQuality lives on %s" % self.device)
        maps = [_maps(p if torch.is_tensor(p) else np.ascontiguousarray(p, dtype=np.int32), self.device, torch.int32) for p in preds]
        tables = [self._pred_table(s) for s in pred_segments]
        return self._add([(m.data_ptr(), int(m.shape[0]), int(m.shape[1]), t, None, len(t)) for m, t in zip(maps, tables)], list(gts),
                         list(gt_segments), maps)

    def add_decodes(self, decodes, gts, gt_segments):
        """decodes: launched PanopticDecodes (`_launch_panoptic`); map, segment table and count are read where each decode left them, so
        neither has to be copied back first.  Their categories are the semantic palette's indices.  -> self."""
        decodes = list(decodes)
        srcs = []
        for d in decodes:
            if d.out.device != self.device:
                raise RuntimeError("painter_engine: this PanopticQuality lives on %s" % self.device)
            at = lambda name: d.out.data_ptr() + d.at[name][0]
            srcs.append((at("panoptic"), d.h, d.w, at("segments"), at("count"), d.max_inst + d.k - d.n_things))
        return self._add(srcs, list(gts), list(gt_segments), decodes)

    def counts(self):
        """The one copy back (and synchronisation), with the flag words -> tp, fp, fn int64 [n_classes], iou float64 [n_classes] (numpy).
        ValueError names the first refused picture (counted over all `add` calls since `reset`) and why."""
        a = torch.cat([self.out] + [f.view(torch.uint8) for f in self._flags]).cpu().numpy()
        _refuse("PanopticQuality", a[self.out.numel():].view(np.uint32), PQ_FLAGS, self.k, rest="pictures are refused and add nothing")
        return tuple(_section(a, self.at, name).copy() for name in ("tp", "fp", "fn", "iou"))

    def result(self):
        """`pq_averages` of `counts()`: PQ, SQ, RQ over all categories, things (`_th`) and stuff (`_st`) in percent, `per_class` and `n`
        -- on the host in Python floats; panopticapi's formulas restated, unverified against panopticapi."""
        return pq_averages(*self.counts(), self.isthing, self.labels)


def run_panoptic_quality(semseg_engine, inst_engine, pictures, gts, gt_segments, score, sizes=None, **kw):
    """`run_panoptic`'s loop ending in `score.add_decodes` (a PanopticQuality) instead of `result()`: the panoptic maps, their segment
    tables and the byte masks are never copied back, and nothing else is before `score.counts()` / `score.result()`.  gts, gt_segments:
    per picture the annotation (see PanopticQuality.add), of the painted picture's size (sizes[i], default the query's own).  -> score."""
    if semseg_engine.task != "coco_pano_semseg" or inst_engine.task != "coco_pano_inst":
        raise ValueError("painter_engine: run_panoptic_quality takes a coco_pano_semseg engine and a coco_pano_inst engine, not %r and %r"
                         % (semseg_engine.task, inst_engine.task))
    kw = {k: v for k, v in kw.items() if k != "device"}
    _check_arguments("panoptic", kw, INSTANCE_DEFAULTS, MERGE_DEFAULTS)          # before the first forward is enqueued
    merge = {k: kw.pop(k, v) for k, v in MERGE_DEFAULTS.items()}                 # kw keeps what belongs to the instance decode
    palette, n_things = merge.pop("semseg_palette"), merge.pop("n_things")
    pictures, gts, gt_segments = list(pictures), list(gts), list(gt_segments)
    sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
    if not (len(pictures) == len(gts) == len(gt_segments) == len(sizes)):
        raise ValueError("run_panoptic_quality: %d pictures, %d ground-truth maps, %d segment lists" % (len(pictures), len(gts), len(gt_segments)))
    for i, ((w, h), g) in enumerate(zip(sizes, gts)):
        if (h, w) != tuple(g.shape[:2]):
            raise ValueError("run_panoptic_quality: picture %d is %s, its ground truth %s" % (i, (h, w), tuple(g.shape[:2])))

    def batch(items, sizes):
        pics = [p for p, _, _ in items]
        sem = semseg_engine._launch_batch(pics, sizes, False)
        jobs, step = [], inst_engine.batch_size
        for j in range(0, len(pics), step):
            inst = inst_engine._launch_batch(pics[j:j + step], sizes[j:j + step], False)
            jobs += [_launch_panoptic(sem.picture(j + i), inst.picture(i), None, palette, n_things, merge, kw) for i in range(inst.n_jobs)]
        score.add_decodes(jobs, [g for _, g, _ in items], [s for _, _, s in items])

    with _eval_mode(inst_engine.model):
        semseg_engine._run(list(zip(pictures, gts, gt_segments)), sizes, batch)
    return score


# ---- COCO instance mask AP (csrc/painter_ap.hip)
class ApJob(ctypes.Structure):
    """pa_ap_job of include/painter_hip.h."""
    _fields_ = [("det_masks", ctypes.c_void_p), ("det_scores", ctypes.c_void_p), ("det_classes", ctypes.c_void_p),
                ("det_count", ctypes.c_void_p), ("gt_masks", ctypes.c_void_p), ("gt_table", ctypes.c_void_p), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("n_gt", ctypes.c_int32), ("d_cap", ctypes.c_int32), ("empty_as_one", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


AP_GT = np.dtype([("category", np.int32), ("iscrowd", np.int32), ("area", np.float64)])        # pa_ap_gt of include/painter_hip.h
AP_RECORD = np.dtype([("score", np.float32), ("area", np.int32), ("category", np.int32), ("index", np.int32), ("matched", np.uint64, (2,)),
                      ("ignored", np.uint64, (2,))])                                             # pa_ap_record
AP_MODES = ("agnostic", "per_class")                                                             # COCOeval's useCats = 0 / 1; bit i of `modes`
AP_MAX_DET = AP_MAX_GT = 128                                                                     # pa_ap_add's capacities
AP_AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))                  # COCOeval's all / small / medium / large
AP_FLAGS = ("a NaN score", "a detection class outside the %d classes", "a ground-truth class outside the %d classes")


def _ap_mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def _coco_accumulate(pictures, npig, T, rec_thrs, max_dets, precision, recall):
    """COCOeval.accumulate for one class (or pseudo-class).  pictures: per picture (scores, matched words, ignored words) of its records in
    evaluation order, bit a * T + t of a word = area range a, threshold t; npig: per area range the ground truths that count.  Fills
    precision [T][R][A][M] and recall [T][A][M] (views of the caller's tables) wherever npig > 0: the records cut to the first m of
    max_dets, concatenated in picture order, stable-sorted by descending score; running tp / fp counts; precision made monotone from the
    right and read at the first position whose recall reaches each of rec_thrs."""
    for a, n_gt in enumerate(npig):
        if n_gt == 0:
            continue
        shift = np.arange(a * T, a * T + T, dtype=np.uint64)[:, None]
        for m, max_det in enumerate(max_dets):
            cat = lambda i, dtype: np.concatenate([p[i][:max_det] for p in pictures]) if pictures else np.zeros(0, dtype)
            order = np.argsort(-cat(0, np.float32), kind="mergesort")
            dtm, ign = ((cat(i, np.uint64)[order][None] >> shift) & np.uint64(1) != 0 for i in (1, 2))
            tp = np.cumsum(dtm & ~ign, axis=1).astype(np.float64)
            fp = np.cumsum(~dtm & ~ign, axis=1).astype(np.float64)
            nd = tp.shape[1]
            for t in range(T):
                rc = tp[t] / n_gt
                pr = tp[t] / (fp[t] + tp[t] + np.spacing(1))
                recall[t, a, m] = rc[-1] if nd else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                at = np.searchsorted(rc, rec_thrs, side="left")
                q = np.zeros(len(rec_thrs))
                q[at < nd] = pr[at[at < nd]]
                precision[t, :, a, m] = q


def instance_ap_metrics(records, gt_annotations, n_classes=80, mode="agnostic", iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100),
                        area_ranges=None):
    """COCOeval.accumulate and .summarize (iouType "segm") on the records of `InstanceAP.records()`, on the host in float64.  records: per
    picture its AP_RECORDs in sorted order; gt_annotations: per picture dicts(category_id = class index, iscrowd, area = a number) -- the
    ground truths' ignore flags and their count depend on the annotations alone.  Per class (one pseudo-class in "agnostic" mode), area
    range and m of max_dets: every picture's records (of the class) cut to the first m, concatenated in picture order, stable-sorted by
    descending score; tp / fp = running counts of matched / unmatched records that are not ignored; recall = tp / npig, precision = tp /
    (fp + tp + np.spacing(1)) made monotone from the right and read at the first position whose recall reaches each of rec_thrs.  ->
    dict(AP, AP50, AP75, APs, APm, APl at max_dets[-1]; AR<m> per m; ARs, ARm, ARl; precision [T][R][K][A][M], recall [T][K][A][M], -1 where
    no ground truth counts; `per_class` AP in "per_class" mode).  Means are over the entries > -1, -1.0 without any.  Restated from
    pycocotools' published source; pycocotools is not available where this project is tested, so it is unverified against pycocotools."""
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    rec_thrs = np.linspace(0, 1, 101) if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    area_ranges = AP_AREA_RANGES if area_ranges is None else area_ranges
    mi = AP_MODES.index(mode)
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_ranges), len(max_dets)
    K = int(n_classes) if mode == "per_class" else 1
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    gcls = [np.array([int(g["category_id"]) for g in anns], np.int64) for anns in gt_annotations]
    crowd = [np.array([bool(g.get("iscrowd", 0)) for g in anns], bool) for anns in gt_annotations]
    area = [np.array([float(g["area"]) for g in anns], np.float64) for anns in gt_annotations]
    for k in range(K):
        recs = [r[r["category"] == k] for r in records] if mode == "per_class" else list(records)
        mine = [c == k for c in gcls] if mode == "per_class" else [np.ones(len(c), bool) for c in gcls]
        npig = [sum(int((m & ~(c | (v < lo) | (v > hi))).sum()) for m, c, v in zip(mine, crowd, area)) for lo, hi in area_ranges]
        _coco_accumulate([(r["score"], r["matched"][:, mi], r["ignored"][:, mi]) for r in recs], npig, T, rec_thrs, max_dets,
                         precision[:, :, k], recall[:, k])
    at = lambda v: np.flatnonzero(iou_thrs == v)
    res = dict(AP=_ap_mean(precision[:, :, :, 0, -1]), AP50=_ap_mean(precision[at(.5), :, :, 0, -1]),
               AP75=_ap_mean(precision[at(.75), :, :, 0, -1]))
    for a, name in enumerate("sml", 1):
        res["AP" + name] = _ap_mean(precision[:, :, :, a, -1]) if a < A else -1.0
    for m, max_det in enumerate(max_dets):
        res["AR%d" % max_det] = _ap_mean(recall[:, :, 0, m])
    for a, name in enumerate("sml", 1):
        res["AR" + name] = _ap_mean(recall[:, :, a, -1]) if a < A else -1.0
    res.update(precision=precision, recall=recall)
    if mode == "per_class":
        res["per_class"] = [_ap_mean(precision[:, :, k, 0, -1]) for k in range(K)]
    return res


class InstanceAP:
    """COCO instance mask AP of a data set (pa_ap_add, csrc/painter_ap.hip): COCOeval's computeIoU and evaluateImg per picture on the
    device -- intersections of bit masks, the IoU doubles, the greedy matching per (mode, area range, threshold) -- and its accumulate /
    summarize on the host (`instance_ap_metrics`).  Per `add` one clear and three launches for the whole list; nothing is copied back
    before `records()` / `result()`: 48 bytes per detection slot, 4 per ground-truth slot and two words per picture.
    tests/painter_ap_host.py is the definition; it is restated from pycocotools' published source and unverified against pycocotools.

    modes: "agnostic" (useCats = 0, COCOCAInstSegEvaluatorCustom.py:404-414) and / or "per_class" (useCats = 1,
    COCOInstSegEvaluatorCustom.py:315-329).  Classes are indices 0 .. n_classes - 1; categories = [ids] (or dicts with `id`) names the data
    set's own ids instead: `category_id`s and classes handed to `add` are mapped through it on the host (an id it does not hold refuses
    the picture), the classes of `add_decodes` come from the device and stay indices.  At most 128 detections and 128 ground truths per
    picture, len(area_ranges) * len(iou_thrs) <= 64.  Masks may be lists of COCO RLE dicts (`rle_decode`).  Polygon decoding, box AP, the class-wise re-NMS route and JSON I/O are not here."""

    def __init__(self, n_classes=80, modes=("agnostic",), iou_thrs=None, area_ranges=None, max_dets=(1, 10, 100), categories=None,
                 device="cuda"):
        self.device = _device((), device)
        self.index = None
        if categories is not None:
            labels = [c["id"] if isinstance(c, dict) else c for c in categories]
            n_classes, self.index = len(labels), {label: i for i, label in enumerate(labels)}
            assert len(self.index) == n_classes, "InstanceAP: a category id is listed twice"
        self.labels = list(range(int(n_classes))) if categories is None else labels
        self.k = int(n_classes)
        self.modes = tuple(modes)
        if not self.modes or any(m not in AP_MODES for m in self.modes):
            raise ValueError("InstanceAP: modes %r (of %s)" % (modes, ", ".join(AP_MODES)))
        self.iou_thrs, self.area_ranges, self.max_dets, ok = _coco_params(iou_thrs, AP_AREA_RANGES if area_ranges is None else area_ranges, max_dets)
        if not 1 <= self.k <= 1024 or not ok:
            raise ValueError("InstanceAP: %d classes (1 .. 1024), %d thresholds x %d area ranges (at most 64 together)"
                             % (self.k, len(self.iou_thrs), len(self.area_ranges)))
        self.min_caps = (1, 1)                               # capacities (d_cap, g_cap) a call has at least (tests, measurements)
        self.params = torch.from_numpy(np.concatenate([self.iou_thrs, self.area_ranges.ravel()])).to(self.device)
        self.reset()

    def reset(self):
        self._outs, self._annotations, self._last, self._records = [], [], None, None

    def _category(self, c):
        return int(c) if self.index is None else self.index.get(c, -1)

    def _add(self, dets, gt_masks, gt_annotations, keep):
        """dets: per picture (h, w, capacity of its buffers, addresses of bit masks / scores / classes / count on the device or None,
        host scores, host classes or None, empty_as_one).  Tables, host scores, counts and the job table go up in ONE pinned copy."""
        n = len(dets)
        if not (n == len(gt_masks) == len(gt_annotations)):
            raise ValueError("InstanceAP: %d pictures of detections, %d of ground-truth masks, %d annotation lists" % (n, len(gt_masks), len(gt_annotations)))
        if n == 0:
            return self
        if _device([list(gt_masks)], self.device) != self.device:
            raise RuntimeError("painter_engine: this InstanceAP lives on %s" % self.device)
        gbits, tables = [], []
        for i, (d, g, anns) in enumerate(zip(dets, gt_masks, gt_annotations)):
            if _is_rles(g):                                  # RLE ground truth (crowd annotations): decoded on the device by _bit_masks
                if _rle_size(g) != (d[0], d[1]):
                    raise ValueError("InstanceAP: the detections of picture %d are %s, its ground truth %s" % (i, (d[0], d[1]), _rle_size(g)))
            else:
                if not torch.is_tensor(g):
                    g = np.asarray(g)
                if g.ndim == 3 and len(g) and tuple(g.shape[1:]) != (d[0], d[1]):
                    raise ValueError("InstanceAP: the detections of picture %d are %s, its ground truth %s" % (i, (d[0], d[1]), tuple(g.shape[1:])))
                if len(g) == 0:
                    g = np.zeros((0, d[0], d[1]), bool)
            bits, n_gt = _bit_masks(g, d[0], d[1], self.device)
            if n_gt != len(anns):
                raise ValueError("InstanceAP: picture %d has %d ground-truth masks and %d annotations" % (i, n_gt, len(anns)))
            t = np.zeros(n_gt, AP_GT)
            for j, a in enumerate(anns):
                t[j] = (self._category(a["category_id"]), int(bool(a.get("iscrowd", 0))), -1.0 if a.get("area") is None else float(a["area"]))
            gbits.append(bits)
            tables.append(t)
        d_cap = max([self.min_caps[0]] + [d[2] for d in dets])
        g_cap = max([self.min_caps[1]] + [len(t) for t in tables])
        if d_cap > AP_MAX_DET or g_cap > AP_MAX_GT:
            raise ValueError("InstanceAP: %d detections / %d ground truths in a picture (at most %d / %d)" % (d_cap, g_cap, AP_MAX_DET, AP_MAX_GT))
        sections = [("jobs", np.uint8, ctypes.sizeof(ApJob) * n, 16)]
        for i, (d, t) in enumerate(zip(dets, tables)):
            own = d[3] is None                               # scores, classes and count come from the host
            sections += [("gt%d" % i, AP_GT, len(t), 8), ("scores%d" % i, np.float32, d[2] if own else 0, 4),
                         ("classes%d" % i, np.int32, d[2] if own and d[5] is not None else 0, 4), ("count%d" % i, np.int32, int(own), 4)]
        up = _Upload(sections, self.device)
        jobs = (ApJob * n)()
        for i, (job, d, g, t) in enumerate(zip(jobs, dets, gbits, tables)):
            job.h, job.w, job.d_cap, job.empty_as_one = d[0], d[1], d[2], int(d[6])
            job.gt_masks, job.gt_table, job.n_gt = g.data_ptr(), up.put("gt%d" % i, t), len(t)
            if d[3] is not None:
                job.det_masks, job.det_scores, job.det_classes, job.det_count = d[3]
            else:
                job.det_masks, job.det_scores, job.det_count = d[7].data_ptr(), up.put("scores%d" % i, d[4]), up.put("count%d" % i, [len(d[4])])
                if d[5] is not None:
                    job.det_classes = up.put("classes%d" % i, d[5])
        shape = (n, d_cap, g_cap)
        what = "pa_ap_add (sizes %s)" % (shape,)
        sent = up.send(jobs)
        workspace = _workspace(lib.pa_ap_workspace_bytes, shape, what, self.device)
        oat, osize = _layout([("records", AP_RECORD, n * d_cap, 8), ("counts", np.int32, n, 4), ("flags", np.uint32, n, 4),
                              ("gpix", np.uint32, n * g_cap, 4)])
        out = torch.zeros(osize, dtype=torch.uint8, device=self.device)
        ptr = lambda name: out.data_ptr() + oat[name][0]
        modes = sum(1 << AP_MODES.index(m) for m in set(self.modes))
        T, A = len(self.iou_thrs), len(self.area_ranges)
        check(lib.pa_ap_add(sent, n, max((d[0] * d[1] + 31) // 32 for d in dets), d_cap, g_cap, self.k, modes, self.params.data_ptr(), T,
                            self.params.data_ptr() + 8 * T, A, ptr("records"), ptr("counts"), ptr("flags"), workspace.data_ptr(), _stream()), what)
        off = lib.pa_ap_workspace_offset(*shape, 2)
        out[oat["gpix"][0]:oat["gpix"][0] + 4 * n * g_cap].copy_(workspace[off:off + 4 * n * g_cap])       # the areas of `area: None`
        self._outs.append((out, oat, shape))
        self._annotations += [[dict(category_id=int(r["category"]), iscrowd=int(r["iscrowd"]), area=float(r["area"])) for r in t] for t in tables]
        self._last = (keep, gbits, up.host, up.dev, workspace)     # what the enqueued launches read, until the next call
        self._records = None
        return self

    def add(self, masks, scores, classes, gt_masks, gt_annotations, sizes=None):
        """Lists with one entry per picture.  masks: bool / uint8 [n][H][W] (numpy or CUDA tensor) or uint32 bit masks [n][ceil(H W / 32)]
        (then the size is that of the ground-truth masks, or sizes[i] = (H, W) where both sides are bit masks); scores: [n]; classes: [n] or None (class 0, "agnostic" only); classes may also
        be None as a whole.  gt_masks: likewise [G][H][W], or per picture a list of RLE dicts (size, counts: crowd ground truth as COCO
        stores it; also accepted for `masks`); gt_annotations: per picture dicts(category_id, iscrowd, area; area None = the
        mask's pixel count).  Detections are taken as they are handed over: a picture without any has none (the reference's single empty
        detection is what `instances` returns for such a picture).  Nothing is copied back.  -> self."""
        masks, scores, gt_masks, gt_annotations = list(masks), list(scores), list(gt_masks), list(gt_annotations)
        classes = [None] * len(masks) if classes is None else list(classes)
        if not (len(masks) == len(scores) == len(classes)):
            raise ValueError("InstanceAP.add: %d mask lists, %d score lists, %d class lists" % (len(masks), len(scores), len(classes)))
        if len(masks) != len(gt_masks):
            raise ValueError("InstanceAP.add: %d pictures of detections, %d of ground-truth masks" % (len(masks), len(gt_masks)))
        if _device([masks], self.device) != self.device:
            raise RuntimeError("painter_engine: this InstanceAP lives on %s" % self.device)
        dets = []
        for i, (m, s, c, g) in enumerate(zip(masks, scores, classes, gt_masks)):
            if c is None and "per_class" in self.modes:
                raise ValueError("InstanceAP.add: picture %d has no classes, which mode \"per_class\" needs" % i)
            shape = next((tuple(int(v) for v in x.shape[1:]) for x in (m, g) if hasattr(x, "shape") and len(x.shape) == 3), None)
            shape = next((_rle_size(x) for x in (m, g) if _is_rles(x)), None) if shape is None else shape
            shape = shape if sizes is None else (int(sizes[i][0]), int(sizes[i][1]))
            if shape is None:
                raise ValueError("InstanceAP.add: picture %d gives bit masks on both sides, so its size is unknown" % i)
            if not torch.is_tensor(m) and len(m) == 0:
                m = np.zeros((0,) + shape, bool)
            bits, count = _bit_masks(m, shape[0], shape[1], self.device)
            s = _host_array(s, np.float32)
            c = None if c is None else np.array([self._category(v) for v in _host_array(c, np.int64).tolist()], np.int32)
            if len(s) != count or (c is not None and len(c) != count):
                raise ValueError("InstanceAP.add: picture %d has %d masks, %d scores, %s classes" % (i, count, len(s), "no" if c is None else len(c)))
            dets.append((shape[0], shape[1], int(bits.shape[0]), None, s, c, False, bits))
        return self._add(dets, gt_masks, gt_annotations, [d[7] for d in dets])

    def add_decodes(self, decodes, gt_masks, gt_annotations):
        """decodes: launched InstanceDecodes (classes null: "agnostic" only) or PanopticDecodes built on one (`_launch_panoptic` with the
        painted instance picture; the classes are those its vote wrote).  Bit masks, scores and count are read where the decode left them;
        a decode whose count is 0 scores as the reference's single empty detection.  The decode's own `result()` is untouched.  -> self."""
        dets, decodes = [], list(decodes)
        for i, d in enumerate(decodes):
            inst = d if isinstance(d, InstanceDecode) else getattr(d, "decode", None)
            if inst is None:
                raise TypeError("InstanceAP.add_decodes: entry %d is neither an InstanceDecode nor a PanopticDecode chained behind one" % i)
            if inst.out.device != self.device:
                raise RuntimeError("painter_engine: this InstanceAP lives on %s" % self.device)
            if inst is d and "per_class" in self.modes:
                raise ValueError("InstanceAP.add_decodes: an InstanceDecode has no classes, which mode \"per_class\" needs")
            base = inst.out.data_ptr()
            classes = None if inst is d else d.out.data_ptr() + d.at["classes"][0]
            dets.append((inst.h, inst.w, inst.max_num, (base + inst.obits, base + inst.o32, classes, base + inst.at["count"][0]), None, None, True))
        return self._add(dets, list(gt_masks), list(gt_annotations), decodes)

    def records(self):
        """The one copy back (and synchronisation) -> per picture its AP_RECORDs in sorted order (numpy).  ValueError names the first
        refused picture (counted over all `add` calls since `reset`) and why."""
        if self._records is None:
            a = torch.cat([o for o, _, _ in self._outs]).cpu().numpy() if self._outs else np.zeros(0, np.uint8)
            recs, flags, areas, base = [], [], [], 0
            for out, oat, (n, d_cap, g_cap) in self._outs:
                part = a[base:base + out.numel()]
                base += out.numel()
                table, counts = _section(part, oat, "records").reshape(n, d_cap), _section(part, oat, "counts")
                recs += [table[i, :counts[i]].copy() for i in range(n)]
                flags += _section(part, oat, "flags").tolist()
                areas += [row for row in _section(part, oat, "gpix").reshape(n, g_cap)]
            _refuse("InstanceAP", flags, AP_FLAGS, self.k)
            anns = [[dict(g, area=float(pix[j])) if g["area"] < 0 else g for j, g in enumerate(p)] for p, pix in zip(self._annotations, areas)]
            self._records = (recs, anns)
        return self._records[0]

    def result(self):
        """`instance_ap_metrics` of `records()` per mode -> {mode: dict(AP, AP50, AP75, APs, APm, APl, AR<m>..., ARs, ARm, ARl, precision,
        recall[, per_class])} -- accumulate and summarize on the host; COCOeval's formulas restated, unverified against pycocotools."""
        recs = self.records()
        return {mode: instance_ap_metrics(recs, self._records[1], self.k, mode, self.iou_thrs, None, self.max_dets,
                                          [tuple(r) for r in self.area_ranges.tolist()]) for mode in self.modes}


def run_instance_ap(inst_engine, pictures, gt_masks, gt_annotations, score, sizes=None, semseg_engine=None, **kw):
    """`run_instances`' loop ending in `score.add_decodes` (an InstanceAP) instead of `result()`: forward, instance decode and scoring are
    chained per batch, the masks are never copied back and nothing else is before `score.records()` / `score.result()`.  With
    `semseg_engine` (task coco_pano_semseg) the loop is `run_panoptic`'s: every instance gets the class the panoptic decode's vote gives it
    and "per_class" is allowed.  gt_masks, gt_annotations: per picture (see InstanceAP.add), of the painted picture's size (sizes[i],
    default the query's own).  -> score."""
    if inst_engine.task != "coco_pano_inst" or (semseg_engine is not None and semseg_engine.task != "coco_pano_semseg"):
        raise ValueError("painter_engine: run_instance_ap takes a coco_pano_inst engine and, optionally, a coco_pano_semseg engine, not %r and %r"
                         % (inst_engine.task, None if semseg_engine is None else semseg_engine.task))
    if semseg_engine is None and "per_class" in score.modes:
        raise ValueError("painter_engine: run_instance_ap scores mode \"per_class\" only with a semseg_engine, which gives the instances their classes")
    kw = {k: v for k, v in kw.items() if k != "device"}
    if semseg_engine is None:
        _check_arguments("run_instance_ap", kw, INSTANCE_DEFAULTS)               # before the first forward is enqueued
        args = dict(INSTANCE_DEFAULTS, **kw)
    else:
        _check_arguments("run_instance_ap", kw, INSTANCE_DEFAULTS, MERGE_DEFAULTS)
        merge = {k: kw.pop(k, v) for k, v in MERGE_DEFAULTS.items()}             # kw keeps what belongs to the instance decode
        palette, n_things = merge.pop("semseg_palette"), merge.pop("n_things")
    pictures, gt_masks, gt_annotations = list(pictures), list(gt_masks), list(gt_annotations)
    sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
    if not (len(pictures) == len(gt_masks) == len(gt_annotations) == len(sizes)):
        raise ValueError("run_instance_ap: %d pictures, %d lists of ground-truth masks, %d annotation lists, %d sizes"
                         % (len(pictures), len(gt_masks), len(gt_annotations), len(sizes)))

    def batch(items, sizes):
        pics, step = [p for p, _, _ in items], inst_engine.batch_size
        sem = None if semseg_engine is None else semseg_engine._launch_batch(pics, sizes, False)
        jobs = []
        for j in range(0, len(pics), step):
            inst = inst_engine._launch_batch(pics[j:j + step], sizes[j:j + step], False)
            if sem is None:
                jobs += [InstanceDecode(inst.picture(i), *args.values()) for i in range(inst.n_jobs)]
            else:
                jobs += [_launch_panoptic(sem.picture(j + i), inst.picture(i), None, palette, n_things, merge, kw) for i in range(inst.n_jobs)]
        score.add_decodes(jobs, [g for _, g, _ in items], [a for _, _, a in items])

    first = inst_engine if semseg_engine is None else semseg_engine
    with _eval_mode(inst_engine.model):
        first._run(list(zip(pictures, gt_masks, gt_annotations)), sizes, batch)
    return score


# ---- COCO keypoint AP (csrc/painter_kpt.hip)
# ---- COCO RLE (csrc/painter_rle.hip, include/painter_rle.h)
RLE_HEADER = np.dtype([("runs", np.int64), ("chars", np.int64), ("overflow", np.int64), ("count", np.int64)])       # pa_rle_header
RLE_RECORD = np.dtype([("char_offset", np.int64), ("char_count", np.int64), ("runs", np.uint32), ("area", np.uint32),
                       ("bbox", np.int32, (4,))])                                                                   # pa_rle_record
RLE_FLAGS = ("", "the counts do not sum to h * w", "a count is negative after the delta", "the string ends inside a value",
             "a value has more than 7 groups", "more runs than the workspace was sized for", "the span lies outside the pool",
             "a byte outside '0' .. 'o'")                                                        # pa_rle_decode's flag values 1 .. 7
RLE_CHARS_PER_COLUMN = 16          # default pool: 16 characters per column and mask slot (+ 64) -- about five runs of two or three
                                   # characters per column; an instance blob has two.  More than that takes the second launch.


def rle_default_chars(w, n_cap):
    return int(n_cap) * (RLE_CHARS_PER_COLUMN * int(w) + 64)


def _address(x):
    return x.data_ptr() if torch.is_tensor(x) else int(x)


class RleEncode:
    """One launched pa_rle_encode: bit masks in pa_inst_decode's layout -> COCO RLE strings, areas and boxes (maskApi.c's rleEncode,
    rleToString, rleArea, rleToBbox; tests/painter_rle_host.py is the definition, restated from pycocotools' published source and
    unverified against pycocotools).  bits, count: CUDA tensors, or device addresses inside a buffer `keep` holds (the `bits` and
    `count` sections of an InstanceDecode: the encode then chains behind the decode with no synchronisation).  `result()` copies back
    header + records and then pool[:total]; if the header reports that the strings did not fit the pool (default:
    `rle_default_chars`), it launches once more with the exact total it just read -- there is no failure mode and no host encode."""

    def __init__(self, bits, count, h, w, n_cap, char_cap=None, device=None, keep=None):
        self.keep = (bits, count, keep)
        self.device = _device([bits, count], device if device is not None else "cuda")
        self.bits, self.count = _address(bits), _address(count)
        self.h, self.w, self.n_cap = int(h), int(w), int(n_cap)
        self.char_cap = rle_default_chars(self.w, self.n_cap) if char_cap is None else int(char_cap)
        self.launches = 0
        self.workspace = _workspace(lib.pa_rle_encode_workspace_bytes, (self.h, self.w, self.n_cap),
                                    "pa_rle_encode (sizes %s)" % ((self.h, self.w, self.n_cap),), self.device)
        self._launch()

    def _launch(self):
        # ONE byte buffer: header, records, pool (at least one byte, so that its address is never null)
        self.at, size = _layout([("header", RLE_HEADER, 1, 8), ("records", RLE_RECORD, self.n_cap, 8), ("pool", np.uint8, max(self.char_cap, 1), 16)])
        self.out = torch.empty(size, dtype=torch.uint8, device=self.device)
        ptr = lambda name: self.out.data_ptr() + self.at[name][0]
        check(lib.pa_rle_encode(self.bits, self.count, self.h, self.w, self.n_cap, self.workspace.data_ptr(), self.char_cap, ptr("header"),
                                ptr("records"), ptr("pool"), _stream()), "pa_rle_encode")
        self.launches += 1

    def _head(self):
        end = self.at["records"][0] + RLE_RECORD.itemsize * self.n_cap
        a = self.out[:end].cpu().numpy()
        return a, _section(a, self.at, "header")[0]

    def result(self):
        """-> dict(header, records RLE_RECORD [count], pool uint8 [total characters], strings: one str per mask)."""
        a, header = self._head()
        if header["overflow"]:
            self.char_cap = int(header["chars"])
            self._launch()
            a, header = self._head()
            assert not header["overflow"]
        n, total = int(header["count"]), int(header["chars"])
        records = _section(a, self.at, "records", n)
        o = self.at["pool"][0]
        pool = self.out[o:o + total].cpu().numpy()
        text = pool.tobytes().decode("ascii")
        strings = [text[int(r["char_offset"]):int(r["char_offset"] + r["char_count"])] for r in records]
        return dict(header=header, records=records, pool=pool, strings=strings)


def _is_rles(x):
    """A non-empty list of COCO RLE dicts (size, counts)?"""
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(r, dict) and "counts" in r and "size" in r for r in x)


def _rle_size(rles):
    sizes = {(int(r["size"][0]), int(r["size"][1])) for r in rles}
    if len(sizes) != 1:
        raise ValueError("painter_engine: the RLE masks of one call have one size, not %s" % sorted(sizes))
    return sizes.pop()


def rle_encode(masks, size=None, device="cuda"):
    """pycocotools.mask.encode on the device.  masks: bool / uint8 [n][H][W] (numpy or CUDA tensor), or bit masks uint32 / int32
    [n][ceil(H W / 32)] with size = (H, W) -> (rles, areas, bboxes): a list of {"size": [h, w], "counts": str}, int64 [n], float64 [n][4]
    (x, y, w, h; zeros for an empty mask)."""
    device = _device([masks], device)
    masks = masks if torch.is_tensor(masks) else np.asarray(masks)
    if size is None:
        assert len(masks.shape) == 3, "rle_encode: bit masks need size=(H, W)"
        size = masks.shape[1:]
    h, w = int(size[0]), int(size[1])
    bits, n = _bit_masks(masks, h, w, device)
    count = torch.tensor([n], dtype=torch.int32, device=device)
    res = RleEncode(bits, count, h, w, int(bits.shape[0])).result()
    rles = [{"size": [h, w], "counts": s} for s in res["strings"]]
    return rles, res["records"]["area"].astype(np.int64), res["records"]["bbox"].astype(np.float64).reshape(n, 4)


def _launch_rle_decode(rles, h, w, compressed, device):
    n = len(rles)
    if compressed:
        parts = [r["counts"].encode("ascii") if isinstance(r["counts"], str) else bytes(r["counts"]) for r in rles]
        pool = np.frombuffer(b"".join(parts), np.uint8)
    else:
        parts = [np.asarray(r["counts"], dtype=np.int64).ravel() for r in rles]
        if any(len(p) and (p.min() < 0 or p.max() >= 1 << 32) for p in parts):
            raise ValueError("rle_decode: uncompressed counts are integers 0 .. 2^32 - 1")
        pool = np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.uint32)
    lengths = np.array([len(p) for p in parts], np.int64)
    spans = np.stack([np.cumsum(lengths) - lengths, lengths], 1)
    total = int(lengths.sum())
    dpool = torch.zeros(max(total, 1), dtype=torch.uint8 if compressed else torch.int32, device=device)
    if total:
        dpool[:total].copy_(torch.from_numpy(pool.copy() if compressed else pool.view(np.int32)))
    dspans = torch.from_numpy(np.ascontiguousarray(spans)).to(device)
    shape = (n, h, w, total)
    what = "pa_rle_decode (sizes %s)" % (shape,)
    workspace = _workspace(lib.pa_rle_decode_workspace_bytes, shape, what, device)
    bits = torch.empty((n, (h * w + 31) // 32), dtype=torch.int32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    check(lib.pa_rle_decode(dpool.data_ptr(), int(compressed), dspans.data_ptr(), n, h, w, total, total, workspace.data_ptr(), bits.data_ptr(),
                            flags.data_ptr(), _stream()), what)
    return bits, flags, (dpool, dspans, workspace)


def rle_decode(rles, device="cuda"):
    """pycocotools.mask.decode on the device, into bit masks.  rles: dicts {"size": [h, w], "counts": ...} of one size, counts a str /
    bytes (compressed) or a list of ints (uncompressed, COCO's crowd annotations) -> int32 CUDA tensor [n][ceil(h w / 32)] in
    pa_inst_decode's bit layout.  A malformed mask raises ValueError naming the mask and its flag (include/painter_rle.h)."""
    device = _device((), device)
    rles = list(rles)
    if not _is_rles(rles):
        raise ValueError("rle_decode: a non-empty list of dicts with `size` and `counts`")
    h, w = _rle_size(rles)
    kinds = np.array([isinstance(r["counts"], (str, bytes, bytearray)) for r in rles])
    if kinds.all() or not kinds.any():
        bits, flags, _ = _launch_rle_decode(rles, h, w, bool(kinds[0]), device)
        flags = flags.cpu().numpy()
    else:                                                                   # both kinds in one list: one launch each
        bits = torch.empty((len(rles), (h * w + 31) // 32), dtype=torch.int32, device=device)
        flags = np.zeros(len(rles), np.int32)
        for kind in (True, False):
            idx = np.flatnonzero(kinds == kind)
            part, f, _ = _launch_rle_decode([rles[i] for i in idx], h, w, kind, device)
            bits[torch.from_numpy(idx).to(device)] = part
            flags[idx] = f.cpu().numpy()
    _refuse("rle_decode", (1 << flags.astype(np.int64)) * (flags != 0), RLE_FLAGS, name=lambda i: "mask %d" % i,
            rest="masks are refused and decode to nothing")
    return bits


class InstanceResults:
    """The entries `instances_to_coco_json` builds for one picture (detectron2's function, restated from its published source and
    unverified), behind a launched InstanceDecode or a PanopticDecode chained behind one: the RLE encode reads bit masks and count where
    the decode left them; `result()` copies back the prefix of the decode's buffer before its `bits` section (count, scores), the classes
    of a PanopticDecode and the RLE buffer -- never `masks`."""

    def __init__(self, decode, image_id):
        if isinstance(decode, MinmaxDecode):             # bits sized by the count (read back once); the encode reads both where they lie
            self.decode, self.inst, self.image_id = decode, decode, image_id
            bits, n = decode.bits()
            self.encode = RleEncode(bits, decode.ptr("count"), decode.h, decode.w, n, device=decode.out.device, keep=decode.out)
            return
        inst = decode if isinstance(decode, InstanceDecode) else getattr(decode, "decode", None)
        if inst is None:
            raise TypeError("instance_results: neither an InstanceDecode, a MinmaxDecode nor a PanopticDecode chained behind one")
        self.decode, self.inst, self.image_id = decode, inst, image_id
        base = inst.out.data_ptr()
        self.encode = RleEncode(base + inst.obits, base + inst.at["count"][0], inst.h, inst.w, inst.max_num, device=inst.out.device, keep=inst.out)

    def result(self):
        inst = self.inst
        if isinstance(inst, MinmaxDecode):
            o, n = inst.at["records"][0], inst.count()
            rec = inst.out[o:o + MINMAX_RECORD.itemsize * n].cpu().numpy().view(MINMAX_RECORD)
            strings = self.encode.result()["strings"]
            return [dict(image_id=self.image_id, category_id=int(c), bbox=[0.0, 0.0, 0.0, 0.0], score=float(s),
                         segmentation={"size": [inst.h, inst.w], "counts": t}) for c, s, t in zip(rec["cls"], rec["score"], strings)]
        a = inst.out[:inst.obits].cpu().numpy()
        n = int(_section(a, inst.at, "count")[0])
        if n == 0:            # :302-310: one all-zero mask, score 0, label 0.  Slot 0 of the decode's bits is zero then: encode it as one mask
            one = torch.ones(1, dtype=torch.int32, device=inst.out.device)
            strings = RleEncode(inst.out.data_ptr() + inst.obits, one, inst.h, inst.w, 1, device=inst.out.device, keep=inst.out).result()["strings"]
            scores, classes = [0.0], [0]
        else:
            strings = self.encode.result()["strings"]
            scores = [float(s) for s in _section(a, inst.at, "scores", n)]
            if inst is self.decode:
                classes = [1] * n
            else:
                off = self.decode.at["classes"][0]
                classes = self.decode.out[off:off + 4 * n].cpu().numpy().view(np.int32).tolist()
        return [dict(image_id=self.image_id, category_id=int(c), bbox=[0.0, 0.0, 0.0, 0.0], score=s,
                     segmentation={"size": [inst.h, inst.w], "counts": t}) for c, s, t in zip(classes, scores, strings)]


def instance_results(decode, image_id):
    """The list `instances_to_coco_json` builds from the evaluators' Instances (COCOCAInstSegEvaluatorCustom.py:147; detectron2's
    function is restated from its published source and unverified), one entry per instance of a launched InstanceDecode or of a
    PanopticDecode chained behind one: image_id; category_id = the voted class behind a PanopticDecode, otherwise the label 1, and 0 for
    the empty-prediction mask; bbox = [0.0] * 4, for the evaluators set zero boxes (:246, :350); score = the Python float of the float32;
    segmentation = {"size": [h, w], "counts": str}, pycocotools.mask.encode's RLE computed on the device (`RleEncode`).  A decode without
    candidates gives the reference's single entry (:302-310): score 0, category 0, the all-zero mask (counts of [h w]).  A MinmaxDecode
    gives one entry per instance in ascending palette row, category_id = its class (0 for the background instance, :220-223)."""
    return InstanceResults(decode, image_id).result()


def run_instance_results(inst_engine, pictures, image_ids, sizes=None, semseg_engine=None, **kw):
    """`run_instance_ap`'s loop ending in `instance_results`: forwards, decodes and RLE encodes of a batch are all enqueued before the
    first copy back, and no mask is copied back.  With `semseg_engine` (task coco_pano_semseg) every instance carries the class the
    panoptic decode's vote gives it.  -> the flat list the evaluator `json.dumps` into coco_instances_results.json.  post_type="minmax":
    the decodes are `MinmaxDecode`s (keyword `palette` only, no semseg_engine); their masks and encodes follow once the counts are back."""
    if inst_engine.task != "coco_pano_inst" or (semseg_engine is not None and semseg_engine.task != "coco_pano_semseg"):
        raise ValueError("painter_engine: run_instance_results takes a coco_pano_inst engine and, optionally, a coco_pano_semseg engine, not %r and %r"
                         % (inst_engine.task, None if semseg_engine is None else semseg_engine.task))
    kw = {k: v for k, v in kw.items() if k != "device"}
    minmax = _post_type("run_instance_results", kw, semseg_engine) == "minmax"
    if minmax:
        args = dict(MINMAX_DEFAULTS, **kw)
    elif semseg_engine is None:
        _check_arguments("run_instance_results", kw, INSTANCE_DEFAULTS)         # before the first forward is enqueued
        args = dict(INSTANCE_DEFAULTS, **kw)
    else:
        _check_arguments("run_instance_results", kw, INSTANCE_DEFAULTS, MERGE_DEFAULTS)
        merge = {k: kw.pop(k, v) for k, v in MERGE_DEFAULTS.items()}             # kw keeps what belongs to the instance decode
        palette, n_things = merge.pop("semseg_palette"), merge.pop("n_things")
    pictures, image_ids = list(pictures), list(image_ids)
    sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
    if not (len(pictures) == len(image_ids) == len(sizes)):
        raise ValueError("run_instance_results: %d pictures, %d image ids, %d sizes" % (len(pictures), len(image_ids), len(sizes)))

    def batch(items, sizes):
        pics, step = [p for p, _ in items], inst_engine.batch_size
        sem = None if semseg_engine is None else semseg_engine._launch_batch(pics, sizes, False)
        jobs = []
        for j in range(0, len(pics), step):
            inst = inst_engine._launch_batch(pics[j:j + step], sizes[j:j + step], False)
            for i in range(inst.n_jobs):
                dec = MinmaxDecode(inst.picture(i), *args.values()) if minmax else InstanceDecode(inst.picture(i), *args.values()) if sem is None else \
                    _launch_panoptic(sem.picture(j + i), inst.picture(i), None, palette, n_things, merge, kw)
                jobs.append((dec, items[j + i][1]) if minmax else InstanceResults(dec, items[j + i][1]))
        if minmax:               # every decode of the batch is enqueued; the masks and the encodes are sized by the counts read back now
            jobs = [InstanceResults(dec, image_id) for dec, image_id in jobs]
        return [e for job in jobs for e in job.result()]

    first = inst_engine if semseg_engine is None else semseg_engine
    with _eval_mode(inst_engine.model):
        return [e for b in first._run(list(zip(pictures, image_ids)), sizes, batch) for e in b]


class KptJob(ctypes.Structure):
    """pa_kpt_job of include/painter_hip.h."""
    _fields_ = [("rows", ctypes.c_void_p), ("gt_keypoints", ctypes.c_void_p), ("gt_table", ctypes.c_void_p), ("n_box", ctypes.c_int32),
                ("n_gt", ctypes.c_int32)]


KPT_GT = np.dtype([("area", np.float64), ("bbox", np.float64, (4,)), ("iscrowd", np.int32), ("num_keypoints", np.int32)])      # pa_kpt_gt
KPT_RECORD = np.dtype([("score", np.float32), ("row", np.int32), ("area", np.float64), ("matched", np.uint64), ("ignored", np.uint64)])
# configs/_base_/coco.py:178-181
COCO_SIGMAS = (0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087, 0.087, 0.089, 0.089)
KPT_AREA_RANGES = ((0, 1e10), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))                    # COCOeval's all / medium / large for keypoints
KPT_MAX_BOX, KPT_MAX_GT, KPT_MAX_EVAL, KPT_MAX_JOBS = 1024, 128, 64, 65535               # pa_kpt_evaluate's capacities
KPT_FLAGS = ("a NaN among its poses, scores or box areas", "a ground truth whose area + 2^-52 is not a positive finite number",
             "a row outside the pose table")


def _kpt_ignore(g):
    return bool(g.get("iscrowd", 0)) or int(g["num_keypoints"]) == 0


def keypoint_ap_metrics(records, ground_truth, iou_thrs=None, rec_thrs=None, area_ranges=None, max_dets=(20,)):
    """COCOeval.accumulate and .summarize (iouType "keypoints", the one category `person`) on the records of `KeypointAP.records()`, on
    the host in float64.  records: {image id: KPT_RECORDs in evaluation order}; ground_truth: {image id: annotation dicts} -- the ground
    truths' ignore flags (iscrowd, num_keypoints == 0, area outside the range) and their count depend on the annotations alone.  Photos in
    ascending image id; the rest is `instance_ap_metrics`' arithmetic.  -> dict(AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl at
    max_dets[-1]; precision [T][R][1][A][M], recall [T][1][A][M], -1 where no ground truth counts).  Means are over the entries > -1, -1.0
    without any.  Restated from xtcocotools' published source; xtcocotools is not available where this project is tested, so it is
    unverified against xtcocotools."""
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    rec_thrs = np.linspace(0, 1, 101) if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    area_ranges = KPT_AREA_RANGES if area_ranges is None else area_ranges
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_ranges), len(max_dets)
    precision, recall = -np.ones((T, R, 1, A, M)), -np.ones((T, 1, A, M))
    images = sorted(ground_truth)
    skip = [np.array([_kpt_ignore(g) for g in ground_truth[i]], bool) for i in images]
    area = [np.array([float(g["area"]) for g in ground_truth[i]], np.float64) for i in images]
    recs = [records[i] for i in images]
    npig = [sum(int((~(s | (v < lo) | (v > hi))).sum()) for s, v in zip(skip, area)) for lo, hi in area_ranges]
    _coco_accumulate([(r["score"], r["matched"], r["ignored"]) for r in recs], npig, T, rec_thrs, max_dets, precision[:, :, 0], recall[:, 0])
    at = lambda v: np.flatnonzero(iou_thrs == v)
    res = {}
    for name, table in (("AP", precision), ("AR", recall)):
        res[name] = _ap_mean(table[..., 0, -1])
        res[name + "50"] = _ap_mean(table[at(.5)][..., 0, -1])
        res[name + "75"] = _ap_mean(table[at(.75)][..., 0, -1])
        for a, size in enumerate("ml", 1):
            res[name + size] = _ap_mean(table[..., a, -1]) if a < A else -1.0
    res.update(precision=precision, recall=recall)
    return res


class KeypointAP:
    """COCO keypoint AP of a data set (pa_kpt_poses, pa_kpt_evaluate; csrc/painter_kpt.hip): what TopDownCocoDatasetCustom.evaluate
    (mmpose_custom/data/topdown_coco_dataset.py:194-315) does with the decoded boxes -- photo coordinates, rescoring, de-duplication, OKS NMS
    per photo (configs/coco_256x192_test_offline.py:100-106) -- and COCOeval's computeOks and evaluateImg per photo on the device, its
    accumulate / summarize on the host (`keypoint_ap_metrics`).  `add` / `add_decodes` launch pa_kpt_poses per chunk and keep the poses on
    the device; nothing is copied back before `records()` / `result()`: 32 bytes per evaluated detection and three words per photo.
    tests/painter_kpt_host.py is the definition; mmpose's oks_nms and xtcocotools' COCOeval are restated there from their published source,
    unverified against mmpose / xtcocotools.

    ground_truth: {image id: [COCO annotation dicts with keypoints (K * 3), area, bbox, iscrowd, num_keypoints]}; every photo of the data
    set is listed, also one without a person.  The NMS order is descending score with equal scores to the higher bbox_id
    (argsort(kind="stable")[::-1]); the reference's `scores.argsort()[::-1]` agrees up to 16 boxes per photo, above that numpy's default
    sort leaves ties unspecified.  At most 1024 boxes and 128 ground truths per photo, K <= 32, len(area_ranges) * len(iou_thrs) <= 64,
    max(max_dets) <= 64.  soft_nms, rle_score and the JSON file are not here."""

    def __init__(self, ground_truth, sigmas=COCO_SIGMAS, vis_thr=0.2, oks_thr=0.9, use_nms=True, iou_thrs=None, area_ranges=None,
                 max_dets=(20,), heatmap_size=(192, 256), device="cuda"):
        self.device = _device((), device)
        self.sigmas = np.array(sigmas, np.float64).ravel()
        self.k = len(self.sigmas)
        self.vis_thr, self.oks_thr, self.use_nms = float(vis_thr), float(oks_thr), bool(use_nms)
        self.iou_thrs, self.area_ranges, self.max_dets, ok = _coco_params(iou_thrs, KPT_AREA_RANGES if area_ranges is None else area_ranges, max_dets)
        self.heatmap_size = (int(heatmap_size[0]), int(heatmap_size[1]))
        if not 1 <= self.k <= 32 or not ok or not 1 <= max(self.max_dets) <= KPT_MAX_EVAL or min(self.heatmap_size) < 1 or not self.oks_thr >= 0:
            raise ValueError("KeypointAP: %d keypoints (1 .. 32), %d thresholds x %d area ranges (at most 64 together), max_dets %s (1 .. %d), "
                             "heat map %s, oks_thr %s (>= 0)" % (self.k, len(self.iou_thrs), len(self.area_ranges), self.max_dets, KPT_MAX_EVAL,
                                                                self.heatmap_size, oks_thr))
        self.ground_truth = {image: list(anns) for image, anns in ground_truth.items()}
        self._gt = {}
        for image, anns in self.ground_truth.items():
            kp = np.array([g["keypoints"] for g in anns], np.float64).reshape(len(anns), self.k, 3)
            table = np.zeros(len(anns), KPT_GT)
            for j, g in enumerate(anns):
                table[j] = (float(g["area"]), tuple(float(v) for v in g["bbox"]), int(bool(g.get("iscrowd", 0))), int(g["num_keypoints"]))
            if len(anns) > KPT_MAX_GT:
                raise ValueError("KeypointAP: photo %r has %d ground truths (at most %d)" % (image, len(anns), KPT_MAX_GT))
            self._gt[image] = (kp, table)
        self.min_caps = (1, 1)                               # capacities (d_cap, g_cap) a call has at least (tests, measurements)
        self.params = torch.from_numpy(np.concatenate([self.sigmas, self.iou_thrs, self.area_ranges.ravel()])).to(self.device)
        self.reset()

    def reset(self):
        """Forgets every box added so far."""
        self._chunks, self._images, self._bbox_ids, self._records, self._last = [], [], [], None, None
        return self

    def _ids(self, n, image_ids, bbox_ids):
        image_ids = list(image_ids)
        bbox_ids = list(range(len(self._images), len(self._images) + n)) if bbox_ids is None else [int(b) for b in bbox_ids]
        if not (len(image_ids) == len(bbox_ids) == n):
            raise ValueError("KeypointAP: %d boxes, %d image ids, %d bbox ids" % (n, len(image_ids), len(bbox_ids)))
        return image_ids, bbox_ids

    def _boxes(self, n, centers, scales, box_scores):
        c, s, b = (_host_array(x, np.float32) for x in (centers, scales, box_scores))
        if c.size != 2 * n or s.size != 2 * n or b.size != n:
            raise ValueError("KeypointAP: %d boxes, %d center values, %d scale values, %d box scores" % (n, c.size, s.size, b.size))
        return np.concatenate([c.reshape(n, 2), s.reshape(n, 2), b[:, None]], 1)

    def _launch(self, parts, boxes, image_ids, bbox_ids, keep):
        """parts: [(address of preds, address of maxvals, boxes)] in the order of `boxes` (float32 [n][5], host).  One upload of the box
        table, one pa_kpt_poses per part into ONE chunk: poses [n][K][3] | scores [n] | areas [n]."""
        n, k = len(boxes), self.k
        table = torch.from_numpy(np.ascontiguousarray(boxes)).pin_memory().to(self.device, non_blocking=True)
        chunk = torch.empty(n * (3 * k + 2), dtype=torch.float32, device=self.device)
        base, first = chunk.data_ptr(), 0
        for preds, maxvals, count in parts:
            check(lib.pa_kpt_poses(preds, maxvals, table.data_ptr() + 20 * first, count, k, self.heatmap_size[0], self.heatmap_size[1],
                                   self.vis_thr, base + 12 * k * first, base + 4 * (3 * k * n + first), base + 4 * ((3 * k + 1) * n + first),
                                   _stream()), "pa_kpt_poses (%d boxes, %d keypoints)" % (count, k))
            first += count
        self._chunks.append((chunk, n))
        self._images += image_ids
        self._bbox_ids += bbox_ids
        self._last = (keep, table)                           # what the enqueued launches read, until the next call
        self._records = None
        return self

    def add(self, preds, maxvals, centers, scales, box_scores, image_ids, bbox_ids=None):
        """n boxes: preds float32 [n][K][2] in heat-map pixels and maxvals float32 [n][K] as `keypoints` returns them (numpy arrays or CUDA
        tensors); centers [n][2], scales [n][2] (box size / 200) and box_scores [n] as mmpose's img_metas carry them; image_ids: the photo
        of every box; bbox_ids: its number among all boxes (default: the order of arrival).  A photo's boxes may arrive in different calls.
        Nothing is copied back.  -> self."""
        dev = _device([preds, maxvals], self.device)
        if dev != self.device:
            raise RuntimeError("painter_engine: this KeypointAP lives on %s" % self.device)
        up = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)).contiguous()
        p, m = up(preds), up(maxvals)
        n = int(m.shape[0]) if m.dim() == 2 else -1
        if p.dtype != torch.float32 or m.dtype != torch.float32 or n < 0 or tuple(m.shape) != (n, self.k) or tuple(p.shape) != (n, self.k, 2):
            raise ValueError("KeypointAP.add: preds %s %s, maxvals %s %s for %d keypoints" % (p.dtype, tuple(p.shape), m.dtype, tuple(m.shape), self.k))
        image_ids, bbox_ids = self._ids(n, image_ids, bbox_ids)
        if n == 0:
            return self
        return self._launch([(p.data_ptr(), m.data_ptr(), n)], self._boxes(n, centers, scales, box_scores), image_ids, bbox_ids, (p, m))

    def add_decodes(self, decodes, centers, scales, box_scores, image_ids, bbox_ids=None):
        """decodes: launched PoseDecodes (`pa_pose_keypoints`); preds and maxvals are read where they left them, their own `result()` is
        untouched.  centers, scales, box_scores, image_ids, bbox_ids: of all their boxes, in the order of the decodes.  -> self."""
        decodes = list(decodes)
        for i, d in enumerate(decodes):
            if not isinstance(d, PoseDecode) or not hasattr(d, "workspace"):
                raise TypeError("KeypointAP.add_decodes: entry %d is not a launched keypoint PoseDecode" % i)
            if d.out.device != self.device:
                raise RuntimeError("painter_engine: this KeypointAP lives on %s" % self.device)
            if d.k != self.k or (d.w, d.h) != self.heatmap_size:
                raise ValueError("KeypointAP.add_decodes: decode %d has %d keypoints on %d x %d pictures, this scorer %d on %d x %d"
                                 % (i, d.k, d.w, d.h, self.k, *self.heatmap_size))
        n = sum(d.n for d in decodes)
        image_ids, bbox_ids = self._ids(n, image_ids, bbox_ids)
        if n == 0:
            return self
        parts = [(d.out.data_ptr(), d.out.data_ptr() + 8 * d.n * d.k, d.n) for d in decodes if d.n]
        return self._launch(parts, self._boxes(n, centers, scales, box_scores), image_ids, bbox_ids, decodes)

    def poses(self):
        """The pose table as it sits on the device, copied back -> (poses float32 [N][K][3], scores float32 [N], areas float32 [N]) of all
        boxes in the order of arrival (tests, measurements)."""
        k = self.k
        if not self._chunks:
            return np.zeros((0, k, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)
        parts = [(c.cpu().numpy(), n) for c, n in self._chunks]
        return (np.concatenate([a[:3 * k * n].reshape(n, k, 3) for a, n in parts]), np.concatenate([a[3 * k * n:3 * k * n + n] for a, n in parts]),
                np.concatenate([a[3 * k * n + n:] for a, n in parts]))

    def _groups(self):
        """Host work on the ids only: per photo the positions of its boxes in ascending bbox_id, of equal ids the first handed over."""
        groups = {}
        for i, image in enumerate(self._images):
            groups.setdefault(image, []).append(i)
        for image in groups:
            if image not in self._gt:
                raise ValueError("KeypointAP: image id %r has boxes but is not in ground_truth" % (image,))
        out = {}
        for image, mine in groups.items():
            mine = sorted(mine, key=lambda i: self._bbox_ids[i])          # stable
            rows = [i for n, i in enumerate(mine) if n == 0 or self._bbox_ids[i] != self._bbox_ids[mine[n - 1]]]
            if len(rows) > KPT_MAX_BOX:
                raise ValueError("KeypointAP: photo %r has %d boxes (at most %d)" % (image, len(rows), KPT_MAX_BOX))
            out[image] = np.array(rows, np.int32)
        return out

    def _evaluate(self, images, groups, tables):
        """One pa_kpt_evaluate over the photos `images` -> (out, its layout, shape): enqueued, not copied back."""
        poses, scores, areas, n_rows = tables
        n, k = len(images), self.k
        d_cap = max([self.min_caps[0]] + [len(groups[i]) for i in images])
        g_cap = max([self.min_caps[1]] + [len(self._gt[i][1]) for i in images])
        max_det = max(self.max_dets)
        sections = [("jobs", np.uint8, ctypes.sizeof(KptJob) * n, 16)]
        for j, image in enumerate(images):
            sections += [("rows%d" % j, np.int32, len(groups[image]), 4), ("kp%d" % j, np.float64, self._gt[image][0].size, 8),
                         ("gt%d" % j, KPT_GT, len(self._gt[image][1]), 8)]
        up = _Upload(sections, self.device)
        jobs = (KptJob * n)()
        for j, (job, image) in enumerate(zip(jobs, images)):
            kp, table = self._gt[image]
            job.rows, job.n_box = up.put("rows%d" % j, groups[image]), len(groups[image])
            if len(table):
                job.gt_keypoints, job.gt_table, job.n_gt = up.put("kp%d" % j, kp.ravel()), up.put("gt%d" % j, table), len(table)
        shape = (n, d_cap, g_cap, max_det)
        what = "pa_kpt_evaluate (sizes %s)" % (shape,)
        sent = up.send(jobs)
        workspace = _workspace(lib.pa_kpt_workspace_bytes, shape, what, self.device)
        oat, osize = _layout([("records", KPT_RECORD, n * max_det, 8), ("counts", np.int32, n, 4), ("survivors", np.int32, n, 4),
                              ("flags", np.uint32, n, 4)])
        out = torch.zeros(osize, dtype=torch.uint8, device=self.device)
        ptr = lambda name: out.data_ptr() + oat[name][0]
        T, A, par = len(self.iou_thrs), len(self.area_ranges), self.params.data_ptr()
        check(lib.pa_kpt_evaluate(sent, n, poses.data_ptr(), scores.data_ptr(), areas.data_ptr(), n_rows, d_cap, g_cap, k, par,
                                  self.oks_thr if self.use_nms else -1.0, max_det, par + 8 * k, T, par + 8 * (k + T), A, ptr("records"),
                                  ptr("counts"), ptr("survivors"), ptr("flags"), workspace.data_ptr(), _stream()), what)
        self._last_eval = (up.host, up.dev, workspace, shape, images)          # the workspace is what the tests read
        return out, oat, shape

    def records(self):
        """Groups and de-duplicates on the host (ids only), concatenates the pose chunks once, launches pa_kpt_evaluate and makes the one
        copy back (and synchronisation) -> {image id: KPT_RECORDs in evaluation order}, for every photo of ground_truth; one without boxes
        has none (its ground truths still count in `result()`); `survivors` then holds per photo how many boxes the NMS kept.  ValueError
        for boxes of a photo that ground_truth does not list, and for a refused photo: it names the photo and the flag bit."""
        if self._records is None:
            groups = self._groups()
            recs = {image: np.zeros(0, KPT_RECORD) for image in self.ground_truth}
            self.survivors = {image: 0 for image in self.ground_truth}
            images = list(groups)
            if images:
                k, total = self.k, len(self._images)
                cat = lambda lo, hi: torch.cat([c[lo(n):hi(n)] for c, n in self._chunks])
                tables = (cat(lambda n: 0, lambda n: 3 * k * n), cat(lambda n: 3 * k * n, lambda n: 3 * k * n + n),
                          cat(lambda n: 3 * k * n + n, lambda n: 3 * k * n + 2 * n), total)
                calls = [self._evaluate(images[i:i + KPT_MAX_JOBS], groups, tables) for i in range(0, len(images), KPT_MAX_JOBS)]
                a = torch.cat([o for o, _, _ in calls]).cpu().numpy()
                self._outs, base, first = calls, 0, 0                # kept for a caller that wants the words of a refused set
                for out, oat, (n, _, _, max_det) in calls:
                    part = a[base:base + out.numel()]
                    base += out.numel()
                    table, counts = _section(part, oat, "records").reshape(n, max_det), _section(part, oat, "counts")
                    flags, surv = _section(part, oat, "flags"), _section(part, oat, "survivors")
                    _refuse("KeypointAP", flags, KPT_FLAGS, name=lambda i: "photo %r" % (images[first + i],),
                            rest="photos of this call are refused and emit nothing")
                    for j in range(n):
                        recs[images[first + j]] = table[j, :counts[j]].copy()
                        self.survivors[images[first + j]] = int(surv[j])
                    first += n
            self._records = recs
        return self._records

    def result(self):
        """`keypoint_ap_metrics` of `records()` -> dict(AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl, precision, recall): accumulate
        and summarize on the host; COCOeval's formulas restated, unverified against xtcocotools."""
        return keypoint_ap_metrics(self.records(), self.ground_truth, self.iou_thrs, None, [tuple(r) for r in self.area_ranges.tolist()],
                                   self.max_dets)


# ---- painting targets from annotations (csrc/painter_paint.hip, include/painter_paint.h)
PAINT_MAX_COLOURS, PAINT_MAX_SEGMENTS, PAINT_MAX_MASKS, PAINT_CELLS, PAINT_MAX_JOINTS, PAINT_MAX_TABLE = 1024, 1024, 4096, 6400, 32, 1024
PAINT_LABELS_U8, PAINT_LABELS_I32, PAINT_IDS_I32, PAINT_IDS_RGB = range(4)


class PaintJob(ctypes.Structure):
    """pa_paint_job of include/painter_paint.h."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("table", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("n_table", ctypes.c_int32)]


def _u8_palette(who, palette, default, rows=None, channels=3):
    """[K][channels] integer colours 0 .. 255, or None for `default()` -> uint8 numpy, a copy."""
    pal = np.array(default() if palette is None else palette)
    if pal.ndim != 2 or pal.shape[1] != channels or pal.shape[0] < 1 or (rows is not None and pal.shape[0] != rows) or \
            not ((pal == np.floor(pal)).all() and pal.min() >= 0 and pal.max() <= 255):
        raise ValueError("%s: the palette holds integer colours 0..255 as [%s][%d], got %s" % (who, rows or "K", channels, pal.shape))
    return np.ascontiguousarray(pal.astype(np.uint8))


def _paint_sources(who, maps, kinds):
    """The maps of a semantic call, checked on the host before anything touches the device: {accepted dtype / trailing shape: kind}."""
    out = []
    for i, m in enumerate(maps):
        m = m if torch.is_tensor(m) else np.asarray(m)
        key = (str(m.dtype).replace("torch.", ""), tuple(m.shape[2:]))
        if len(m.shape) < 2 or key not in kinds or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError("%s: picture %d is %s %s; accepted: %s" % (who, i, key[0], tuple(m.shape), ", ".join(
                "%s [H][W]%s" % (d, "".join("[%d]" % s for s in t)) for d, t in kinds)))
        out.append((m, kinds[key]))
    if not out:
        raise ValueError("%s: no pictures" % who)
    return out


def _paint_launch(who, sources, tables, pal, device):
    """One pa_paint_semantic over a job table -> (the pictures, uint8 CUDA [H][W][3] each; int32 CUDA [n] = labels above the palette)."""
    srcs = [m.contiguous() if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)).to(device) for m, _ in sources]
    for s in srcs:
        if s.device != device:
            raise RuntimeError("%s: the maps are on %s, expected %s" % (who, s.device, device))
    flat = np.concatenate([t.reshape(-1, 2) for t in tables] + [np.zeros((1, 2), np.int32)]).astype(np.int32)
    tab_d = torch.from_numpy(flat).to(device, non_blocking=True)
    pal_d = torch.from_numpy(pal).to(device, non_blocking=True)
    outs = [torch.empty((int(s.shape[0]), int(s.shape[1]), 3), dtype=torch.uint8, device=device) for s in srcs]
    jobs, row = (PaintJob * len(srcs))(), 0
    for k, (s, o, (_, kind), t) in enumerate(zip(srcs, outs, sources, tables)):
        jobs[k] = PaintJob(s.data_ptr(), o.data_ptr(), tab_d.data_ptr() + 8 * row, int(s.shape[0]), int(s.shape[1]), kind, len(t))
        row += len(t)
    host, jobs_d = _job_table(jobs, device)
    bad = torch.empty(len(srcs), dtype=torch.int32, device=device)
    check(lib.pa_paint_semantic(jobs_d.data_ptr(), len(srcs), max(int(s.shape[0]) * int(s.shape[1]) for s in srcs), pal_d.data_ptr(),
                                int(pal.shape[0]), bad.data_ptr(), _stream()), "%s (pa_paint_semantic, %d pictures)" % (who, len(srcs)))
    return outs, bad


def paint_semantic(label_maps, palette=None, device="cuda"):
    """`colorEncode` of Painter/data/ade20k/gen_color_ade20k_sem.py:66-82 on the device: a label map uint8 / int32 [H][W] (numpy or CUDA
    tensor) or a list of them, of any sizes, in ONE launch over a job table -> the painted target, a contiguous uint8 CUDA tensor
    [H][W][3] (a list for a list).  label <= 0 paints black, label l paints palette[l - 1]; palette: [K][3], K <= 1024, default
    `semantic_palette(150, 6)`, that file's PALETTE.  A label above K is an IndexError in the reference: here the pixel paints black, is
    counted on the device, and the call raises ValueError naming the first such picture.  Only the counts come back."""
    single = not isinstance(label_maps, (list, tuple))
    sources = _paint_sources("paint_semantic", [label_maps] if single else list(label_maps),
                             {("uint8", ()): PAINT_LABELS_U8, ("int32", ()): PAINT_LABELS_I32})
    pal = _u8_palette("paint_semantic", palette, lambda: semantic_palette(150, 6))
    if pal.shape[0] > PAINT_MAX_COLOURS:
        raise ValueError("paint_semantic: %d colours, at most %d" % (pal.shape[0], PAINT_MAX_COLOURS))
    device = _device([m for m, _ in sources], device)
    outs, bad = _paint_launch("paint_semantic", sources, [np.zeros((0, 2), np.int32)] * len(sources), pal, device)
    bad = bad.cpu().numpy()
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError("paint_semantic: picture %d has %d pixel(s) with a label above the palette's %d colours; %d of %d pictures do"
                         % (i, int(bad[i]), pal.shape[0], int((bad != 0).sum()), len(bad)))
    return outs[0] if single else outs


def paint_panoptic_semantic(id_maps, segments_info, category_index, palette=None, device="cuda"):
    """The paint loop of Painter/data/coco_semseg/gen_color_coco_panoptic_segm.py:122-138 on the device.  id_maps: a segment-id map
    int32 [H][W], or the RGB annotation PNG uint8 [H][W][3] whose ids are formed on the device as r + 256 g + 65536 b (numpy or CUDA
    tensors), or a list of them; segments_info: per picture the annotation's segments, (segment id, category id) pairs or dicts with
    "id" and "category_id"; category_index: category id -> colour index (the script's catid2colorid); palette [K][3], default
    `semantic_palette()`.  An id no segment lists paints black; where two segments share an id the later one wins, as the script's
    sequential overwrite does.  -> uint8 CUDA [H][W][3] (a list for a list).  A category without a colour index is a KeyError, a colour
    index outside the palette a ValueError, both before anything is launched.  (The script skips an annotation without segments; here
    it paints black.)"""
    single = not isinstance(id_maps, (list, tuple))
    sources = _paint_sources("paint_panoptic_semantic", [id_maps] if single else list(id_maps),
                             {("int32", ()): PAINT_IDS_I32, ("uint8", (3,)): PAINT_IDS_RGB})
    infos = [segments_info] if single else list(segments_info)
    if len(infos) != len(sources):
        raise ValueError("paint_panoptic_semantic: %d pictures, %d segment lists" % (len(sources), len(infos)))
    pal = _u8_palette("paint_panoptic_semantic", palette, semantic_palette)
    if pal.shape[0] > PAINT_MAX_COLOURS:
        raise ValueError("paint_panoptic_semantic: %d colours, at most %d" % (pal.shape[0], PAINT_MAX_COLOURS))
    tables = []
    for i, info in enumerate(infos):
        rows = [(s["id"], s["category_id"]) if isinstance(s, dict) else tuple(s) for s in info]
        if len(rows) > PAINT_MAX_SEGMENTS:
            raise ValueError("paint_panoptic_semantic: picture %d has %d segments, at most %d" % (i, len(rows), PAINT_MAX_SEGMENTS))
        t = np.zeros((len(rows), 2), np.int32)
        for k, (sid, cat) in enumerate(rows):
            colour = int(category_index[cat])
            if not 0 <= colour < pal.shape[0]:
                raise ValueError("paint_panoptic_semantic: picture %d, category %r has colour index %d outside the palette's %d colours"
                                 % (i, cat, colour, pal.shape[0]))
            if not 0 <= int(sid) < 1 << 31:
                raise ValueError("paint_panoptic_semantic: picture %d, segment id %r" % (i, sid))
            t[k] = int(sid), colour
        tables.append(t)
    device = _device([m for m, _ in sources], device)
    outs, _ = _paint_launch("paint_panoptic_semantic", sources, tables, pal, device)
    return outs[0] if single else outs


def _geo_cells(boxes, n, h, w):
    """method="geo_center" of SaveDataPairCustom.__call__ (:115-118, :124-125) with its own expressions, on the host."""
    boxes = np.asarray(boxes)
    if boxes.shape != (n, 4):
        raise ValueError("paint_instances: boxes are [n][4] = x1, y1, x2, y2 for the %d masks, got %s" % (n, boxes.shape))
    cells = np.zeros((n, 2), np.int32)
    for idx in range(n):
        box = boxes[idx]
        center_x, center_y = (box[:2] + box[2:]) / 2
        cells[idx] = int(center_x / w * 79), int(center_y / h * 79)
    if n and (cells.min() < 0 or cells.max() > 79):
        raise ValueError("paint_instances: the centre of box %d lies outside the picture" % int(np.flatnonzero(((cells < 0) | (cells > 79)).any(1))[0]))
    return cells


def paint_instances(masks, size=None, palette=None, method="mass_center", boxes=None, device="cuda"):
    """SaveDataPairCustom.__call__ of Painter/data/mmdet_custom/data/pipelines/transforms.py:93-131 (center_of_mass :153-172) on the
    device: the class-agnostic instance target.  masks: whatever `_bit_masks` takes -- bool / uint8 [n][H][W], bit masks uint32 / int32
    [n][ceil(H W / 32)] with size = (H, W), or a list of COCO RLE dicts; palette [6400][3] in `location_palette()`'s order (the default);
    method "mass_center", or "geo_center" with boxes [n][4] = x1, y1, x2, y2 (the centre is then computed on the host).

    Every mask is painted in the colour of the cell its centre falls in: the integers n, sum x, sum y over its bits, then the
    reference's float64 operations in its order (norm = n or 1e-6, cx = sum x / norm, ax = int(cx / W * 79)).  The reference asserts
    disjoint masks; where masks overlap, the HIGHEST index wins, which is what its sequential overwrite does.  Up to 4096 masks.

    -> (picture uint8 CUDA [H][W][3], cells int32 numpy [n][2] = (ax, ay), empty bool = the reference's "pure black label" that it does
    not save).  The picture stays on the device; 8 n + 4 bytes come back."""
    if method not in ("mass_center", "geo_center"):
        raise NotImplementedError(method)
    if (method == "geo_center") != (boxes is not None):
        raise ValueError("paint_instances: boxes go with method=\"geo_center\", and only with it")
    pal = _u8_palette("paint_instances", palette, location_palette, rows=PAINT_CELLS)
    if _is_rles(masks):
        size = _rle_size(masks) if size is None else size
    else:
        masks = masks if torch.is_tensor(masks) else np.asarray(masks)
        if size is None:
            if len(masks.shape) != 3:
                raise ValueError("paint_instances: bit masks need size=(H, W)")
            size = masks.shape[1:]
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or h * w >= 1 << 31 or len(masks) > PAINT_MAX_MASKS:
        raise ValueError("paint_instances: %d masks of %d x %d; at most %d masks, 1 <= H W < 2^31" % (len(masks), h, w, PAINT_MAX_MASKS))
    cells_in = _geo_cells(boxes, len(masks), h, w) if method == "geo_center" else None
    device = _device([masks], device)
    bits, n = _bit_masks(masks, h, w, device)
    pal_d = torch.from_numpy(pal).to(device, non_blocking=True)
    cells_d = None if cells_in is None else torch.from_numpy(np.concatenate([cells_in, np.zeros((1, 2), np.int32)])).to(device, non_blocking=True)
    ws = _workspace(lib.pa_paint_instances_workspace_bytes, (n,), "pa_paint_instances (%d masks)" % n, device)
    picture = torch.empty((h, w, 3), dtype=torch.uint8, device=device)
    small = torch.empty(2 * max(n, 1) + 1, dtype=torch.int32, device=device)            # cells [n][2] | empty
    check(lib.pa_paint_instances(bits.data_ptr(), n, h, w, pal_d.data_ptr(), None if cells_d is None else cells_d.data_ptr(), ws.data_ptr(),
                                 picture.data_ptr(), small.data_ptr(), small.data_ptr() + 8 * max(n, 1), _stream()),
          "pa_paint_instances (%d masks of %d x %d)" % (n, h, w))
    back = small.cpu().numpy()
    return picture, back[:2 * n].reshape(n, 2).copy(), bool(back[2 * max(n, 1)])


def msra_rectangles(joints, visible, heatmap_size, sigma, image_size=None):
    """mmpose 0.x `TopDownGenerateTarget._msra_generate_target` up to its rectangles, with its own Python expressions (restated from
    mmpose's published source; mmpose is not available where this project is tested, so the rule is UNVERIFIED against it): per joint
    mu = int(joint / feat_stride + 0.5), ul = int(mu - 3 sigma), br = int(mu + 3 sigma + 1), weight = visible, and 0 where
    ul_x >= W or ul_y >= H or br_x < 0 or br_y < 0.  `int()` truncates toward zero, so for sigma = 1.5 and mu < 5 the patch is 9 wide and
    its centre, ul + 5, is not mu.  joints [B][K][>= 2], visible [B][K] or [B][K][>= 1]
    -> (rects int32 [B][K][4] = ul_x, ul_y, br_x, br_y, zeros for weight 0; weights float32 [B][K])."""
    W, H = int(heatmap_size[0]), int(heatmap_size[1])
    joints, visible = np.asarray(joints), np.asarray(visible)
    B, K = joints.shape[:2]
    feat_stride = np.array(image_size if image_size is not None else (W, H)) / [W, H]
    tmp_size = sigma * 3
    rects, weights = np.zeros((B, K, 4), np.int32), np.zeros((B, K), np.float32)
    for b in range(B):
        for k in range(K):
            weight = visible[b, k, 0] if visible.ndim == 3 else visible[b, k]
            mu_x = int(joints[b][k][0] / feat_stride[0] + 0.5)
            mu_y = int(joints[b][k][1] / feat_stride[1] + 0.5)
            ul = [int(mu_x - tmp_size), int(mu_y - tmp_size)]
            br = [int(mu_x + tmp_size + 1), int(mu_y + tmp_size + 1)]
            if ul[0] >= W or ul[1] >= H or br[0] < 0 or br[1] < 0:
                weight = 0
            weights[b, k] = weight
            if weights[b, k] > 0.5:
                rects[b, k] = ul[0], ul[1], br[0], br[1]
    return rects, weights


def msra_table(sigma):
    """R by squared distance from the patch centre for one sigma, with the reference's own numpy expression (the patch of
    _msra_generate_target, `* 255.` and `.astype(np.uint8)` of encode_rgb_target_to_image) -> (uint8 [2 r^2 + 1] with r the patch's
    largest offset, the float32 values before rounding, the centre size // 2)."""
    size = 2 * (sigma * 3) + 1
    c = int(size // 2)
    r = max(c, int(np.ceil(size)) - 1 - c)
    d2 = np.arange(2 * r * r + 1, dtype=np.float32)
    g = np.exp(-d2 / (2 * sigma ** 2))
    return (g * 255.).astype(np.uint8), g, c


def paint_pose(joints, visible, heatmap_size=(192, 256), sigmas=(1.5, 3), palette=None, image_size=None, device="cuda"):
    """The `coco_pose` target: mmpose's MSRA heat maps for both sigmas followed by `encode_rgb_target_to_image` of
    Painter/data/mmpose_custom/data/pipelines/custom_transform.py:64-112, without a heat map in memory.  joints [B][K][>= 2] in pixels
    of `image_size` (default: the heat map's own size, as in the reference's configuration), visible [B][K] or [B][K][>= 1], K <= 32;
    heatmap_size (W, H); sigmas (class sigma -> G, B; kernel sigma -> R); palette [K][2] = (G, B) per joint, default `pose_palette()`.

    Host: `msra_rectangles` for both sigmas and `msra_table` -- a few integers per joint.  Device, integers only: R = table[min d^2] over
    the kernel rectangles that hold the pixel (the table is strictly decreasing, so the smallest d^2 is the reference's max and the
    lowest joint among equals its argmax); (G, B) = black without a class rectangle, the joint's colour with one, and with several the
    colour of the kernel argmax joint.  The MSRA rule is mmpose's, restated from its published source and UNVERIFIED against mmpose;
    the encoding is the reference's own and pinned by tests/golden/painter_paint.npz.  Not built: the TopDownAffine crop of the photo,
    Megvii / UDP encodings, use_different_joint_weights.

    -> (pictures uint8 CUDA [B][H][W][3], weights float32 numpy [B][K]: the target_weight of the kernel sigma)."""
    joints, visible = np.asarray(joints), np.asarray(visible)
    if joints.ndim != 3 or joints.shape[2] < 2 or joints.shape[0] < 1 or not 1 <= joints.shape[1] <= PAINT_MAX_JOINTS or \
            visible.shape[:2] != joints.shape[:2] or visible.ndim not in (2, 3):
        raise ValueError("paint_pose: joints [B][K][>= 2] with 1 <= K <= %d and visible [B][K], got %s and %s"
                         % (PAINT_MAX_JOINTS, joints.shape, visible.shape))
    B, K = joints.shape[:2]
    W, H = int(heatmap_size[0]), int(heatmap_size[1])
    if len(sigmas) != 2 or W < 1 or H < 1 or H * W >= 1 << 31:
        raise ValueError("paint_pose: sigmas = (class sigma, kernel sigma), heatmap_size = (W, H)")
    pal = _u8_palette("paint_pose", palette, lambda: pose_palette()[:-1], channels=2)
    if pal.shape[0] < K:
        raise ValueError("paint_pose: %d joints, the palette has %d colours" % (K, pal.shape[0]))
    table, g, c = msra_table(sigmas[1])
    if len(table) > PAINT_MAX_TABLE or not (np.diff(g) < 0).all():
        raise ValueError("paint_pose: for sigma %r the float32 heat values are not strictly decreasing in d^2 (or the patch is too large):"
                         " the device rule does not hold" % (sigmas[1],))
    rects_c, _ = msra_rectangles(joints, visible, (W, H), sigmas[0], image_size)
    rects_k, weights = msra_rectangles(joints, visible, (W, H), sigmas[1], image_size)
    device = _device((), device)
    tables = np.concatenate([np.stack([rects_c, rects_k], 1).astype(np.int32).view(np.uint8).ravel(), pal[:K].ravel(), table])
    tab_d = torch.from_numpy(tables).to(device, non_blocking=True)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=device)
    o_pal = 32 * B * K
    check(lib.pa_paint_pose(tab_d.data_ptr(), B, K, H, W, c, tab_d.data_ptr() + o_pal, tab_d.data_ptr() + o_pal + 2 * K, len(table),
                            out.data_ptr(), _stream()), "pa_paint_pose (%d boxes of %d joints, %d x %d)" % (B, K, H, W))
    return out, weights


class PainterEngine:
    """One prompt pair, one task, any number of query pictures.  prompt_img / prompt_tgt: RGB uint8 arrays of any size, or contiguous
    uint8 CUDA tensors [H][W][3] on the engine's device (what the `paint_*` encoders return), resized once
    (`Image.resize((input_size, input_size))`, Pillow-exact) and kept on the device."""

    def __init__(self, model, device, task, prompt_img, prompt_tgt, input_size=448, batch_size=8):
        self.device = _device((), device)
        self.task, self.spec = task, _task(task)
        self.model = _unwrap(model)
        self.res = int(input_size)
        self.batch_size = int(batch_size)
        assert self.batch_size >= 1
        self.io = DeviceIO(self.device, res=self.res, hres=self.res, patch=int(self.model.patch_size))
        on_device = lambda x: _pictures(x, self.device) if torch.is_tensor(x) else self.io.upload(x)
        self.prompt = self.io.resize(on_device(prompt_img), (self.res, self.res))
        self.prompt_tgt = self.io.resize(on_device(prompt_tgt), (self.res, self.res))

    def stitch(self, queries):
        """queries: uint8 CUDA [N][res][res][3] -> (imgs, tgts) float32 [N][3][2*res][res]."""
        n = queries.shape[0]
        assert queries.is_cuda and queries.dtype == torch.uint8 and queries.is_contiguous() and \
            tuple(queries.shape) == (n, self.res, self.res, 3), (queries.dtype, tuple(queries.shape))
        imgs = torch.empty((n, 3, 2 * self.res, self.res), dtype=torch.float32, device=self.device)
        tgts = torch.empty_like(imgs)
        check(lib.pa_painter_stitch(self.prompt.data_ptr(), self.prompt_tgt.data_ptr(), queries.data_ptr(), imgs.data_ptr(), tgts.data_ptr(),
                                    n, self.res, self.res, _stream()), "pa_painter_stitch")
        return imgs, tgts

    @torch.no_grad()
    def _launch_batch(self, pictures, sizes, saved):
        """Host copies (the uint8 pictures, the job table) are all enqueued BEFORE the forward, while the stream holds nothing but
        this batch's own resizes; from the forward's first launch to the copy back the host only enqueues kernels.  -> the launched
        DecodePlan, its pictures still on the device."""
        io = self.io
        queries = torch.stack([io.resize(io.upload(p), (self.res, self.res)) for p in pictures])
        plan = DecodePlan(self.task, sizes, self.device, saved=saved)
        imgs, tgts = self.stitch(queries)
        y = _forward(self.model, imgs, tgts)
        return plan.launch(y, self.res, self.res, io.patch)

    def _run_batch(self, pictures, sizes, saved):
        plan = self._launch_batch(pictures, sizes, saved)
        return plan.pictures(), (plan.saved_pictures() if saved else None)

    def _run(self, pictures, sizes, batch, step=None):
        """batch(pictures, sizes) -> one result per picture, called once per `step` (default `batch_size`) pictures in eval mode."""
        if sizes is None:
            sizes = [(p.shape[1], p.shape[0]) for p in pictures]
        assert len(sizes) == len(pictures)
        step = step or self.batch_size
        with _eval_mode(self.model):
            return [batch(pictures[i:i + step], sizes[i:i + step]) for i in range(0, len(pictures), step)]

    def run(self, pictures, sizes=None):
        """pictures: list of RGB uint8 arrays [H][W][3] of any sizes -> one array per picture at its own size, or at sizes[i] =
        (width, height): uint8 [H][W][3], int32 [H][W] or float64 [H][W][3] by task."""
        return [o for b in self._run(pictures, sizes, lambda p, s: self._run_batch(p, s, False)[0]) for o in b]

    def run_restoration(self, pictures, sizes=None):
        """derain / lol / sidd: -> (float64 arrays as `run` returns them, the uint8 pictures those scripts save), both written by the
        one decode launch (a second copy back carries the uint8 pictures)."""
        if self.spec["kind"] != "f64":
            raise ValueError("painter_engine: task %r saves its output as it is; run_restoration is for derain / lol / sidd" % self.task)
        pairs = self._run(pictures, sizes, lambda p, s: self._run_batch(p, s, True))
        return [o for b in pairs for o in b[0]], [o for b in pairs for o in b[1]]

    def run_restoration_scores(self, pictures, gts, sizes=None, metric=None, data_range=2.0):
        """derain / lol / sidd: forward and decode as `run`, then `restoration_scores` of every batch straight from the decode plan's
        device-resident output -- "skimage" reads the float64 pictures, "matlab_y" the `saved` uint8 pictures of the same decode launch;
        no picture is copied back, eight doubles per picture are.  gts: one uint8 [H][W][3] ground truth per picture, of the restored
        picture's size (sizes[i], default the query's own).  metric: None for the task's own -- lol: "skimage", derain: "matlab_y"; sidd's
        eval_sidd.m (MATLAB's built-in ssim / psnr on single blocks) is not restated, so sidd has no default and a metric must be named.
        -> dict(psnr float64 [n], ssim float64 [n]), as `restoration_scores` returns it."""
        if self.task not in RESTORE_DEFAULT_METRIC:
            raise ValueError("painter_engine: run_restoration_scores scores the pictures of derain / lol / sidd, not of %r" % self.task)
        if metric is None:
            metric = RESTORE_DEFAULT_METRIC[self.task]
            if metric is None:
                raise ValueError("painter_engine: %s has no default metric (eval_sidd.m is not restated): pass metric=\"skimage\" or "
                                 "metric=\"matlab_y\" and say which one the numbers are" % self.task)
        win = len(_restore_setup(metric, data_range)[1])                    # everything is checked before the first forward is enqueued
        pictures, gts = list(pictures), list(gts)
        sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
        assert len(sizes) == len(pictures)
        _restore_sizes("run_restoration_scores", [(h, w) for w, h in sizes], gts, win)
        saved = metric == "matlab_y"

        def batch(pairs, sizes):
            truths = [_pictures(g, self.device) for _, g in pairs]
            plan = self._launch_batch([p for p, _ in pairs], sizes, saved)
            preds = [plan.saved_picture(i) if saved else plan.picture(i) for i in range(plan.n_jobs)]
            return RestorationScores(preds, truths, metric, data_range).sums()
        sums = self._run(list(zip(pictures, gts)), sizes, batch)
        return restoration_metrics(np.concatenate(sums) if sums else np.zeros((0, RESTORE_OUT)), metric)

    def run_instances(self, pictures, sizes=None, **kw):
        """coco_pano_inst: forward and decode as `run`, then `instances(picture, **kw)` of every decoded picture straight from the
        decode plan's device-resident uint8 output -- no PNG, no host copy of the picture; the decodes of a batch are all enqueued behind
        its forward before the first copy back.  -> one dict per picture, as `instances` returns it.  post_type="minmax": the evaluator's
        other route, `instances_minmax(picture, palette=...)`; it takes `palette` only."""
        if self.task != "coco_pano_inst":
            raise ValueError("painter_engine: run_instances decodes the pictures of coco_pano_inst, not of %r" % self.task)
        kw.pop("device", None)
        minmax = _post_type("run_instances", kw) == "minmax"
        if not minmax:
            _check_arguments("run_instances", kw, INSTANCE_DEFAULTS)      # before the first forward is enqueued
        args = dict(MINMAX_DEFAULTS if minmax else INSTANCE_DEFAULTS, **kw)
        decode = MinmaxDecode if minmax else InstanceDecode

        def batch(pics, sizes):
            plan = self._launch_batch(pics, sizes, False)
            jobs = [decode(plan.picture(i), *args.values()) for i in range(plan.n_jobs)]
            return [j.result() for j in jobs]
        return [o for b in self._run(pictures, sizes, batch) for o in b]

    def run_pose(self, pictures, flipped=None, sizes=None, **kw):
        """coco_pose: forward and decode as `run` (nearest), then `keypoints` of every batch straight from the decode plan's
        device-resident uint8 output -- no PNG, no copy back of a picture, one copy back of preds / maxvals per batch.

        pictures: the person boxes' query pictures; flipped: None (no flip test), a list with one flipped query per picture (the
        reference's `_flip` files), or "mirror": the columns of every query are mirrored on the host before upload.  Queries and their
        flipped twins go through the same batched forwards.  sizes: (width, height) of the painted pictures, all equal within a call
        (default (192, 256) for every picture).  kw: palette, flip_pairs, shift_heatmap of `keypoints`.
        -> one dict(preds float32 [K][2], maxvals float32 [K]) per picture."""
        def finish(decode, rows):
            res = decode.result()
            return [dict(preds=res["preds"][i], maxvals=res["maxvals"][i]) for i in range(len(rows))]
        # called through the class: `self` needs only task, batch_size, _launch_batch and _run (the argument tests pass a stand-in)
        return [o for b in PainterEngine._pose_decodes(self, "run_pose", pictures, flipped, sizes, kw, finish) for o in b]

    def _pose_decodes(self, who, pictures, flipped, sizes, kw, finish):
        """The batches of `run_pose`: per batch of boxes the forwards of the queries and their twins, one launched PoseDecode, then
        finish(decode, positions of the batch's pictures in `pictures`) -> the list of what `finish` returned."""
        if self.task != "coco_pose":
            raise ValueError("painter_engine: %s decodes the pictures of coco_pose, not of %r" % (who, self.task))
        kw.pop("device", None)
        _check_arguments(who, kw, POSE_DEFAULTS)                          # before the first forward is enqueued
        args = dict(POSE_DEFAULTS, **kw)
        pictures = list(pictures)
        sizes = [(192, 256)] * len(pictures) if sizes is None else [(int(w), int(h)) for w, h in sizes]
        assert len(sizes) == len(pictures)
        assert len(set(sizes)) <= 1, "painter_engine: run_pose needs one output size within a call, got %s" % sorted(set(sizes))
        if isinstance(flipped, str):
            if flipped != "mirror":
                raise ValueError("painter_engine: flipped is None, a list of pictures or \"mirror\", not %r" % flipped)
            flipped = [np.ascontiguousarray(np.asarray(p)[:, ::-1]) for p in pictures]
        elif flipped is not None:
            flipped = list(flipped)
            assert len(flipped) == len(pictures), "painter_engine: one flipped query per picture"
        step = self.batch_size if flipped is None else max(1, self.batch_size // 2)          # boxes per batch: twins share the forward

        def painted(plans, first, count):
            """Pictures first .. first + count of the batch's decode plans as one uint8 tensor [count][H][W][3] (a view when one plan
            holds them all)."""
            if len(plans) == 1:
                return plans[0].run_of(first, count)
            return torch.cat([p.run_of(0, p.n_jobs) for p in plans])[first:first + count]

        def batch(boxes, sizes):
            m, both = len(boxes), [b[0] for b in boxes] + ([b[1] for b in boxes] if flipped else [])
            plans = [self._launch_batch(both[j:j + self.batch_size], sizes[:1] * len(both[j:j + self.batch_size]), False)
                     for j in range(0, len(both), self.batch_size)]
            decode = PoseDecode(painted(plans, 0, m), painted(plans, m, m) if flipped else None, *args.values())
            return finish(decode, [b[2] for b in boxes])
        return self._run(list(zip(pictures, flipped or pictures, range(len(pictures)))), sizes, batch, step)

    def run_pose_ap(self, pictures, centers, scales, box_scores, image_ids, score, flipped=None, sizes=None, bbox_ids=None, **kw):
        """coco_pose: `run_pose`'s batches ending in `score.add_decodes` (a KeypointAP) instead of the copy back: forward, keypoint decode
        and pa_kpt_poses are chained per batch and nothing is copied back before `score.records()` / `score.result()`.  centers, scales,
        box_scores, image_ids, bbox_ids: one per picture (see KeypointAP.add); flipped, sizes, kw: as `run_pose` takes them.  Everything
        is checked before the first forward.  -> score."""
        if self.task != "coco_pose":
            raise ValueError("painter_engine: run_pose_ap scores the pictures of coco_pose, not of %r" % self.task)
        pictures, image_ids = list(pictures), list(image_ids)
        n = len(pictures)
        sizes = [(192, 256)] * n if sizes is None else [(int(w), int(h)) for w, h in sizes]
        bbox_ids = list(range(len(score._images), len(score._images) + n)) if bbox_ids is None else list(bbox_ids)
        boxes = score._boxes(len(box_scores), centers, scales, box_scores)
        if not (n == len(boxes) == len(image_ids) == len(bbox_ids) == len(sizes)):
            raise ValueError("run_pose_ap: %d pictures, %d boxes, %d image ids, %d bbox ids, %d sizes"
                             % (n, len(boxes), len(image_ids), len(bbox_ids), len(sizes)))
        if len(set(sizes)) > 1 or (sizes and sizes[0] != score.heatmap_size):
            raise ValueError("run_pose_ap: the painted pictures are %s, the scorer's heat map %s" % (sorted(set(sizes)), score.heatmap_size))
        unknown = [i for i in image_ids if i not in score.ground_truth]
        if unknown:
            raise ValueError("run_pose_ap: image id %r is not in the scorer's ground_truth" % (unknown[0],))
        if flipped is not None and not isinstance(flipped, str):
            flipped = list(flipped)
            if len(flipped) != n:
                raise ValueError("run_pose_ap: %d pictures, %d flipped pictures" % (n, len(flipped)))

        def finish(decode, idx):
            score.add_decodes([decode], boxes[idx, :2], boxes[idx, 2:4], boxes[idx, 4], [image_ids[i] for i in idx], [bbox_ids[i] for i in idx])
        PainterEngine._pose_decodes(self, "run_pose_ap", pictures, flipped, sizes, kw, finish)
        return score

    def run_semseg_score(self, pictures, gts, score, sizes=None):
        """ade20k_semseg / coco_pano_semseg: forward and decode as `run`, then `score.add` (a SemsegScore or SemsegBoundaryScore) of every batch
        straight from the decode plan's device-resident uint8 output -- the painted pictures are never copied back, and nothing else is before
        `score.matrix()`.  gts: one uint8 label map per picture, of the painted picture's size (sizes[i], default the query's own).
        -> score."""
        if self.task not in ("ade20k_semseg", "coco_pano_semseg"):
            raise ValueError("painter_engine: run_semseg_score scores the pictures of ade20k_semseg / coco_pano_semseg, not of %r" % self.task)
        pictures, gts = list(pictures), list(gts)
        sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
        _same_sizes("run_semseg_score", [np.empty((h, w, 0)) for w, h in sizes], gts)          # before the first forward is enqueued
        assert len(sizes) == len(pictures)

        def batch(pairs, sizes):
            plan = self._launch_batch([p for p, _ in pairs], sizes, False)
            score.add([plan.picture(i) for i in range(plan.n_jobs)], [g for _, g in pairs])
        self._run(list(zip(pictures, gts)), sizes, batch)
        return score

    def run_depth_errors(self, pictures, gts, sizes=None, **kw):
        """nyuv2_depth: forward and decode as `run`, then `depth_errors(picture, gt, **kw)` of every batch straight from the decode plan's
        device-resident int32 output -- no PNG, no copy back of a picture, ten doubles per picture back.  gts: one uint16 map per picture,
        of the painted picture's size.  kw: min_depth, max_depth, crop, divisor.  -> what `depth_errors` returns, for all pictures."""
        if self.task != "nyuv2_depth":
            raise ValueError("painter_engine: run_depth_errors scores the pictures of nyuv2_depth, not of %r" % self.task)
        kw.pop("device", None)
        _check_arguments("run_depth_errors", kw, DEPTH_DEFAULTS)          # before the first forward is enqueued
        args = dict(DEPTH_DEFAULTS, **kw)
        pictures, gts = list(pictures), list(gts)
        sizes = [(p.shape[1], p.shape[0]) for p in pictures] if sizes is None else [(int(w), int(h)) for w, h in sizes]
        _same_sizes("run_depth_errors", [np.empty((h, w, 0)) for w, h in sizes], gts)
        for w, h in sizes:
            _crop_box(args["crop"], h, w)
        assert len(sizes) == len(pictures)

        def batch(pairs, sizes):
            plan = self._launch_batch([p for p, _ in pairs], sizes, False)
            maps = [_maps(g, self.device, torch.uint16) for _, g in pairs]
            return DepthErrors([plan.picture(i) for i in range(plan.n_jobs)], maps, *args.values()).sums()
        sums = self._run(list(zip(pictures, gts)), sizes, batch)
        return depth_metrics(np.concatenate(sums) if sums else np.zeros((0, 10)))


@torch.no_grad()
def run_one_image(img, tgt, size, model, out_path, device, task):
    """The scripts' `run_one_image(img, tgt, size, model, out_path, device)` plus the task name: img, tgt = the normalised float
    arrays [2*res][res][3] the script built, size = (width, height).  Decodes on the device and writes the file the script writes
    (u8 / depth tasks); the three restoration tasks return the float64 array [H][W][3] as theirs do."""
    device = _device((), device)
    spec = _task(task)
    m = _unwrap(model)
    x = torch.as_tensor(np.asarray(img)).unsqueeze(0).permute(0, 3, 1, 2).float().to(device).contiguous()
    t = torch.as_tensor(np.asarray(tgt)).unsqueeze(0).permute(0, 3, 1, 2).float().to(device).contiguous()
    y = _forward(m, x, t)
    output = decode(task, y, [size], x.shape[2] // 2, x.shape[3], int(m.patch_size)).pictures()[0]
    if spec["kind"] == "f64":
        return output
    Image.fromarray(output).save(out_path)
