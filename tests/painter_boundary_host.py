"""Host statement of the boundary-IoU branch of the two semantic evaluators (csrc/painter_score.hip: pa_semseg_boundary_confusion,
pa_label_boundary): the definition the device path is held to.  TEST INFRASTRUCTURE.

Restated from detectron2's published SemSegEvaluator (_mask_to_boundary, _compute_boundary_iou, evaluate), which
ADE20kSemSegEvaluatorCustom.py:103-110 and COCOPanoSemSegEvaluatorCustom.py:97-104 run on every picture.  detectron2 and cv2 are not
available where this project is tested, so the definition is unverified against them; no fixture of the reference can be made for it.
Two independent statements of the erosion are held to each other instead (tests/test_painter_boundary_cpu.py).

  dilation            d = max(1, int(round(dilation_ratio * sqrt(h^2 + w^2)))), Python's round.
  boundary            map - (minimum of the map over the (2d + 1)^2 window, every pixel outside the picture read as 0): what d
                      iterations of a 3 x 3 erosion make of the map behind a ring of one zero pixel, cv2.erode ignoring what lies beyond
                      its input.  The minimum is over label values: detectron2 erodes the label map itself.
  boundary_iterated   the same said as the evaluator says it: the zero ring, d times scipy's 3 x 3 grey erosion whose own border never
                      wins (cval = 255), the ring cut off again.
  boundary_confusion  (conf, bconf, invalid) of a list of pictures: conf is painter_score_host.confusion's, bconf the joint histogram of
                      boundary(class map) and boundary(gt with the ignore label replaced by K), every pixel.
  boundary_scores     the boundary lines of `evaluate`."""
import math

import numpy as np

from tests import painter_eval_host as EH
from tests import painter_score_host as SH


# (height, width, dilation_ratio, d): d >= w and d >= h, 2d + 1 wider than the picture, d = 16 / 21 / 25 / 36 across the tiles of 64
# columns and strips of 32 rows the device works in, one-pixel rows and columns, 61 x 83 = 5063 pixels (no multiple of 64).
SHAPES = [(1, 1, .02, 1), (5, 7, .02, 1), (1, 300, .02, 6), (300, 1, .02, 6), (61, 83, .02, 2), (96, 128, .02, 3), (96, 128, .1, 16),
          (61, 83, .2, 21), (150, 200, .1, 25), (61, 83, .35, 36)]


def label_maps(h, w, seed=40):
    """The two maps the branch erodes for the seeded "coco" case of tests/painter_score_cases at h x w -> (picture, ground truth, palette,
    class map uint8, gt' uint8)."""
    from tests import painter_score_cases as C
    pic, gt, pal = C.semseg_case("coco", seed + h + w, h, w)
    pred = EH.class_map(pic, np.array(pal), "abs").astype(np.uint8)
    return pic, gt, pal, pred, np.where(gt == C.IGNORE, len(pal), gt).astype(np.uint8)


def dilation(h, w, dilation_ratio=0.02):
    return max(1, int(round(dilation_ratio * math.sqrt(h * h + w * w))))


def boundary(label_map, d):
    """uint8 [h][w], d >= 1 -> uint8 [h][w]."""
    m = np.asarray(label_map)
    assert m.dtype == np.uint8 and m.ndim == 2 and d >= 1
    h, w = m.shape
    padded = np.zeros((h + 2 * d, w + 2 * d), np.uint8)
    padded[d:d + h, d:d + w] = m
    rows = np.full((h + 2 * d, w), 255, np.uint8)                   # separable: first along the rows, then down the columns
    for dx in range(2 * d + 1):
        np.minimum(rows, padded[:, dx:dx + w], out=rows)
    eroded = np.full((h, w), 255, np.uint8)
    for dy in range(2 * d + 1):
        np.minimum(eroded, rows[dy:dy + h], out=eroded)
    return m - eroded


def boundary_iterated(label_map, d):
    from scipy import ndimage
    m = np.asarray(label_map)
    assert m.dtype == np.uint8 and m.ndim == 2 and d >= 1
    padded = np.zeros((m.shape[0] + 2, m.shape[1] + 2), np.uint8)
    padded[1:-1, 1:-1] = m
    for _ in range(d):
        padded = ndimage.grey_erosion(padded, size=(3, 3), mode="constant", cval=255)
    return m - padded[1:-1, 1:-1]


def boundary_confusion(pictures, gts, palette, dist_type="abs", ignore_label=255, dilation_ratio=0.02):
    """-> (conf int64 [K + 1][K + 1], bconf int64 [K + 1][K + 1], invalid).  A ground-truth value >= K that is not the ignore label makes
    the evaluator fail; here it is counted in `invalid` and read as K in bconf (the device leaves that case unspecified)."""
    palette = np.array(palette)
    k = len(palette)
    assert k <= 254
    conf, invalid = SH.confusion(pictures, gts, palette, dist_type, ignore_label)
    bconf = np.zeros((k + 1, k + 1), np.int64)
    for pic, gt in zip(pictures, gts):
        pred = EH.class_map(pic, palette, dist_type).astype(np.uint8)
        gt = np.asarray(gt).astype(np.int64)
        gt = np.where((gt == ignore_label) | (gt >= k), k, gt).astype(np.uint8)
        d = dilation(pred.shape[0], pred.shape[1], dilation_ratio)
        key = (k + 1) * boundary(pred, d).astype(np.int64) + boundary(gt, d).astype(np.int64)
        bconf += np.bincount(key.reshape(-1), minlength=bconf.size).reshape(bconf.shape)
    return conf, bconf, invalid


def boundary_scores(conf, bconf):
    """-> dict(BoundaryIoU, minIoU_BIoU), float64 [K] in percent, the per-class lines of `evaluate`: b_iou where the boundary union is
    not empty, else NaN; Python's min(iou, b_iou) = b_iou if b_iou < iou else iou."""
    iou = SH.scores(conf)["IoU"] / 100
    bconf = np.asarray(bconf)
    k = bconf.shape[0] - 1
    b_iou = np.full(k, np.nan)
    b_tp = bconf.diagonal()[:-1].astype(float)
    b_pos_gt = np.sum(bconf[:-1, :-1], axis=0).astype(float)
    b_pos_pred = np.sum(bconf[:-1, :-1], axis=1).astype(float)
    b_union = b_pos_gt + b_pos_pred - b_tp
    b_valid = b_union > 0
    b_iou[b_valid] = b_tp[b_valid] / b_union[b_valid]
    return dict(BoundaryIoU=100 * b_iou, minIoU_BIoU=np.array([100 * min(float(a), float(b)) for a, b in zip(iou, b_iou)]))
