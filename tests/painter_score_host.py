"""Host statement of the scoring routes (csrc/painter_score.hip): the definition the device path is held to.  TEST INFRASTRUCTURE.

  confusion    SemSegEvaluatorCustom.process (ADE20kSemSegEvaluatorCustom.py:75-112, COCOPanoSemSegEvaluatorCustom.py:67-106): the class
               map of tests/painter_eval_host.class_map (CPU torch, float32) and np.bincount over (K + 1) * pred + gt'.
  depth_sums   nyuv2_depth/eval_with_pngs.py:148-209 and compute_errors (:50-71) up to the sums: the float32 steps in numpy float32, the
               six sums as math.fsum over float64 terms -- the exactly rounded sum, which the device's float64 additions are bounded
               against -- and sum |ln p - ln g|, the scale of the one signed sum.
  depth_metrics, scores   the final ratios.
  torch_evaluator_route   the evaluator's own op sequence on a device, for tools/painter_score_bench.py."""
import math

import numpy as np

from tests import painter_eval_host as EH

EIGEN_CROP = (45, 471, 41, 601)                       # eval_with_pngs.py:205
NAMES = ("silog", "log10", "abs_rel", "sq_rel", "rmse", "rmse_log", "d1", "d2", "d3")          # compute_errors' return order (:71)
SUMS = ("sq", "log_sq", "abs_rel", "sq_rel", "log_diff", "log10")                             # the six sums, in the device's order


def confusion(pictures, gts, palette, dist_type="abs", ignore_label=255):
    """-> (int64 [K + 1][K + 1], number of pixels whose label >= K is not the ignore label; they enter no bin)."""
    palette = np.array(palette)                      # a copy: the engine's cached palettes are read-only
    k = len(palette)
    conf, invalid = np.zeros((k + 1, k + 1), np.int64), 0
    for pic, gt in zip(pictures, gts):
        pred = EH.class_map(pic, palette, dist_type).astype(np.int64).reshape(-1)
        gt = np.asarray(gt).astype(np.int64).reshape(-1)
        assert pred.shape == gt.shape
        ok = (gt < k) | (gt == ignore_label)
        gt = np.where(gt == ignore_label, k, gt)
        invalid += int((~ok).sum())
        conf += np.bincount((k + 1) * pred[ok] + gt[ok], minlength=conf.size).reshape(conf.shape)
    return conf, invalid


def box_of(crop, h, w):
    return (0, h, 0, w) if crop is None else (EIGEN_CROP if isinstance(crop, str) else tuple(int(v) for v in crop))


def depth_sums(pred, gt, min_depth=1e-3, max_depth=80.0, crop=None, divisor=1000.0):
    """pred int32 [H][W], gt uint16 [H][W] -> (float64 [10]: n, three counts, six fsum sums; sum |ln p - ln g|; dict(low, high) = number
    of valid pixels whose prediction was clamped at either end)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.ndim == 2
    div, lo, hi = np.float32(divisor), np.float32(min_depth), np.float32(max_depth)
    p = pred.astype(np.float32) / div
    g = gt.astype(np.float32) / div
    low, high = p < lo, p > hi
    p = np.where(low, lo, p)
    p = np.where(p > hi, hi, p)
    valid = (g > lo) & (g < hi)
    y0, y1, x0, x1 = box_of(crop, *pred.shape)
    box = np.zeros(valid.shape, bool)
    box[y0:y1, x0:x1] = True
    valid &= box
    p, g = p[valid], g[valid]
    assert p.dtype == g.dtype == np.float32
    t = np.maximum(g / p, p / g)
    assert t.dtype == np.float32
    counts = [int(valid.sum())] + [int((t < c).sum()) for c in (1.25, 1.5625, 1.953125)]
    pd, gd = p.astype(np.float64), g.astype(np.float64)
    d, dl = gd - pd, np.log(gd) - np.log(pd)
    terms = [d * d, dl * dl, np.abs(d) / gd, (d * d) / gd, np.log(pd) - np.log(gd), np.abs(np.log10(pd) - np.log10(gd))]
    sums = [math.fsum(x.tolist()) for x in terms]
    return np.array(counts + sums, np.float64), math.fsum(np.abs(terms[4]).tolist()), dict(low=int(low[valid].sum()), high=int(high[valid].sum()))


def depth_metrics(sums):
    """float64 [..][10] -> float64 [..][9] in NAMES order; NaN where n = 0."""
    s = np.asarray(sums, np.float64)
    n = s[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        d1, d2, d3, sq, lg2, abs_rel, sq_rel, err, l10 = np.moveaxis(s[..., 1:] / n[..., None], -1, 0)
        return np.stack([np.sqrt(lg2 - err ** 2) * 100, l10, abs_rel, sq_rel, np.sqrt(sq), np.sqrt(lg2), d1, d2, d3], -1)


def scores(conf):
    """detectron2's SemSegEvaluator.evaluate from the matrix, restated from its published source (the release with the boundary-IoU
    branch); unverified against detectron2, which is not available here."""
    conf = np.asarray(conf)
    k = conf.shape[0] - 1
    acc, iou = np.full(k, np.nan), np.full(k, np.nan)
    tp = conf.diagonal()[:-1].astype(float)
    pos_gt = np.sum(conf[:-1, :-1], axis=0).astype(float)
    class_weights = pos_gt / np.sum(pos_gt)
    pos_pred = np.sum(conf[:-1, :-1], axis=1).astype(float)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    union = pos_gt + pos_pred - tp
    iou_valid = np.logical_and(acc_valid, union > 0)
    iou[iou_valid] = tp[iou_valid] / union[iou_valid]
    return dict(mIoU=100 * np.sum(iou[iou_valid]) / np.sum(iou_valid), fwIoU=100 * np.sum(iou[iou_valid] * class_weights[iou_valid]),
                mACC=100 * np.sum(acc[acc_valid]) / np.sum(acc_valid), pACC=100 * np.sum(tp) / np.sum(pos_gt), IoU=100 * iou, ACC=100 * acc)


def torch_evaluator_route(picture, gt, palette, dist_type="abs", ignore_label=255):
    """What SemSegEvaluatorCustom.process does for one picture, op for op, with the palette and the picture on palette.device (a torch
    tensor float32 [K][3]): the [H][W][K][3] difference tensor, its sum and arg-min there, the copy of the class map to the host, and
    np.bincount.  picture: uint8 numpy [H][W][3]; gt: integer numpy [H][W].  -> int64 [K + 1][K + 1]."""
    import torch
    segm = torch.from_numpy(picture).float().to(palette.device)
    h, w, k = segm.shape[0], segm.shape[1], palette.shape[0]
    diff = segm.view(h, w, 1, 3) - palette.view(1, 1, k, 3)
    if dist_type == "abs":
        dist = torch.abs(diff)
    elif dist_type == "square":
        dist = torch.pow(diff, 2)
    else:
        dist = (torch.abs(diff) + torch.pow(diff, 2)) / 2.
    pred = np.array(torch.sum(dist, dim=-1).argmin(dim=-1).cpu(), dtype=np.int64)
    gt = np.asarray(gt).astype(np.int64)
    gt[gt == ignore_label] = k
    return np.bincount((k + 1) * pred.reshape(-1) + gt.reshape(-1), minlength=(k + 1) ** 2).reshape(k + 1, k + 1)
