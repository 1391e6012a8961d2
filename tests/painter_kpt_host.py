"""COCO keypoint AP in plain numpy -- the DEFINITION that csrc/painter_kpt.hip and painter_engine.KeypointAP are held to.

What TopDownCocoDatasetCustom.evaluate (mmpose_custom/data/topdown_coco_dataset.py:194-315) does after the decode, with the configuration
of configs/coco_256x192_test_offline.py:100-106 (oks_thr 0.9, vis_thr 0.2, soft_nms False) and the sigmas of configs/_base_/coco.py:178-181.
The reference holds `evaluate` itself; the functions it calls are restated here from their published source: mmpose 0.x
`_sort_and_unique_bboxes`, `oks_iou` / `oks_nms`, `_write_coco_keypoint_results` (a JSON round trip: float32 -> its exact double) and
xtcocotools' COCOeval (`loadRes`, `computeOks`, `evaluateImg`, `accumulate`, `summarize` for iouType "keypoints").  Neither mmpose nor
xtcocotools is available where this project is tested: restated, unverified against mmpose / xtcocotools.

The arithmetic, operation by operation (float32 where the reference's arrays are float32, float64 elsewhere):
    to_image   float64 from float32 inputs: ((p * (full / size)) + c) - full * 0.5 with full = (double)scale * 200, rounded to float32
               (painter_engine.to_image).
    box_area   float32(float32(sx * 200) * float32(sy * 200)): np.prod(s * 200.0, axis=1) on a float32 array.
    rescore    a float32 running sum of the maxvals > float32(vis_thr) in joint order, one float32 division by their count (0 without
               any), one float32 multiply by the box score.
    unique     per photo ascending bbox_id (stable), of equal ids the first in the caller's order stays.
    nms order  descending score, equal scores to the HIGHER row: argsort(kind="stable")[::-1].  The reference's scores.argsort()[::-1]
               (numpy's default sort) agrees up to 16 boxes; above that numpy leaves the order of ties unspecified.
    nms oks    between a pivot i and a later box j: dx, dy, dx^2 + dy^2 in float32; e_k = d2_k / var_k / den / 2 in float64, var_k =
               (2 sigma_k)^2, den = (double)float32((a_i + a_j) / 2) + 2^-52; oks = (sum_k exp(-e_k)) / K over ALL K keypoints, added in
               ascending k (the reference's np.sum adds in numpy's unrolled order; the difference is far inside the tolerance of the
               tests); rounded to float32; j is suppressed when float32(oks) > float32(oks_thr).  Greedy.
    eval order the survivors in NMS order (a stable sort by -score keeps it), the first max_det of them.  Without NMS the boxes stay in
               bbox_id order and the stable sort by -score gives equal scores to the LOWER row.
    eval oks   computeOks, all float64; keypoints and scores are the exact doubles of the float32 values.
    matching   evaluateImg's greedy loop: best = min(t, 1 - 1e-10), ignored ground truths last, crowd ground truths can be matched again;
               a ground truth is ignored when iscrowd or num_keypoints == 0, per range also when its area is < lo or > hi.

`nudge` multiplies every OKS by (1 + nudge), in the NMS before the rounding to float32: tests/painter_kpt_cases.py keeps only cases
whose decisions do not change at nudge = -1e-9, 0, +1e-9, which is what makes comparing the device's decisions as bytes legitimate (exp is
the one operation that cannot be made bit-equal to numpy's)."""
import numpy as np

SIGMAS = np.array([0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087, 0.087, 0.089, 0.089])
VIS_THR, OKS_THR = 0.2, 0.9
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (20,)
AREA_RANGES = ((0, 1e10), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))                  # all, medium, large
NAN_POSE, GT_AREA = 1, 2                                                         # flag bits of a refused photo
EPS = np.spacing(1)                                                              # 2^-52

RECORD = np.dtype([("score", np.float32), ("row", np.int32), ("area", np.float64), ("matched", np.uint64), ("ignored", np.uint64)])


def to_image(preds, center, scale, heatmap_size):
    """preds float32 [K][2] in heat-map pixels -> float32 [K][2] in photo pixels."""
    p = np.asarray(preds, np.float32).astype(np.float64)
    c = np.asarray(center, np.float32).astype(np.float64)
    full = np.asarray(scale, np.float32).astype(np.float64) * 200.0
    out = np.empty(p.shape, np.float64)
    for a in range(2):
        out[:, a] = ((p[:, a] * (full[a] / heatmap_size[a])) + c[a]) - full[a] * 0.5
    return out.astype(np.float32)


def box_area(scale):
    s = np.asarray(scale, np.float32)
    return np.float32(np.float32(s[0] * np.float32(200)) * np.float32(s[1] * np.float32(200)))


def rescore(maxvals, box_score, vis_thr=VIS_THR):
    total, count = np.float32(0), 0
    for v in np.asarray(maxvals, np.float32):
        if v > np.float32(vis_thr):
            total = np.float32(total + v)
            count += 1
    if count:
        total = np.float32(total / np.float32(count))
    return np.float32(total * np.float32(box_score))


def poses(preds, maxvals, centers, scales, box_scores, heatmap_size=(192, 256), vis_thr=VIS_THR):
    """Per box what pa_kpt_poses writes -> (poses float32 [n][K][3] = (x, y, maxval) in photo pixels, rescored scores float32 [n], box
    areas float32 [n])."""
    preds, maxvals = np.asarray(preds, np.float32), np.asarray(maxvals, np.float32)
    n, k = maxvals.shape
    out, scores, areas = np.zeros((n, k, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        out[i, :, :2] = to_image(preds[i], centers[i], scales[i], heatmap_size)
        out[i, :, 2] = maxvals[i]
        scores[i] = rescore(maxvals[i], box_scores[i], vis_thr)
        areas[i] = box_area(scales[i])
    return out, scores, areas


def unique_rows(bbox_ids):
    """_sort_and_unique_bboxes for one photo: positions in ascending bbox_id, of equal ids the first one handed over."""
    ids = np.asarray(bbox_ids)
    order = np.argsort(ids, kind="stable")
    return np.array([i for n, i in enumerate(order) if n == 0 or ids[i] != ids[order[n - 1]]], np.int64)


def nms_order(scores, use_nms=True):
    s = np.asarray(scores, np.float32)
    return np.argsort(s, kind="stable")[::-1] if use_nms else np.argsort(-s, kind="stable")


def nms_oks(pivot, others, a_pivot, a_others, sigmas=SIGMAS, nudge=0.0):
    """oks_iou of a pivot float32 [K][3] against boxes float32 [M][K][3] -> float32 [M]."""
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    pivot, others = np.asarray(pivot, np.float32), np.asarray(others, np.float32)
    dx = others[:, :, 0] - pivot[None, :, 0]
    dy = others[:, :, 1] - pivot[None, :, 1]
    d2 = dx * dx + dy * dy
    assert d2.dtype == np.float32
    den = ((np.float32(a_pivot) + np.asarray(a_others, np.float32)) / np.float32(2)).astype(np.float64) + EPS
    e = d2.astype(np.float64) / var[None] / den[:, None] / 2
    term = np.exp(-e)
    total = np.zeros(len(others))
    for k in range(term.shape[1]):                              # ascending k
        total = total + term[:, k]
    return (total / term.shape[1] * (1.0 + nudge)).astype(np.float32)


def oks_nms(pose, scores, areas, sigmas=SIGMAS, oks_thr=OKS_THR, use_nms=True, nudge=0.0):
    """pose float32 [D][K][3], scores float32 [D], areas float32 [D] of one photo's boxes in bbox_id order -> (order int [D], survivor
    flags bool [D] by position in the order)."""
    pose, areas = np.asarray(pose, np.float32), np.asarray(areas, np.float32)
    order = nms_order(scores, use_nms)
    alive = np.ones(len(order), bool)
    if use_nms:
        for r, i in enumerate(order):
            if not alive[r]:
                continue
            later = r + 1 + np.flatnonzero(alive[r + 1:])
            if len(later):
                oks = nms_oks(pose[i], pose[order[later]], areas[i], areas[order[later]], sigmas, nudge)
                alive[later[oks > np.float32(oks_thr)]] = False
    return order, alive


def eval_oks(det, gt_keypoints, gt, sigmas=SIGMAS, nudge=0.0):
    """computeOks of one pair: det float32 [K][3], gt_keypoints [K][3], gt = the annotation (area, bbox) -> float64."""
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    k = len(var)
    g = np.asarray(gt_keypoints, np.float64).reshape(k, 3)
    xd, yd = np.asarray(det, np.float32)[:, 0].astype(np.float64), np.asarray(det, np.float32)[:, 1].astype(np.float64)
    xg, yg, vg = g[:, 0], g[:, 1], g[:, 2]
    k1 = int(np.count_nonzero(vg > 0))
    if k1 > 0:
        dx, dy = xd - xg, yd - yg
    else:
        bb = [float(v) for v in gt["bbox"]]
        x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
        z = np.zeros(k)
        dx = np.maximum(z, x0 - xd) + np.maximum(z, xd - x1)
        dy = np.maximum(z, y0 - yd) + np.maximum(z, yd - y1)
    e = (dx * dx + dy * dy) / var / (float(gt["area"]) + EPS) / 2
    if k1 > 0:
        e = e[vg > 0]
    total = 0.0
    for v in np.exp(-e):
        total = total + v
    return total / e.shape[0] * (1.0 + nudge)


def det_area(det):
    """loadRes: the area of a result's keypoint hull box, float64."""
    x, y = np.asarray(det, np.float32)[:, 0].astype(np.float64), np.asarray(det, np.float32)[:, 1].astype(np.float64)
    return (np.max(x) - np.min(x)) * (np.max(y) - np.min(y))


def gt_ignore(g):
    return bool(g.get("iscrowd", 0)) or int(g["num_keypoints"]) == 0


def _match(oks, dareas, gts, thr, lo, hi):
    """evaluateImg's loop at one threshold and one range over the detections in order -> matched [E], ignored [E], and which [E]: the
    ground truth each detection took, -1 for none."""
    ign = [gt_ignore(g) or float(g["area"]) < lo or float(g["area"]) > hi for g in gts]
    crowd = [bool(g.get("iscrowd", 0)) for g in gts]
    gorder = [g for g in range(len(gts)) if not ign[g]] + [g for g in range(len(gts)) if ign[g]]
    taken = set()
    matched, ignored, which = np.zeros(len(dareas), bool), np.zeros(len(dareas), bool), -np.ones(len(dareas), np.int64)
    for d in range(len(dareas)):
        best, m = min(thr, 1 - 1e-10), -1
        for g in gorder:
            if g in taken and not crowd[g]:
                continue
            if m > -1 and not ign[m] and ign[g]:
                break
            if oks[d, g] < best:
                continue
            best, m = oks[d, g], g
        if m > -1:
            matched[d], ignored[d], which[d] = True, ign[m], m
            taken.add(m)
        else:
            ignored[d] = dareas[d] < lo or dareas[d] > hi
    return matched, ignored, which


def photo_flags(pose, scores, areas, gts):
    flags = 0
    if np.isnan(np.asarray(pose, np.float32)).any() or np.isnan(np.asarray(scores, np.float32)).any() or np.isnan(np.asarray(areas, np.float32)).any():
        flags |= NAN_POSE
    for g in gts:
        a = float(g["area"]) + EPS
        if not (a > 0 and a < np.inf):
            flags |= GT_AREA
    return flags


def photo_records(pose, scores, areas, gts, rows=None, sigmas=SIGMAS, oks_thr=OKS_THR, use_nms=True, iou_thrs=IOU_THRS,
                  area_ranges=AREA_RANGES, max_det=20, nudge=0.0):
    """One photo: its boxes (de-duplicated, in bbox_id order) as pose float32 [D][K][3], rescored scores [D], box areas [D]; gts = COCO
    annotation dicts (keypoints K*3, area, bbox, iscrowd, num_keypoints); rows = the number each box is reported under (default its
    position).  -> dict(records RECORD [E] in evaluation order, order, alive, oks float64 [E][G], flags); a refused photo has no record."""
    pose, scores, areas = np.asarray(pose, np.float32), np.asarray(scores, np.float32), np.asarray(areas, np.float32)
    rows = np.arange(len(scores)) if rows is None else np.asarray(rows)
    flags = photo_flags(pose, scores, areas, gts)
    if flags:
        return dict(records=np.zeros(0, RECORD), order=np.zeros(0, np.int64), alive=np.zeros(0, bool), oks=np.zeros((0, len(gts))), flags=flags)
    order, alive = oks_nms(pose, scores, areas, sigmas, oks_thr, use_nms, nudge)
    kept = order[alive][:max_det]
    oks = np.zeros((len(kept), len(gts)), np.float64)
    for e, d in enumerate(kept):
        for j, g in enumerate(gts):
            oks[e, j] = eval_oks(pose[d], g["keypoints"], g, sigmas, nudge)
    rec = np.zeros(len(kept), RECORD)
    rec["score"], rec["row"] = scores[kept], rows[kept]
    rec["area"] = [det_area(pose[d]) for d in kept]
    T = len(iou_thrs)
    for a, (lo, hi) in enumerate(area_ranges):
        for t, thr in enumerate(iou_thrs):
            matched, ignored, _ = _match(oks, rec["area"], gts, thr, lo, hi)
            bit = np.uint64(1 << (a * T + t))
            rec["matched"][matched] |= bit
            rec["ignored"][ignored] |= bit
    return dict(records=rec, order=order, alive=alive, oks=oks, flags=0)


def dataset_records(pose, scores, areas, image_ids, bbox_ids, ground_truth, **kw):
    """A data set's boxes in the caller's order -> {image id: photo_records(...)} for every photo of ground_truth."""
    image_ids = list(image_ids)
    bbox_ids = list(range(len(image_ids))) if bbox_ids is None else list(bbox_ids)
    out = {}
    for image in ground_truth:
        mine = np.array([i for i, v in enumerate(image_ids) if v == image], np.int64)
        rows = mine[unique_rows([bbox_ids[i] for i in mine])] if len(mine) else mine
        out[image] = photo_records(np.asarray(pose)[rows], np.asarray(scores)[rows], np.asarray(areas)[rows], ground_truth[image], rows, **kw)
    return out


def accumulate(records, ground_truth, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, area_ranges=AREA_RANGES):
    """COCOeval.accumulate for the one category `person`.  records: {image id: RECORD [E]}; photos in ascending image id.
    -> precision [T][R][1][A][M], recall [T][1][A][M], -1 where no ground truth counts."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_ranges), len(max_dets)
    precision, recall = -np.ones((T, R, 1, A, M)), -np.ones((T, 1, A, M))
    images = sorted(ground_truth)
    for a, (lo, hi) in enumerate(area_ranges):
        for m, max_det in enumerate(max_dets):
            scores, matched, ignored, npig = [], [], [], 0
            for image in images:
                rec, anns = records[image], ground_truth[image]
                if len(rec) == 0 and len(anns) == 0:
                    continue
                rec = rec[:max_det]
                scores.append(rec["score"])
                matched.append(rec["matched"])
                ignored.append(rec["ignored"])
                npig += sum(1 for g in anns if not (gt_ignore(g) or float(g["area"]) < lo or float(g["area"]) > hi))
            if npig == 0:
                continue
            scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
            inds = np.argsort(-scores, kind="mergesort")
            matched = (np.concatenate(matched) if matched else np.zeros(0, np.uint64))[inds]
            ignored = (np.concatenate(ignored) if ignored else np.zeros(0, np.uint64))[inds]
            for t in range(T):
                bit = np.uint64(1 << (a * T + t))
                dtm, ign = (matched & bit) != 0, (ignored & bit) != 0
                tp = np.cumsum(dtm & ~ign).astype(np.float64)
                fp = np.cumsum(~dtm & ~ign).astype(np.float64)
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                q = np.zeros(R)
                recall[t, 0, a, m] = rc[-1] if nd else 0
                pr = pr.tolist()
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                    if pi >= nd:
                        break
                    q[ri] = pr[pi]
                precision[t, :, 0, a, m] = q
    return precision, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(precision, recall, iou_thrs=IOU_THRS):
    """COCOeval._summarizeKps: ten numbers at max_dets[-1]; a threshold or range that is not there gives -1.0."""
    A = precision.shape[3]
    at = lambda v: np.flatnonzero(np.asarray(iou_thrs) == v)
    res = {}
    for name, table in (("AP", precision), ("AR", recall)):
        res[name] = _mean(table[..., 0, -1])
        res[name + "50"] = _mean(table[at(.5)][..., 0, -1])
        res[name + "75"] = _mean(table[at(.75)][..., 0, -1])
        for a, size in enumerate("ml", 1):
            res[name + size] = _mean(table[..., a, -1]) if a < A else -1.0
    return res


def keypoint_ap(records, ground_truth, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, area_ranges=AREA_RANGES):
    precision, recall = accumulate(records, ground_truth, iou_thrs, rec_thrs, max_dets, area_ranges)
    res = summarize(precision, recall, iou_thrs)
    res.update(precision=precision, recall=recall)
    return res
