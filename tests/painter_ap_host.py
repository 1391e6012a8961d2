"""COCO instance mask AP in plain numpy, float64 -- the DEFINITION that csrc/painter_ap.hip and painter_engine.InstanceAP are held to.

Restated from the published source of pycocotools' COCOeval (computeIoU / maskUtils.iou, evaluateImg, accumulate, summarize; iouType
"segm") as COCOCAInstSegEvaluatorCustom.py:404-414 (useCats = 0) and COCOInstSegEvaluatorCustom.py:315-329 (useCats = 0 and 1) call it.
pycocotools is not available where this project is tested: restated, unverified against pycocotools.

A picture is (detections, ground truths):
    detections    = dict(masks bool [D][H][W], scores float32 [D], classes int [D] or None = all 0)
    ground truths = dict(masks bool [G][H][W], annotations = [dict(category_id, iscrowd, area), ...]); `area` is the annotation's own
                    number (a double; it decides the area ranges) and None means the pixel count.  The IoU always uses the pixel count.

`picture_records` is computeIoU + evaluateImg for every (mode, range, threshold) at once and returns one RECORD per detection in sorted
order -- the bytes the device writes.  It matches ALL detections, not only the first max_dets[-1]: the greedy loop walks the detections in
order and a detection never changes what an earlier one got, so the first m records are what evaluateImg gives for maxDet = m
(`evaluate_picture` is the loop with the cut, tests/test_painter_ap_cpu.py compares the two).  `accumulate` cuts, as COCOeval.accumulate
does, and `summarize` takes the means."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))          # all, small, medium, large
MODES = ("agnostic", "per_class")                                                    # useCats = 0, useCats = 1
NAN_SCORE, DET_CLASS, GT_CLASS = 1, 2, 4                                             # flag bits of a refused picture

RECORD = np.dtype([("score", np.float32), ("area", np.int32), ("category", np.int32), ("index", np.int32), ("matched", np.uint64, (2,)),
                   ("ignored", np.uint64, (2,))])


def empty_detections(h, w):
    """The reference's stand-in for a picture without a candidate (COCOCAInstSegEvaluatorCustom.py:302-310): one empty mask, score 0."""
    return dict(masks=np.zeros((1, h, w), bool), scores=np.zeros(1, np.float32), classes=np.zeros(1, np.int32))


def _masks(m):
    m = np.asarray(m)
    return (m != 0).reshape(m.shape[0], int(np.prod(m.shape[1:])))


def gt_areas(gts):
    """The area of every annotation as a double: its own number, or the pixel count for None."""
    pix = _masks(gts["masks"]).sum(1) if len(gts["annotations"]) else np.zeros(0, np.int64)
    return np.array([float(pix[g]) if a.get("area") is None else float(a["area"]) for g, a in enumerate(gts["annotations"])], np.float64)


def intersections(dets, gts):
    """-> I int64 [D][G], the detections' pixel counts [D], the ground truths' [G]."""
    d, g = _masks(dets["masks"]), _masks(gts["masks"])
    inter = d.astype(np.int64) @ g.astype(np.int64).T
    return inter, d.sum(1).astype(np.int64), g.sum(1).astype(np.int64)


def ious(inter, darea, gpix, crowd):
    """maskUtils.iou on pixel counts: 0.0 without a common pixel, else I / U in float64, U = area(d) for a crowd ground truth."""
    out = np.zeros(inter.shape, np.float64)
    for d in range(inter.shape[0]):
        for g in range(inter.shape[1]):
            i = int(inter[d, g])
            if i:
                u = int(darea[d]) if crowd[g] else int(darea[d]) + int(gpix[g]) - i
                out[d, g] = np.float64(i) / np.float64(u)
    return out


def detection_order(scores):
    return np.argsort(-np.asarray(scores, np.float32), kind="mergesort")


def picture_flags(dets, gts, n_classes, modes):
    scores = np.asarray(dets["scores"], np.float32)
    flags = NAN_SCORE if np.isnan(scores).any() else 0
    cls = dets.get("classes")
    if "per_class" in modes and cls is not None and len(cls) and ((np.asarray(cls) < 0) | (np.asarray(cls) >= n_classes)).any():
        flags |= DET_CLASS
    if any(not 0 <= int(a["category_id"]) < n_classes for a in gts["annotations"]):
        flags |= GT_CLASS
    return flags


def _match(iou, order, dcls, darea, gcls, crowd, garea, thr, lo, hi, per_class):
    """evaluateImg's loop at one threshold and one range over the detections `order` -> matched [len(order)], ignored [len(order)]."""
    gt_ignore = [bool(crowd[g]) or garea[g] < lo or garea[g] > hi for g in range(len(gcls))]
    gorder = [g for g in range(len(gcls)) if not gt_ignore[g]] + [g for g in range(len(gcls)) if gt_ignore[g]]
    taken = set()
    matched, ignored = np.zeros(len(order), bool), np.zeros(len(order), bool)
    for r, d in enumerate(order):
        best, m = min(thr, 1 - 1e-10), -1
        for g in gorder:
            if per_class and gcls[g] != dcls[d]:
                continue
            if g in taken and not crowd[g]:
                continue
            if m > -1 and not gt_ignore[m] and gt_ignore[g]:
                break
            if iou[d, g] < best:
                continue
            best, m = iou[d, g], g
        if m > -1:
            matched[r], ignored[r] = True, gt_ignore[m]
            taken.add(m)
        else:
            ignored[r] = darea[d] < lo or darea[d] > hi
    return matched, ignored


def _tables(dets, gts):
    n = len(dets["scores"])
    dcls = np.zeros(n, np.int32) if dets.get("classes") is None else np.asarray(dets["classes"]).astype(np.int32)
    gcls = [int(a["category_id"]) for a in gts["annotations"]]
    crowd = [bool(a.get("iscrowd", 0)) for a in gts["annotations"]]
    return dcls, gcls, crowd


def picture_records(dets, gts, n_classes=80, modes=MODES, iou_thrs=IOU_THRS, area_ranges=AREA_RANGES):
    """-> (RECORD [D] in sorted order, flags).  A refused picture (flags != 0) has no record."""
    flags = picture_flags(dets, gts, n_classes, modes)
    if flags:
        return np.zeros(0, RECORD), flags
    return records_from_counts(*intersections(dets, gts), dets, gts, modes, iou_thrs, area_ranges), 0


def records_from_counts(inter, darea, gpix, dets, gts, modes=MODES, iou_thrs=IOU_THRS, area_ranges=AREA_RANGES):
    """The records of a picture from its pixel counts (`intersections`), wherever those were counted; the masks are not read again."""
    dcls, gcls, crowd = _tables(dets, gts)
    iou = ious(inter, darea, gpix, crowd)
    garea = np.array([float(gpix[g]) if a.get("area") is None else float(a["area"]) for g, a in enumerate(gts["annotations"])], np.float64)
    order = detection_order(dets["scores"])
    rec = np.zeros(len(order), RECORD)
    rec["score"], rec["area"], rec["category"], rec["index"] = np.asarray(dets["scores"], np.float32)[order], darea[order], dcls[order], order
    T = len(iou_thrs)
    for mi, mode in enumerate(MODES):
        if mode not in modes:
            continue
        for a, (lo, hi) in enumerate(area_ranges):
            for t, thr in enumerate(iou_thrs):
                matched, ignored = _match(iou, order, dcls, darea, gcls, crowd, garea, thr, lo, hi, mode == "per_class")
                bit = np.uint64(1 << (a * T + t))
                rec["matched"][matched, mi] |= bit
                rec["ignored"][ignored, mi] |= bit
    return rec


def evaluate_picture(dets, gts, thr, area_range, max_det, category=None):
    """COCOeval.evaluateImg as it is written there: the detections (of `category`, or all) in sorted order CUT to max_det, then the loop.
    -> (indices of those detections, matched, ignored)."""
    inter, darea, gpix = intersections(dets, gts)
    dcls, gcls, crowd = _tables(dets, gts)
    iou = ious(inter, darea, gpix, crowd)
    order = [d for d in detection_order(dets["scores"]) if category is None or dcls[d] == category][:max_det]
    if category is not None:                                  # the ground truths of the category only
        keep = [g for g in range(len(gcls)) if gcls[g] == category]
        iou, gcls, crowd, garea = iou[:, keep], [gcls[g] for g in keep], [crowd[g] for g in keep], gt_areas(gts)[keep]
    else:
        garea = gt_areas(gts)
    matched, ignored = _match(iou, order, dcls, darea, gcls, crowd, garea, thr, area_range[0], area_range[1], False)
    return np.array(order, np.int64), matched, ignored


def accumulate(records, annotations, n_classes=80, mode="agnostic", iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS,
               area_ranges=AREA_RANGES):
    """COCOeval.accumulate.  records: per picture its RECORDs; annotations: per picture the ground-truth dicts, `area` a number (see
    `gt_areas`).  -> precision [T][R][K][A][M], recall [T][K][A][M], -1 where there is no non-ignored ground truth; K = 1 in agnostic
    mode."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_ranges), len(max_dets)
    K = n_classes if mode == "per_class" else 1
    mi = MODES.index(mode)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a, (lo, hi) in enumerate(area_ranges):
            for m, max_det in enumerate(max_dets):
                scores, matched, ignored, npig = [], [], [], 0
                for rec, anns in zip(records, annotations):
                    if mode == "per_class":
                        rec, anns = rec[rec["category"] == k], [g for g in anns if int(g["category_id"]) == k]
                    if len(rec) == 0 and len(anns) == 0:
                        continue
                    rec = rec[:max_det]
                    scores.append(rec["score"])
                    matched.append(rec["matched"][:, mi])
                    ignored.append(rec["ignored"][:, mi])
                    npig += sum(1 for g in anns if not (bool(g.get("iscrowd", 0)) or float(g["area"]) < lo or float(g["area"]) > hi))
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
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """COCOeval.summarize's twelve numbers: AP, AP50, AP75, APs, APm, APl at max_dets[-1]; AR<m> for every m of max_dets over all areas;
    ARs, ARm, ARl at max_dets[-1].  A threshold or range that is not there gives -1.0."""
    A = precision.shape[3]
    at = lambda v: np.flatnonzero(np.asarray(iou_thrs) == v)
    res = dict(AP=_mean(precision[:, :, :, 0, -1]), AP50=_mean(precision[at(.5), :, :, 0, -1]), AP75=_mean(precision[at(.75), :, :, 0, -1]))
    for a, name in enumerate(("s", "m", "l"), 1):
        res["AP" + name] = _mean(precision[:, :, :, a, -1]) if a < A else -1.0
    for m, max_det in enumerate(max_dets):
        res["AR%d" % max_det] = _mean(recall[:, :, 0, m])
    for a, name in enumerate(("s", "m", "l"), 1):
        res["AR" + name] = _mean(recall[:, :, a, -1]) if a < A else -1.0
    return res


def with_areas(gts):
    """The annotations of a picture with `area` filled in."""
    return [dict(a, area=v) for a, v in zip(gts["annotations"], gt_areas(gts))]


def instance_ap(pictures, n_classes=80, mode="agnostic", iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, area_ranges=AREA_RANGES):
    """pictures: [(detections, ground truths)] -> dict of `summarize`, plus precision, recall and, per class, `per_class` AP."""
    records = [picture_records(d, g, n_classes, (mode,), iou_thrs, area_ranges) for d, g in pictures]
    assert all(f == 0 for _, f in records), [f for _, f in records]
    precision, recall = accumulate([r for r, _ in records], [with_areas(g) for _, g in pictures], n_classes, mode, iou_thrs, rec_thrs,
                                   max_dets, area_ranges)
    res = summarize(precision, recall, iou_thrs, max_dets)
    res.update(precision=precision, recall=recall)
    if mode == "per_class":
        res["per_class"] = [_mean(precision[:, :, k, 0, -1]) for k in range(n_classes)]
    return res
