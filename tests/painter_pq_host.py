"""Panoptic quality, stated in numpy: the definition csrc/painter_pq.hip and painter_engine.PanopticQuality are held to.

Restated from panopticapi's published source -- `pq_compute_single_core` (the joint `np.unique` of gt_id * 2^24 + pred_id, the match at
IoU > 0.5 with the VOID pixels of a prediction taken out of the union, `crowd_labels_dict` where the last crowd segment of a category
wins, the false-positive rule at more than half VOID or crowd) and `PQStat.pq_average`.  panopticapi is not available where this project
is tested: the statement is UNVERIFIED AGAINST panopticapi.  tests/test_painter_pq_cpu.py pins it on cases whose answer is known by
construction.

Tables.  A predicted table is a list of (id, category); a ground-truth table a list of (id, category, iscrowd, area, rank) with area
None (or < 0) = count it from the map; categories are indices 0 .. K - 1; both tables in ascending id order, as the kernels get them.
`tables` builds them from lists of dicts as the Python layer does (category ids mapped, rank = position, sorted by id)."""
import math

import numpy as np

UNLISTED, EMPTY, CATEGORY, UNION, TWICE, ORDER = 1, 2, 4, 8, 16, 32          # the flag bits, 0 .. 5


def gt_ids(gt):
    """int32 [H][W], or uint8 [H][W][3] -> r + 256 g + 65536 b."""
    gt = np.asarray(gt)
    if gt.ndim == 3:
        assert gt.dtype == np.uint8 and gt.shape[2] == 3
        return gt[..., 0].astype(np.int32) + 256 * gt[..., 1].astype(np.int32) + 65536 * gt[..., 2].astype(np.int32)
    assert gt.ndim == 2
    return gt.astype(np.int32)


def _index_map(ids):
    """id -> 1-based index; ids <= 0 are never listed, of a repeated id the first entry stays."""
    out = {}
    for i, v in enumerate(ids):
        if v > 0 and v not in out:
            out[v] = i + 1
    return out


def counts(pred, pred_ids, gt, gt_ids_):
    """-> (C int64 [G + 2][P + 1], whether a non-zero predicted id is not listed).  Such a pixel is not counted."""
    pred, gt = np.asarray(pred).astype(np.int64).ravel(), gt_ids(gt).astype(np.int64).ravel()
    gmap, pmap = _index_map(gt_ids_), _index_map(pred_ids)
    G, P = len(gt_ids_), len(pred_ids)
    C = np.zeros((G + 2, P + 1), np.int64)
    unlisted = False
    pairs, n = np.unique(np.stack([gt, pred], 1), axis=0, return_counts=True) if len(pred) else (np.zeros((0, 2), np.int64), [])
    for (gid, pid), c in zip(pairs.tolist(), n):
        g = 0 if gid == 0 else gmap.get(gid, G + 1)
        if pid != 0 and pid not in pmap:
            unlisted = True
            continue
        C[g, pmap[pid] if pid else 0] += int(c)
    return C, unlisted


def picture(pred, pred_table, gt, gt_table, n_classes):
    """One picture -> dict(flags, matches = [(g, p, category, iou)] in ascending (g, p), fn int64 [K], fp int64 [K], counts).  With a
    non-zero flag word the picture adds nothing (matches, fn, fp are then empty / zero)."""
    K = int(n_classes)
    G, P = len(gt_table), len(pred_table)
    C, unlisted = counts(pred, [s[0] for s in pred_table], gt, [s[0] for s in gt_table])
    flags = UNLISTED if unlisted else 0
    parea = C.sum(0)
    if (parea[1:] == 0).any():
        flags |= EMPTY
    for table in (pred_table, gt_table):
        before = 0
        for s in table:
            if s[0] <= before:
                flags |= ORDER
            before = s[0]
            if not 0 <= s[1] < K:
                flags |= CATEGORY
    out = dict(flags=flags, matches=[], fn=np.zeros(K, np.int64), fp=np.zeros(K, np.int64), counts=C)
    if flags & (ORDER | CATEGORY):
        return out                                                   # nothing is matched: bits 3 and 4 stay clear
    garea = [None] + [int(C[g].sum()) if (s[3] is None or s[3] < 0) else int(s[3]) for g, s in enumerate(gt_table, 1)]
    gmatched, pmatched, matches = [0] * (G + 1), [0] * (P + 1), []
    for g in range(1, G + 1):
        for p in range(1, P + 1):
            c = int(C[g, p])
            if c == 0 or gt_table[g - 1][2] or gt_table[g - 1][1] != pred_table[p - 1][1]:
                continue
            union = int(parea[p]) + garea[g] - c - int(C[0, p])
            if union <= 0:
                flags |= UNION
                continue
            iou = float(np.float64(c) / np.float64(union))
            if iou > 0.5:
                if gmatched[g] or pmatched[p]:
                    flags |= TWICE
                gmatched[g] += 1
                pmatched[p] += 1
                matches.append((g, p, gt_table[g - 1][1], iou))
    crowd = {}
    for g, s in enumerate(gt_table, 1):
        if s[2] and (s[1] not in crowd or s[4] >= gt_table[crowd[s[1]] - 1][4]):
            crowd[s[1]] = g
    fn, fp = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for g, s in enumerate(gt_table, 1):
        if not s[2] and not gmatched[g]:
            fn[s[1]] += 1
    for p, s in enumerate(pred_table, 1):
        if pmatched[p]:
            continue
        inter = int(C[0, p]) + (int(C[crowd[s[1]], p]) if s[1] in crowd else 0)
        if parea[p] > 0 and float(np.float64(inter) / np.float64(parea[p])) > 0.5:
            continue
        fp[s[1]] += 1
    out["flags"] = flags
    if flags == 0:
        out.update(matches=matches, fn=fn, fp=fp)
    return out


def accumulate(pictures, n_classes, acc=None):
    """pictures: iterable of (pred, pred_table, gt, gt_table) in the order they are added -> (tp int64 [K], fp, fn, iou float64 [K]),
    the flag words.  The float64 additions: pictures in order, matches in ascending (g, p)."""
    K = int(n_classes)
    tp, fp, fn, iou = acc if acc is not None else (np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.float64))
    flags = []
    for pred, pred_table, gt, gt_table in pictures:
        r = picture(pred, pred_table, gt, gt_table, K)
        flags.append(r["flags"])
        if r["flags"]:
            continue
        for _, _, cat, v in r["matches"]:
            tp[cat] += 1
            iou[cat] = iou[cat] + np.float64(v)
        fp += r["fp"]
        fn += r["fn"]
    return (tp, fp, fn, iou), flags


def averages(tp, fp, fn, iou, isthing):
    """PQStat.pq_average over all categories, the things and the stuff, in Python floats -> the keys detectron2's COCOPanopticEvaluator
    prints (x 100), `per_class` = [(pq, sq, rq)] x 100 and `n` = the categories averaged per group.  A group without a category that
    has tp + fp + fn > 0 gives nan (panopticapi divides by zero there)."""
    K = len(tp)
    per_class, res, n = [], {}, {}
    for c in range(K):
        t, p, f, s = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        if t + p + f == 0:
            per_class.append((0.0, 0.0, 0.0))
            continue
        per_class.append((100 * (s / (t + 0.5 * p + 0.5 * f)), 100 * (s / t if t != 0 else 0), 100 * (t / (t + 0.5 * p + 0.5 * f))))
    for name, want in (("", None), ("_th", True), ("_st", False)):
        pq = sq = rq = 0.0
        count = 0
        for c in range(K):
            t, p, f, s = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
            if (want is not None and bool(isthing[c]) != want) or t + p + f == 0:
                continue
            count += 1
            pq += s / (t + 0.5 * p + 0.5 * f)
            sq += s / t if t != 0 else 0
            rq += t / (t + 0.5 * p + 0.5 * f)
        n[{"": "All", "_th": "Things", "_st": "Stuff"}[name]] = count
        for key, v in (("PQ", pq), ("SQ", sq), ("RQ", rq)):
            res[key + name] = 100 * (v / count) if count else math.nan
    res["per_class"], res["n"] = per_class, n
    return res


def tables(pred_segments, gt_segments, index=None):
    """Lists of dicts (predictions: id, category_id; ground truth: id, category_id, iscrowd, area) -> the two tables as the Python layer
    hands them to the kernels: categories mapped through `index` (data-set id -> index; None = they are indices; an unknown id gives
    -1), rank = position in the list, sorted by id."""
    look = (lambda c: int(c)) if index is None else (lambda c: index.get(c, -1))
    pt = sorted(((int(s["id"]), look(s["category_id"])) for s in pred_segments), key=lambda s: s[0])
    gt = sorted(((int(s["id"]), look(s["category_id"]), int(bool(s.get("iscrowd", 0))), s.get("area"), rank)
                 for rank, s in enumerate(gt_segments)), key=lambda s: s[0])
    return pt, gt


def pq(preds, pred_segments, gts, gt_segments, n_classes=133, n_things=80, index=None, acc=None):
    """What PanopticQuality.add computes for lists of pictures -> ((tp, fp, fn, iou), flags)."""
    pics = []
    for pred, ps, gt, gs in zip(preds, pred_segments, gts, gt_segments):
        pt, gtab = tables(ps, gs, index)
        pics.append((pred, pt, gt, gtab))
    return accumulate(pics, n_classes, acc)
