"""Seeded inputs of the keypoint-AP tests and of tools/painter_kpt_bench.py.  TEST INFRASTRUCTURE.

A data set is a list of photos.  A photo's ground truths are persons in a 640 x 480 frame: a box, K keypoints inside it with visibility
0 / 1 / 2, an area, sometimes a crowd flag, and (where asked) one person without a labelled keypoint.  Its boxes are given as the decode
leaves them -- preds in heat-map pixels (quarters), maxvals in eighths so that equal scores occur, center, scale, box score -- and copy
ground truth d % n_gt with a jitter that grows with every round of copies, so that the NMS meets pairs on both sides of its threshold;
the last quarter are poses of their own.

Decisions on the device are compared as bytes.  That is legitimate only where no decision sits within the arithmetic's error of its
threshold, so `dataset` regenerates a case, seed + 1000, + 2000, ..., until `stable` holds: the statement's records, orders and survivors
are identical with every OKS multiplied by 1 - 1e-9, 1 and 1 + 1e-9 (1000 x the tests' bar on the OKS doubles).  tests/test_painter_kpt_cpu.py
asserts the condition for every case of CASES, which is what the device tests use.  Exempt are only the cases built from OKS exactly 1.0
(EXACT): identical poses give e = 0 and exp(-0.0) = 1 on both sides."""
import functools

import numpy as np

from tests import painter_kpt_host as H

K = 17
HEAT = (192, 256)                                                # (W, H) of the heat map
NUDGES = (-1e-9, 0.0, 1e-9)


def person(rng, k=K, labelled=True, crowd=False):
    """-> (annotation dict, center float32 [2], scale float32 [2])."""
    h = float(rng.uniform(40, 300))
    w = h * 0.75
    x, y = float(rng.uniform(0, 640 - w)), float(rng.uniform(0, 480 - h))
    kp = np.zeros((k, 3))
    kp[:, 0], kp[:, 1] = np.round(rng.uniform(x, x + w, k)), np.round(rng.uniform(y, y + h, k))
    kp[:, 2] = rng.integers(0, 3, k) if labelled else 0
    if labelled:
        kp[int(rng.integers(0, k)), 2] = 2
    kp[kp[:, 2] == 0, :2] = 0                                    # COCO writes 0, 0, 0 for a keypoint without a label
    ann = dict(keypoints=kp.ravel().tolist(), area=round(w * h * float(rng.uniform(0.3, 0.7)), 2), bbox=[x, y, w, h], iscrowd=int(crowd),
               num_keypoints=int((kp[:, 2] > 0).sum()))
    center = np.array([x + w * 0.5, y + h * 0.5], np.float32)
    scale = np.array([w * 1.25 / 200, h * 1.25 / 200], np.float32)
    return ann, center, scale


def to_heat(xy, center, scale, heat=HEAT):
    """Photo pixels -> heat-map pixels in quarters: the inverse of to_image, rounded."""
    full = np.asarray(scale, np.float64) * 200
    p = (np.asarray(xy, np.float64) - np.asarray(center, np.float64) + full * 0.5) * (np.asarray(heat) / full)
    return (np.round(p * 4) / 4).astype(np.float32)


def photo(rng, n_box, n_gt, k=K, unlabelled=False, crowd=False, jitter=1.5):
    """-> (annotations, preds [n_box][k][2], maxvals [n_box][k], centers, scales, box scores)."""
    people = [person(rng, k, labelled=not (unlabelled and g == n_gt - 1), crowd=crowd and g == 0) for g in range(n_gt)]
    preds, maxvals = np.zeros((n_box, k, 2), np.float32), np.zeros((n_box, k), np.float32)
    centers, scales, box_scores = np.zeros((n_box, 2), np.float32), np.zeros((n_box, 2), np.float32), np.zeros(n_box, np.float32)
    n_copy = n_box - n_box // 4 if n_gt else 0
    for d in range(n_box):
        if d < n_copy:
            ann, centers[d], scales[d] = people[d % n_gt]
            xy = np.array(ann["keypoints"]).reshape(k, 3)[:, :2]
            if ann["num_keypoints"] == 0:                       # a pose of its own inside the unlabelled person's box
                xy = np.stack([rng.uniform(ann["bbox"][0], ann["bbox"][0] + ann["bbox"][2], k),
                               rng.uniform(ann["bbox"][1], ann["bbox"][1] + ann["bbox"][3], k)], -1)
            preds[d] = to_heat(xy, centers[d], scales[d]) + (np.round(rng.normal(0, jitter * (1 + d // n_gt), (k, 2)) * 4) / 4).astype(np.float32)
        else:
            _, centers[d], scales[d] = person(rng, k)
            preds[d] = (np.round(rng.uniform(0, [HEAT[0] - 1, HEAT[1] - 1], (k, 2)) * 4) / 4).astype(np.float32)
        maxvals[d] = np.round(rng.uniform(0, 1, k) * 8) / 8
        box_scores[d] = np.round(rng.uniform(0.25, 1) * 8) / 8
        if d % 5 == 4:                                           # the score of the box before: a tie
            maxvals[d], box_scores[d] = maxvals[d - 1], box_scores[d - 1]
    return [p[0] for p in people], preds, maxvals, centers, scales, box_scores


def build(seed, spec, k=K, **kw):
    """spec: [(n_box, n_gt)] per photo, image ids 100, 101, ... -> the data set as a dict; boxes in photo order, bbox_ids None."""
    rng = np.random.default_rng(seed)
    parts, gt, ids = [], {}, []
    for i, (n_box, n_gt) in enumerate(spec):
        anns, *arrays = photo(rng, n_box, n_gt, k, unlabelled=n_gt >= 5, crowd=n_gt >= 5, **kw)
        gt[100 + i] = anns
        parts.append(arrays)
        ids += [100 + i] * n_box
    cat = lambda j: np.concatenate([p[j] for p in parts])
    return dict(ground_truth=gt, preds=cat(0), maxvals=cat(1), centers=cat(2), scales=cat(3), box_scores=cat(4), image_ids=ids, bbox_ids=None,
                settings={})


def statement(case, nudge=0.0, **override):
    """The host statement of a case -> {image id: photo_records(...)}."""
    kw = dict(case["settings"], **override)
    sigmas = kw.get("sigmas", H.SIGMAS)
    pose, scores, areas = H.poses(case["preds"], case["maxvals"], case["centers"], case["scales"], case["box_scores"],
                                  kw.get("heatmap_size", HEAT), kw.get("vis_thr", H.VIS_THR))
    return H.dataset_records(pose, scores, areas, case["image_ids"], case["bbox_ids"], case["ground_truth"], sigmas=sigmas,
                             oks_thr=kw.get("oks_thr", H.OKS_THR), use_nms=kw.get("use_nms", True), iou_thrs=kw.get("iou_thrs", H.IOU_THRS),
                             area_ranges=kw.get("area_ranges", H.AREA_RANGES), max_det=max(kw.get("max_dets", H.MAX_DETS)), nudge=nudge)


def same_decisions(a, b):
    return all(a[i]["records"].tobytes() == b[i]["records"].tobytes() and np.array_equal(a[i]["order"], b[i]["order"]) and
               np.array_equal(a[i]["alive"], b[i]["alive"]) and a[i]["flags"] == b[i]["flags"] for i in a)


def stable(case):
    """The nudge condition on the statement -> (holds, the statement at nudge 0)."""
    runs = [statement(case, nudge) for nudge in NUDGES]
    return same_decisions(runs[0], runs[1]) and same_decisions(runs[2], runs[1]), runs[1]


def dataset(seed, spec, settings=None, check=None, **kw):
    """`build` with the first of seed, seed + 1000, ... whose case is stable (and passes `check(case, statement)`), with its statement."""
    for attempt in range(20):
        case = build(seed + 1000 * attempt, spec, **kw)
        case["settings"] = dict(settings or {})
        ok, ref = stable(case)
        if ok and (check is None or check(case, ref)):
            case["statement"], case["seed"] = ref, seed + 1000 * attempt
            return case
    raise AssertionError("no stable case from seed %d" % seed)


def crowded(seed, n_box=1024, n_distinct=40, n_gt=6):
    """One photo whose n_box boxes are n_distinct poses and their near copies (a quarter-pixel jitter on a few keypoints): the NMS has
    real work and keeps more than 20 and far fewer than n_box."""
    rng = np.random.default_rng(seed)
    anns, preds, maxvals, centers, scales, box_scores = photo(rng, n_distinct, n_gt, unlabelled=True, crowd=True)
    pick = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, n_box - n_distinct)])
    preds = preds[pick].copy()
    moved = rng.random(preds.shape) < 0.1
    preds[moved] += np.float32(0.25)
    maxvals = (np.round(rng.uniform(0, 1, (n_box, K)) * 8) / 8).astype(np.float32)
    return dict(ground_truth={7: anns}, preds=preds, maxvals=maxvals, centers=centers[pick], scales=scales[pick],
                box_scores=(np.round(rng.uniform(0.25, 1, n_box) * 8) / 8).astype(np.float32), image_ids=[7] * n_box, bbox_ids=None, settings={})


def stable_crowded(seed):
    for attempt in range(20):
        case = crowded(seed + 1000 * attempt)
        ok, ref = stable(case)
        if ok and 20 < int(ref[7]["alive"].sum()) < 1024:
            case["statement"], case["seed"] = ref, seed + 1000 * attempt
            return case
    raise AssertionError("no stable case from seed %d" % seed)


def spread(n_box, k=K, far=False, n_gt=2):
    """One photo of n_box poses that cannot suppress one another, the first n_gt of them also its ground truths (EXACT: the ground truth's
    keypoints are the detection's own float32 photo coordinates, so every matched OKS is exactly 1.0).  far: tiny boxes 10^4 pixels apart, so
    that every term of every other OKS underflows to 0."""
    rng = np.random.default_rng(n_box + 7 * k)
    preds = (np.round(rng.uniform(0, [HEAT[0] - 1, HEAT[1] - 1], (n_box, k, 2)) * 4) / 4).astype(np.float32)
    maxvals = (np.round(rng.uniform(0.25, 1, (n_box, k)) * 8) / 8).astype(np.float32)
    step = 1e4 if far else 400.0
    centers = np.stack([step * np.arange(n_box), np.full(n_box, 300.0)], -1).astype(np.float32)
    scales = np.tile(np.array([[0.005, 0.005]] if far else [[0.75, 1.0]], np.float32), (n_box, 1))
    box_scores = np.linspace(1.0, 0.5, n_box).astype(np.float32)
    pose, _, _ = H.poses(preds, maxvals, centers, scales, box_scores, HEAT)
    anns = []
    for g in range(n_gt):
        kp = np.concatenate([pose[g, :, :2].astype(np.float64), np.full((k, 1), 2.0)], 1)
        if far:
            kp[:, 0] += 5e3                                      # far from every detection
        anns.append(dict(keypoints=kp.ravel().tolist(), area=1.0 if far else 9000.0, bbox=[0.0, 0.0, 10.0, 10.0], iscrowd=0, num_keypoints=k))
    return dict(ground_truth={3: anns}, preds=preds, maxvals=maxvals, centers=centers, scales=scales, box_scores=box_scores,
                image_ids=[3] * n_box, bbox_ids=None, settings={})


def with_statement(case, **settings):
    case["settings"] = settings
    case["statement"] = statement(case)
    return case


SIGMAS3 = (0.05, 0.1, 0.2)


def hand_made():
    """K = 3, one box on one ground truth, one keypoint 6 pixels off: the OKS is (2 + exp(-e)) / 3 with e = 36 / (2 sigma_1)^2 / (area +
    2^-52) / 2; the caller's thresholds sit a millionth below and above it, outside the nudge margin.  A second box, identical to the first
    and scored lower, survives only because the NMS is switched off."""
    preds = np.array([[[40, 60], [80, 100], [120, 160]]] * 2, np.float32)
    centers, scales = np.array([[96, 128]] * 2, np.float32), np.array([[0.96, 1.28]] * 2, np.float32)
    maxvals, box_scores = np.array([[1, 1, 1], [0.5, 0.5, 0.5]], np.float32), np.array([1, 1], np.float32)
    pose = H.poses(preds, maxvals, centers, scales, box_scores, HEAT)[0]
    kp = np.concatenate([pose[0, :, :2].astype(np.float64), [[2], [2], [1]]], 1)          # the box's own photo coordinates ...
    kp[1, 1] += 6.0                                                                       # ... but for one: exact in float64
    area = 50.0
    e = 36.0 / (0.1 * 2) ** 2 / (area + H.EPS) / 2
    oks = (2 + np.exp(-e)) / 3
    case = dict(ground_truth={1: [dict(keypoints=kp.ravel().tolist(), area=area, bbox=[40, 60, 80, 100], iscrowd=0, num_keypoints=3)]},
                preds=preds, maxvals=maxvals, centers=centers, scales=scales, box_scores=box_scores, image_ids=[1, 1], bbox_ids=None, oks=oks)
    return with_statement(case, sigmas=SIGMAS3, use_nms=False, iou_thrs=(oks * (1 - 1e-6), oks * (1 + 1e-6)), area_ranges=((0, 1e10),))


CHAIN_HEAT = (24, 32)


def chain(seed=31, n=6):
    """Painted `coco_pose` pictures (tests/painter_pose_cases.py) of 32 x 24 pixels with their flipped twins for two photos of three boxes;
    preds and maxvals are the pose statement's (tests/painter_pose_host.py), which the device decode equals as bytes."""
    from tests import painter_pose_cases as PC
    from tests import painter_pose_host as PH
    rng = np.random.default_rng(seed)
    pictures, flipped = PC.painted_pair(seed, n, CHAIN_HEAT[1], CHAIN_HEAT[0])
    ref = PH.keypoints(pictures, flipped, PC.PALETTE, PC.PAIR, shift=True)
    people = [person(rng) for _ in range(n)]
    gt = {50: [p[0] for p in people[:2]], 51: [people[3][0]], 52: []}
    return dict(ground_truth=gt, preds=ref["preds"], maxvals=ref["maxvals"], centers=np.stack([p[1] for p in people]),
                scales=np.stack([p[2] for p in people]), box_scores=(np.round(rng.uniform(0.25, 1, n) * 8) / 8).astype(np.float32),
                image_ids=[50, 51, 50, 51, 50, 51], bbox_ids=[7, 3, 1, 9, 4, 3], pictures=pictures, flipped=flipped, settings={})


def stable_chain():
    case = chain()
    case["settings"] = dict(heatmap_size=CHAIN_HEAT)
    ok, ref = stable(case)
    assert ok
    case["statement"] = ref
    return case


MIXED = [(0, 2), (3, 0), (1, 1), (65, 9), (130, 5)]           # boxes / ground truths per photo


def _mixed_check(case, ref):
    """Equal scores among the boxes, NMS on both sides of its threshold, matched and unmatched detections."""
    big = ref[104]
    scores = H.poses(case["preds"], case["maxvals"], case["centers"], case["scales"], case["box_scores"], HEAT)[1]
    matched = np.concatenate([r["records"]["matched"] for r in ref.values()])
    return len(set(scores.tolist())) < len(scores) and 1 < int(big["alive"].sum()) < 130 and (matched & np.uint64(1) != 0).any() and \
        (matched & np.uint64(1) == 0).any()


SECOND_WORD = [(93, 70)]           # 70 of the 93 boxes copy a ground truth each, so those of index 64 .. 69 have a box as well


def second_word_facts(case, ref):
    """What the case "second_word" is there for, read from the statement alone: the ground truths of index >= 64 are the second 64-bit
    word of the kernel's free / ignored / taken bits.  -> (evaluated detections, those that take a ground truth of index >= 64 at range
    `all`, threshold 0.5, those that take none there, ground truths of index >= 64 ignored in a range other than `all`)."""
    out, gts = ref[100], case["ground_truth"][100]
    matched, _, which = H._match(out["oks"], out["records"]["area"], gts, 0.5, *H.AREA_RANGES[0])
    ignored = [g for g in range(64, len(gts)) if any(H.gt_ignore(gts[g]) or not lo <= float(gts[g]["area"]) <= hi for lo, hi in H.AREA_RANGES[1:])]
    return len(out["records"]), int((which >= 64).sum()), int((~matched).sum()), len(ignored)


def _second_word_check(case, ref):
    evaluated, high, unmatched, ignored = second_word_facts(case, ref)
    return evaluated == 64 and high >= 1 and unmatched >= 1 and ignored >= 1


# name -> builder; everything the device tests and the measurement use.  EXACT names the cases exempt from the nudge condition.
CASES = {
    "mixed": lambda: dataset(11, MIXED, check=_mixed_check),
    "mixed_64": lambda: dataset(11, MIXED, settings=dict(max_dets=(20, 64)), check=_mixed_check),
    "one": lambda: dataset(12, [(1, 1)]),
    "wave": lambda: dataset(13, [(65, 3)]),
    "crowded": lambda: stable_crowded(14),
    "twenty_one": lambda: with_statement(spread(21)),
    "identical": lambda: with_statement(spread(4), iou_thrs=(0.5, 0.95, 1.0)),
    "far": lambda: with_statement(spread(5, far=True)),
    "no_nms": lambda: dataset(15, [(12, 3), (9, 9)], settings=dict(use_nms=False)),
    "hand_made": hand_made,
    "split": lambda: dataset(16, [(7, 2), (5, 3)]),
    "chain": stable_chain,
    "flags": lambda: dataset(17, [(3, 2), (4, 2), (2, 1)]),
    "second_word": lambda: dataset(18, SECOND_WORD, settings=dict(max_dets=(20, 64)), check=_second_word_check),
}
EXACT = ("identical",)                                           # OKS exactly 1.0 at a threshold of 1.0


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
