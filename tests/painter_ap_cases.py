"""Seeded inputs of the instance-AP tests and of tools/painter_ap_bench.py: ground truths are random rectangles that may overlap;
detections are shifted copies of ground truths plus strays; scores are rounded to eighths so that ties occur; three classes."""
import numpy as np

from tests import painter_ap_host as H

K = 3
SMALL_RANGES = ((0, 1e10), (0, 36), (36, 400), (400, 1e10))              # all / small / medium / large, scaled to small pictures


def rectangle(rng, h, w, lo=2, hi=0.5):
    """bool [h][w]: one rectangle with sides between `lo` pixels and `hi` of the picture."""
    rh = int(rng.integers(min(lo, h), max(min(lo, h), int(h * hi)) + 1))
    rw = int(rng.integers(min(lo, w), max(min(lo, w), int(w * hi)) + 1))
    y, x = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
    m = np.zeros((h, w), bool)
    m[y:y + rh, x:x + rw] = True
    return m


def case(seed, h, w, n_gt, n_det, crowd=1, k=K, areas="annotation", strays=0.25):
    """-> (detections, ground truths) as tests/painter_ap_host.py takes them.  The first `crowd` ground truths carry iscrowd and are
    large; a detection copies ground truth d % n_gt shifted by a few pixels (every fourth one keeps the class of another), the last
    `strays` of them are rectangles of their own.  areas: "annotation" = the pixel count times a factor near 1, as a polygon's area
    differs from its mask's; None = area None."""
    rng = np.random.default_rng(seed)
    gmasks = np.zeros((n_gt, h, w), bool)
    anns = []
    for g in range(n_gt):
        gmasks[g] = rectangle(rng, h, w, hi=0.7 if g < crowd else 0.4)
        pix = int(gmasks[g].sum())
        area = None if areas is None else float(pix) * (1.0 + 0.1 * float(rng.integers(-2, 3)))
        anns.append(dict(category_id=int(rng.integers(0, k)), iscrowd=int(g < crowd), area=area))
    dmasks = np.zeros((n_det, h, w), bool)
    classes = np.zeros(n_det, np.int32)
    n_copy = n_det - int(n_det * strays) if n_gt else 0
    for d in range(n_det):
        if d < n_copy:
            g = d % n_gt
            dy, dx = (int(v) for v in rng.integers(-2, 3, size=2))
            dmasks[d] = np.roll(gmasks[g], (dy, dx), axis=(0, 1))
            if anns[g]["iscrowd"]:                              # a part of the crowd region
                dmasks[d] &= rectangle(rng, h, w, hi=0.6)
            classes[d] = anns[g]["category_id"] if d % 4 else int(rng.integers(0, k))
        else:
            dmasks[d] = rectangle(rng, h, w, hi=0.3)
            classes[d] = int(rng.integers(0, k))
    scores = (np.round(rng.random(n_det) * 8) / 8).astype(np.float32)
    return dict(masks=dmasks, scores=scores, classes=classes), dict(masks=gmasks, annotations=anns)


def not_vacuous(dets, gts, ranges=SMALL_RANGES, k=K):
    """What the issue asks of a fixture, on the STATEMENT: >= 2 true positives, >= 1 false positive, >= 1 detection ignored through a
    crowd match, a pair of equal scores, 0 < AP < 1."""
    rec, flags = H.picture_records(dets, gts, k, ("agnostic",), H.IOU_THRS, ranges)
    assert flags == 0
    bit = np.uint64(1)                                           # range `all`, threshold 0.5
    matched, ignored = (rec["matched"][:, 0] & bit) != 0, (rec["ignored"][:, 0] & bit) != 0
    assert (matched & ~ignored).sum() >= 2 and (~matched & ~ignored).sum() >= 1 and (matched & ignored).sum() >= 1, (matched, ignored)
    assert len(set(rec["score"].tolist())) < len(rec)
    ap = H.instance_ap([(dets, gts)], k, "agnostic", area_ranges=ranges)["AP"]
    assert 0 < ap < 1, ap
    return True


def bits_of(masks):
    """bool [n][H][W] -> uint32 [n][ceil(H W / 32)] in pa_inst_decode's bit layout (pixel p = bit p % 32 of word p / 32)."""
    m = np.asarray(masks)
    m = m.reshape(m.shape[0], int(np.prod(m.shape[1:])))
    pad = (-m.shape[1]) % 32
    m = np.concatenate([m, np.zeros((len(m), pad), bool)], 1)
    return np.packbits(m, axis=1, bitorder="little").view(np.uint32)


def gt_for_instances(seed, masks, classes, n_extra=3, k=80):
    """A synthetic annotation for decoded instances: every other mask shifted by a few pixels under the class the decode gave it, plus
    `n_extra` rectangles, the first a crowd region.  -> ground truths."""
    rng = np.random.default_rng(seed)
    n, h, w = masks.shape
    out, anns = [], []
    for i in range(n):
        m = np.roll(masks[i], 2 + i % 3, axis=1) if i % 2 else masks[i].copy()
        if m.any():
            out.append(m)
            anns.append(dict(category_id=int(classes[i]) if classes is not None else 0, iscrowd=0, area=float(m.sum())))
    for i in range(n_extra):
        m = rectangle(rng, h, w, hi=0.5)
        out.append(m)
        anns.append(dict(category_id=int(rng.integers(0, k)), iscrowd=int(i == 0), area=None))
    return dict(masks=np.stack(out), annotations=anns)
