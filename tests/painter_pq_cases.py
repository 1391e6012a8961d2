"""Seeded inputs of the panoptic-quality tests and of tools/painter_pq_bench.py: segment maps from random rectangles painted in order
(later ones cover earlier ones), optional pixel noise that makes the runs of equal neighbours short, arbitrary 24-bit ids on the
ground-truth side."""
import numpy as np

K, THINGS = 133, 80


def random_ids(rng, n):
    """n distinct values in [1, 2^24)."""
    draw = [int(v) for v in rng.integers(1, 1 << 24, size=4 * n + 8)]
    ids = list(dict.fromkeys(draw))[:n]
    assert len(ids) == n
    return ids


def rectangles(rng, h, w, n, ids, void=0.15):
    """int32 [h][w]: `n` random rectangles painted in order with ids[i]; about `void` of the picture is never painted over when n is
    small (0 stays VOID)."""
    m = np.zeros((h, w), np.int32)
    for i in range(n):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        y1, x1 = y0 + 1 + int(rng.integers(0, max(1, int(h * (1 - void))))), x0 + 1 + int(rng.integers(0, max(1, int(w * (1 - void)))))
        m[y0:y1, x0:x1] = ids[i]
    return m


def noisy(rng, m, ids, fraction):
    """A copy of `m` where `fraction` of the pixels take a random value of `ids`."""
    out = m.copy()
    hit = rng.random(m.shape) < fraction
    out[hit] = rng.choice(np.asarray(ids, np.int32), size=int(hit.sum()))
    return out


def case(seed, h, w, n_gt, n_pred, noise=0.0, crowd=1, unlisted_gt=True, areas="annotation"):
    """-> dict(pred int32 [h][w], pred_segments, gt int32 [h][w], gt_rgb uint8 [h][w][3], gt_segments).  The prediction is the ground
    truth's layout with some rectangles moved, so that pairs match, miss and overlap; categories are drawn so that several segments share
    one; `crowd` ground-truth segments carry iscrowd; one ground-truth id is left out of the list (`unlisted_gt`); every listed
    predicted id has a pixel.  areas: "annotation" = the counted areas, as a consistent annotation holds them; None = area None."""
    rng = np.random.default_rng(seed)
    gt_ids = random_ids(rng, n_gt + 1)
    gt = rectangles(rng, h, w, n_gt + 1, gt_ids) if n_gt else np.zeros((h, w), np.int32)
    if n_gt and noise:
        gt = noisy(rng, gt, [0] + gt_ids, noise)
    cats = [int(c) for c in rng.integers(0, K, size=max(n_gt, n_pred) + 1)]
    cats[1::3] = cats[0::3][:len(cats[1::3])]                             # neighbours in the list share a category
    listed = gt_ids[:n_gt] if unlisted_gt else gt_ids
    gt_segments = []
    for i, v in enumerate(listed):
        area = int((gt == v).sum())
        gt_segments.append(dict(id=v, category_id=cats[i], iscrowd=int(i < crowd), area=area if areas == "annotation" else None))
    # predictions: the ground-truth layout, ids 1 .. n, then a few rectangles on top
    pred = np.zeros((h, w), np.int32)
    for i, v in enumerate(gt_ids[:n_pred]):
        pred[gt == v] = i + 1
    extra = rectangles(rng, h, w, max(1, n_pred // 3), [int(v) for v in rng.integers(1, n_pred + 1, size=max(1, n_pred // 3))], void=0.6) \
        if n_pred else pred
    pred = np.where(extra > 0, extra, pred).astype(np.int32)
    if n_pred and noise:
        pred = noisy(rng, pred, list(range(0, n_pred + 1)), noise)
    pred_segments = [dict(id=i + 1, category_id=cats[i] if i % 4 else cats[(i + 1) % len(cats)], isthing=True)
                     for i in range(n_pred) if (pred == i + 1).any()]
    rgb = np.stack([gt % 256, gt // 256 % 256, gt // 65536], -1).astype(np.uint8)
    return dict(pred=pred, pred_segments=pred_segments, gt=gt, gt_rgb=rgb, gt_segments=gt_segments)


def gt_for_map(seed, pan, segments, n_extra=3):
    """A synthetic annotation for a decoded panoptic map: its segments under arbitrary 24-bit ids and the categories the decode gave
    them (every other one shifted by a few pixels, so that some pairs match and some do not), plus `n_extra` rectangles of other
    categories, one of them a crowd segment.  -> (gt int32 [H][W], gt_segments)."""
    rng = np.random.default_rng(seed)
    h, w = pan.shape
    ids = random_ids(rng, len(segments) + n_extra)
    gt = np.zeros((h, w), np.int32)
    out = []
    for i, s in enumerate(segments):
        mask = pan == s["id"]
        if i % 2:
            mask = np.roll(mask, 3 + i, axis=1)
        gt[mask] = ids[i]
    extra = rectangles(rng, h, w, n_extra, ids[len(segments):], void=0.7)
    gt = np.where(extra > 0, extra, gt).astype(np.int32)
    for i, s in enumerate(segments):
        if (gt == ids[i]).any():
            out.append(dict(id=ids[i], category_id=int(s["category_id"]), iscrowd=0, area=int((gt == ids[i]).sum())))
    for i in range(n_extra):
        v = ids[len(segments) + i]
        if (gt == v).any():
            out.append(dict(id=v, category_id=int(rng.integers(0, K)), iscrowd=int(i == 0), area=int((gt == v).sum())))
    return gt, out
