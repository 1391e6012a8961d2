"""Host statement of the class-agnostic instance decode (painter_amd.painter_engine.instances, csrc/painter_inst.hip): numpy, exact
integers, stable sorts, float64.  This IS the definition the device path is held to.  TEST INFRASTRUCTURE.

What the reference computes (COCOCAInstSegEvaluatorCustom.post_process_segm_output_by_threshold, then util/matrix_nms.mask_matrix_nms)
is defined only up to float32 summation order and an unspecified sort among tied masknesses; here
  * n (pixels of a mask), S (sum of L1 over them), areas and intersections are integers,
  * the first sort compares maskness = S / (3 n) as rationals, ties to the lower candidate index t * K + c,
  * both sorts of the NMS are descending and stable (ties to the earlier position; a NaN score sorts first, as torch.sort places it),
  * the NMS arithmetic is float64, written operation by operation as the reference writes it in float32.
`torch_evaluator_route` restates the reference's own op sequence on torch tensors (any device) for tools/painter_inst_bench.py."""
from fractions import Fraction

import numpy as np


def _l1_rows(pic, pal, lo, hi):
    """int32 [hi - lo][H * W]: L1 distance of every pixel to the colours lo..hi-1 (per channel one table row per distinct value)."""
    px = pic.reshape(-1, 3).astype(np.int32)
    out = np.zeros((hi - lo, px.shape[0]), np.int32)
    for ch in range(3):
        vals, inv = np.unique(pal[lo:hi, ch].astype(np.int32), return_inverse=True)
        out += np.abs(px[None, :, ch] - vals[:, None])[inv.ravel()]
    return out


def _mask_of(l1, thr):
    return l1.astype(np.float32) / np.float32(3.0) < np.float32(thr)


def stats(pic, pal, thresholds, chunk=400):
    """-> n, S: int64 [T * K], candidate t * K + c."""
    k = len(pal)
    n = np.zeros((len(thresholds), k), np.int64)
    s = np.zeros((len(thresholds), k), np.int64)
    for lo in range(0, k, chunk):
        l1 = _l1_rows(pic, pal, lo, min(lo + chunk, k))
        for t, thr in enumerate(thresholds):
            m = _mask_of(l1, thr)
            n[t, lo:lo + chunk] = m.sum(1)
            s[t, lo:lo + chunk] = (l1 * m).sum(1)
    return n.ravel(), s.ravel()


def survivors(n, s, nms_pre):
    """-> candidate indices of the first nms_pre live candidates in the rational maskness order."""
    live = np.flatnonzero(n > 0)
    order = sorted(live.tolist(), key=lambda i: (Fraction(int(s[i]), int(n[i])), i))
    return np.array(order[:nms_pre], np.int64)


def masks_of(pic, pal, thresholds, cand):
    """-> bool [len(cand)][H * W]."""
    k = len(pal)
    out = np.zeros((len(cand), pic.shape[0] * pic.shape[1]), bool)
    for r, i in enumerate(cand):
        out[r] = _mask_of(_l1_rows(pic, pal, int(i) % k, int(i) % k + 1), thresholds[int(i) // k])[0]
    return out


def intersections(masks):
    """-> int64 [N][N], exact: the products are 0 / 1 and a row sum stays far below 2^24."""
    f = masks.astype(np.float32)
    assert masks.shape[1] < (1 << 24)
    return np.rint(f @ f.T).astype(np.int64)


def pack_bits(masks):
    """bool [N][P] -> uint32 [N][ceil(P / 32)], bit b of word w = pixel 32 w + b."""
    n, p = masks.shape
    pad = np.zeros((n, (p + 31) // 32 * 32), np.uint8)
    pad[:, :p] = masks
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32)


def _descending_stable(scores):
    key = np.where(np.isnan(scores), np.inf, scores)
    return np.argsort(-key, kind="stable")


def matrix_nms(masks, scores, inter=None, max_num=100, kernel="gaussian", sigma=2.0):
    """mask_matrix_nms (util/matrix_nms.py:43-121, filter_thr = nms_pre = -1, labels all one) in float64.
    -> (updated scores of the kept, positions of the kept in the input, intersection matrix of the sorted input)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        order = _descending_stable(scores)
        scores, masks = scores[order], masks[order]
        area = masks.sum(1).astype(np.float64)
        if inter is None:
            inter = intersections(masks)
        fi = inter.astype(np.float64)
        iou = np.triu(fi / (area[None, :] + area[:, None] - fi), 1)
        comp = iou.max(0)[:, None]                                     # compensate_iou[i][j] = column maximum of column i
        if kernel == "gaussian":
            coef = (np.exp(-1 * sigma * iou ** 2) / np.exp(-1 * sigma * comp ** 2)).min(0)
        elif kernel == "linear":
            coef = ((1 - iou) / (1 - comp)).min(0)
        else:
            raise NotImplementedError(kernel)
        scores = scores * coef
        keep = _descending_stable(scores)[:max_num]
    return scores[keep], order[keep], inter


def decode(pic, pal, thresholds, nms_pre=2000, max_num=100, kernel="gaussian", sigma=2.0, stages=None):
    """The whole definition with every stage kept: n, S; survivors (candidate indices in NMS order), their masks, areas, scores before
    the NMS and intersection matrix; the result (scores float64, candidates, masks bool [n][H][W]); `empty` for the reference's
    single zero mask.  stages: an earlier result for the same picture, palette, thresholds and nms_pre, whose integer stages are reused."""
    pal = np.asarray(pal)
    thresholds = [float(t) for t in np.atleast_1d(thresholds)]
    h, w = pic.shape[:2]
    n, s = (stages["n"], stages["s"]) if stages else stats(pic, pal, thresholds)
    cand = stages["survivors"] if stages else survivors(n, s, nms_pre)
    out = dict(n=n, s=s, survivors=cand, live=int((n > 0).sum()))
    if len(cand) == 0:
        out.update(empty=True, scores=np.zeros(1), candidates=np.full(1, -1), masks=np.zeros((1, h, w), bool), labels=np.zeros(1))
        return out
    maskness = s[cand].astype(np.float64) / (3.0 * n[cand].astype(np.float64))
    scores = 1 - maskness / max(maskness.max(), 1.0)
    m = stages["survivor_masks"] if stages else masks_of(pic, pal, thresholds, cand)
    assert np.array_equal(m.sum(1), n[cand])
    new_scores, keep, inter = matrix_nms(m, scores, inter=stages["inter"] if stages else None, max_num=max_num, kernel=kernel, sigma=sigma)
    assert np.array_equal(_descending_stable(scores), np.arange(len(scores)))          # the sort before the NMS moves nothing
    out.update(empty=False, survivor_masks=m, survivor_scores=scores, areas=n[cand], inter=inter, scores=new_scores,
               candidates=cand[keep], masks=m[keep].reshape(-1, h, w), labels=np.ones(len(keep)), maskness=maskness)
    return out


def torch_evaluator_route(segm_u8, palette, thresholds, nms_pre=2000, max_num=100, sigma=2.0):
    """The evaluator's default route as it runs on a GPU, op for op in float32 on torch tensors of segm_u8's device: eight chunks of
    800 colours per threshold, float masks, `torch.sort`, a dense `torch.mm` for the intersections, gaussian decay.
    -> (scores, masks bool [n][H][W])."""
    import torch
    segm = segm_u8.float()
    h, w = segm.shape[:2]
    mask_list, maskness_list = [], []
    for thr in thresholds:
        for lo in range(0, palette.shape[0] + 1, 800):
            colour = palette[lo:lo + 800]
            dist = torch.abs(segm.view(1, h, w, 3) - colour.view(-1, 1, 1, 3)).sum(-1) / 3.
            mask = dist < thr
            keep = mask.sum((1, 2)) > 0
            mask, dist = mask[keep], dist[keep]
            if len(dist) > 0:
                maskness_list.append((dist * mask.float()).sum((1, 2)) / mask.sum((1, 2)))
                mask_list.append(mask)
    if not mask_list:
        return torch.zeros(1), torch.zeros(1, h, w, dtype=torch.bool)
    masks, maskness = torch.cat(mask_list), torch.cat(maskness_list)
    maskness, idx = torch.sort(maskness)
    masks, maskness = masks[idx][:nms_pre], maskness[:nms_pre]
    scores = 1 - maskness / max(torch.max(maskness), 1.)
    area = masks.sum((1, 2)).float()
    scores, idx = torch.sort(scores, descending=True)
    masks, area = masks[idx], area[idx]
    n = len(scores)
    flat = masks.reshape(n, -1).float()
    inter = torch.mm(flat, flat.t())
    area = area.expand(n, n)
    iou = (inter / (area + area.t() - inter)).triu(diagonal=1)
    comp = iou.max(0)[0].expand(n, n).t()
    coef = (torch.exp(-1 * sigma * iou ** 2) / torch.exp(-1 * sigma * comp ** 2)).min(0)[0]
    scores, idx = torch.sort(scores * coef, descending=True)
    return scores[:max_num], masks[idx[:max_num]]
