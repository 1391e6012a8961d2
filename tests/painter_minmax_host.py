"""Instance decode by nearest colour on the host: the statement csrc/painter_minmax.hip is held to (not a test).

COCOEvaluatorCustom.post_process_segm_output_by_minmax (Painter/eval/coco_panoptic/COCOCAInstSegEvaluatorCustom.py:172-250) in slow,
obvious numpy on integers.  tests/golden/make_golden_painter_minmax.py asserts that the unmodified method gives the same label map,
distance map, instances, classes and float32 scores (bit for bit) on every picture of the fixture.

    L1(p, c)  = sum over the channels of |p_ch - c_ch|                       integer 0..765
    label(p)  = the LOWEST c that attains min_c L1(p, c); dist(p) = that minimum
    n_c, S_c  = number of pixels with label c, sum of their dist
    instances = the colours with n_c > 0, ascending (torch.unique's order, :219)
    neg_c     = (float)((double)S_c / (double)n_c)                            torch.mean of integer-valued float32 (:225)
    m         = max(max_c neg_c, 1.0f); score_c = 1.0f - neg_c / m           one float32 division, one float32 subtraction (:229)
    class     = 0 for the last palette row (the background), otherwise 1     (:220-223)

The reference's float32 sums are exact integers whatever their order only while S_c < 2^24; the statement itself is exact at any size.
`num_windows` of the reference only bounds its memory and has no counterpart."""
import numpy as np

RECORD = np.dtype([("colour", np.int32), ("cls", np.int32), ("n", np.uint32), ("reserved", np.uint32), ("S", np.uint64), ("neg", np.float32),
                   ("score", np.float32)])                     # pa_minmax_record of include/painter_minmax.h


def with_background(palette):
    """[K][3] without the background row -> float32 [K + 1][3], black appended as the evaluator's constructor does (:114-115)."""
    return np.concatenate([np.asarray(palette, np.float32).reshape(-1, 3), np.zeros((1, 3), np.float32)])


def nearest(picture, palette, rows=16):
    """uint8 [H][W][3], [K][3] (background row included) -> (label int32 [H][W], dist int32 [H][W], ties: pixels whose minimum is attained
    by more than one colour)."""
    pic = np.asarray(picture).astype(np.int16)
    pal = np.asarray(palette).astype(np.int16)                 # (|difference| <= 255 and their sum <= 765 fit 16 bits)
    h, w = pic.shape[:2]
    label, dist, ties = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32), 0
    for y in range(0, h, rows):
        d = sum(np.abs(pic[y:y + rows, :, None, ch] - pal[None, None, :, ch]) for ch in range(3))
        label[y:y + rows] = d.argmin(-1)                       # numpy's argmin returns the first minimum
        dist[y:y + rows] = d.min(-1)
        ties += int(((d == d.min(-1, keepdims=True)).sum(-1) > 1).sum())
    return label, dist, ties


def constant_nearest(colour, h, w, palette):
    """`nearest` of a picture of one colour, without the [H][W][K] table."""
    label, dist, ties = nearest(np.array(colour, np.uint8).reshape(1, 1, 3), palette)
    return np.full((h, w), label[0, 0], np.int32), np.full((h, w), dist[0, 0], np.int32), ties * h * w


def statistics(label, dist, k):
    """-> (n uint32 [k], S uint64 [k])"""
    n = np.bincount(label.ravel(), minlength=k).astype(np.uint32)
    s = np.bincount(label.ravel(), weights=dist.ravel().astype(np.float64), minlength=k)      # integers below 2^53: exact in any order
    assert s.max() < 2.0 ** 53
    return n, s.astype(np.uint64)


def records(n, s):
    """-> (RECORD [count] in ascending colour, slot int32 [k]: colour -> position, -1 for a colour without a pixel)"""
    k = len(n)
    colours = np.flatnonzero(n)
    rec = np.zeros(len(colours), RECORD)
    rec["colour"], rec["cls"] = colours, np.where(colours == k - 1, 0, 1)
    rec["n"], rec["S"] = n[colours], s[colours]
    rec["neg"] = (s[colours].astype(np.float64) / n[colours].astype(np.float64)).astype(np.float32)
    m = np.maximum(rec["neg"].max(), np.float32(1.0))
    rec["score"] = np.float32(1.0) - rec["neg"] / m            # float32 throughout
    assert rec["neg"].dtype == np.float32 and rec["score"].dtype == np.float32 and m.dtype == np.float32
    slot = np.full(k, -1, np.int32)
    slot[colours] = np.arange(len(colours), dtype=np.int32)
    return rec, slot


def pack_bits(masks):
    """bool [n][P] -> uint32 [n][ceil(P / 32)], pixel p = bit p % 32 of word p / 32 (pa_inst_decode's layout)."""
    n, p = masks.shape
    pad = np.zeros((n, (p + 31) // 32 * 32), np.uint8)
    pad[:, :p] = masks
    return np.packbits(pad.reshape(n, -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(n, -1)


def masks_of(label, slot, first=0, n_cap=None):
    """-> bool [n_cap][H][W]: the masks of the slots [first, first + n_cap) (default: all)."""
    n_cap = int(slot.max()) + 1 - first if n_cap is None else n_cap
    at = slot[label] - first
    return at[None] == np.arange(n_cap)[:, None, None]


def decode(picture, palette, maps=None):
    """The whole route.  palette: with the background row.  maps: (label, dist, ties) if the caller has them already.
    -> dict(label, dist, ties, n, S, records, slot, count, scores, classes, candidates, areas)."""
    k = len(palette)
    label, dist, ties = nearest(picture, palette) if maps is None else maps
    n, s = statistics(label, dist, k)
    rec, slot = records(n, s)
    return dict(label=label, dist=dist, ties=ties, n=n, S=s, records=rec, slot=slot, count=len(rec), scores=rec["score"].copy(),
                classes=rec["cls"].copy(), candidates=rec["colour"].copy(), areas=rec["n"].astype(np.int32))
