"""COCO run-length encoding of masks on the host: the statement csrc/painter_rle.hip is held to (not a test).

Restated from pycocotools' published common/maskApi.c (rleEncode, rleToString, rleFrString, rleDecode, rleArea, rleToBbox) and
unverified against pycocotools, which is installed nowhere this project is tested.

    pixels are walked column-major, j = x * h + y (mask[y, x], shape (h, w)); `counts` are the lengths of alternating runs, starting
    with a run of zeros: the first count is 0 when pixel 0 is set; the bottom pixel of column x and the top pixel of column x + 1 are
    neighbours.  string: count i leaves as x = cnts[i] - (i > 2 ? cnts[i - 2] : 0) in groups of five bits, lowest first, bit 0x20 =
    another group follows, + 48.  area = sum of the odd counts; bbox = x, y, w, h, zeros for an empty mask.

The per-pixel loop of `encode` is the definition; `encode_fast` is the vectorised numpy form a host would run (the baseline
tools/painter_rle_bench.py times).  `check` states the order in which the device decode refuses a malformed mask (include/painter_rle.h)."""
import numpy as np


def encode(mask):
    """mask [h][w] (anything truthy is set) -> counts, a list of ints (rleEncode)."""
    mask = np.asarray(mask)
    h, w = mask.shape
    cnts, c, p = [], 0, 0
    for x in range(w):
        for y in range(h):
            v = 1 if mask[y, x] else 0
            if v != p:
                cnts.append(c)
                c, p = 0, v
            c += 1
    cnts.append(c)
    return cnts


def encode_fast(mask):
    """The same counts from the column-major difference, vectorised."""
    mask = np.asarray(mask)
    flat = np.asfortranarray(mask != 0).ravel(order="F").view(np.uint8)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    cnts = np.diff(edges).tolist()
    return ([0] if flat[0] else []) + cnts


def to_string(cnts):
    """counts -> bytes (rleToString)."""
    out = bytearray()
    for i, c in enumerate(cnts):
        x = int(c) - (int(cnts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            c5 = x & 0x1f
            x >>= 5                                   # Python's >> of a negative int is arithmetic
            more = (x != -1) if (c5 & 0x10) else (x != 0)
            if more:
                c5 |= 0x20
            out.append(c5 + 48)
    return bytes(out)


def values(s):
    """bytes / str -> (the signed values before the delta, flag): 7 a byte outside '0' .. 'o', 4 a value of more than 7 groups, 3 the
    string ends inside a value; else 0."""
    s = s.encode("ascii") if isinstance(s, str) else bytes(s)
    if any(not 48 <= b <= 111 for b in s):
        return [], 7
    vals, flag, p = [], 0, 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p == len(s):
                return vals, flag or 3
            c = s[p] - 48
            if k < 7:
                x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10) and k <= 7:
                x |= -1 << (5 * k)
        if k > 7:
            flag = 4
        vals.append(x)
    return vals, flag


def from_string(s):
    """bytes / str -> counts (rleFrString; the counts stay Python ints, so a negative one shows)."""
    vals, _ = values(s)
    cnts = []
    for x in vals:
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def check(counts, h, w):
    """Why the device refuses this mask, 0 if it does not: counts a str / bytes (compressed) or a list of ints (uncompressed).
    7, 4, 3 as `values`; 2 a count is negative after the delta; 1 the counts do not sum to h * w."""
    if isinstance(counts, (str, bytes)):
        _, flag = values(counts)
        if flag:
            return flag
        counts = from_string(counts)
    if any(c < 0 for c in counts):
        return 2
    return 0 if sum(counts) == h * w else 1


def decode(cnts, h, w):
    """counts -> bool [h][w] (rleDecode)."""
    assert all(c >= 0 for c in cnts) and sum(cnts) == h * w, (sum(cnts), h * w)
    flat = np.repeat(np.arange(len(cnts)) & 1, cnts).astype(bool)
    return flat.reshape(w, h).T.copy()


def area(cnts):
    return int(sum(cnts[1::2]))


def to_bbox(cnts, h, w):
    """rleToBbox -> [x, y, w, h] as ints."""
    m = len(cnts) // 2 * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += cnts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]


def pack_bits(masks):
    """bool [n][h][w] -> uint32 [n][ceil(h w / 32)], pixel p = y * w + x is bit p % 32 of word p / 32 (pa_inst_decode's layout)."""
    masks = np.asarray(masks) != 0
    n = masks.shape[0]
    flat = masks.reshape(n, -1)
    words = (flat.shape[1] + 31) // 32
    padded = np.zeros((n, words * 32), np.uint8)
    padded[:, :flat.shape[1]] = flat
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(n, words)


def unpack_bits(bits, h, w):
    """The inverse of `pack_bits` -> bool [n][h][w]."""
    bits = np.ascontiguousarray(bits).view(np.uint32)
    n = bits.shape[0]
    return np.unpackbits(bits.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :h * w].reshape(n, h, w).astype(bool)


def encode_mask(mask, fast=True):
    """-> dict(size, counts (str), runs, area, bbox, cnts): what the device returns per mask."""
    mask = np.asarray(mask)
    h, w = mask.shape
    cnts = encode_fast(mask) if fast else encode(mask)
    return dict(size=[h, w], counts=to_string(cnts).decode("ascii"), runs=len(cnts), area=area(cnts), bbox=to_bbox(cnts, h, w), cnts=cnts)
