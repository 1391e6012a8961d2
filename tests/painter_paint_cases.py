"""Inputs of the target-encoder tests (tests/test_painter_paint_cpu.py, tests/test_painter_paint_gpu.py) and of the fixture maker
(tests/golden/make_golden_painter_paint.py): the smallest shapes at which a wrong kernel still shows.  Everything is built from integer
arithmetic on index grids and a fixed multiplicative hash, so the same bytes come out everywhere; `digest` pins them in the fixture."""
import hashlib

import numpy as np


def _hash(*shape_and_salt):
    """uint32 noise over an index grid: (*shape, salt) -> [*shape]."""
    *shape, salt = shape_and_salt
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    v = (idx + np.uint64(salt) * np.uint64(0x9E3779B1)) * np.uint64(0x85EBCA6B) % np.uint64(1 << 32)
    v ^= v >> np.uint64(13)
    v = v * np.uint64(0xC2B2AE35) % np.uint64(1 << 32)
    return (v ^ (v >> np.uint64(16))).astype(np.uint32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---- semantic: 5 x 7, 37 x 53 (a row of 159 bytes: no multiple of 4) and 512 x 683 go into ONE job table
def _labels(h, w, salt, dtype):
    y, x = np.mgrid[0:h, 0:w]
    m = ((y // 9) * 7 + x // 11 + salt) % 151                     # blocks of every label 0 .. 150
    noise = _hash(h, w, salt)
    m = np.where(y < 4, noise % 151, m)                           # and rows where neighbours differ
    m = m.astype(np.int64)
    m.flat[:3] = 0, 1, 150
    m.flat[-1] = 150
    if dtype == np.int32:
        m.flat[3:5] = -1, -2147483648                             # label <= 0 paints black
    return m.astype(dtype)


def semantic_cases():
    """-> [(name, label map)]: uint8 and int32, the three sizes."""
    return [("u8_5x7", _labels(5, 7, 1, np.uint8)), ("i32_37x53", _labels(37, 53, 2, np.int32)), ("u8_512x683", _labels(512, 683, 3, np.uint8)),
            ("i32_5x7", _labels(5, 7, 4, np.int32)), ("u8_37x53", _labels(37, 53, 5, np.uint8))]


def semantic_bad_case():
    """A batch whose picture 1 holds two labels above the 150 colours."""
    good, bad = _labels(5, 7, 1, np.uint8), _labels(37, 53, 2, np.int32)
    bad[7, 9], bad[36, 52] = 151, 70000
    return [good, bad]


# panoptic: 133 categories with gaps in their ids, as COCO's have
CATEGORY_IDS = [i for i in range(1, 201) if i % 3 != 0][:133]
CATEGORY_INDEX = {c: k for k, c in enumerate(CATEGORY_IDS)}
PANOPTIC_IDS = [0, 1, 16777215, 3592, 65536, 77, 255, 256]               # 77 is listed by no segment
# (segment id, category id) in annotation order; id 3592 is listed twice: the later row wins
PANOPTIC_SEGMENTS = [(0, CATEGORY_IDS[5]), (1, CATEGORY_IDS[0]), (3592, CATEGORY_IDS[17]), (16777215, CATEGORY_IDS[132]), (65536, CATEGORY_IDS[60]),
                     (3592, CATEGORY_IDS[99]), (255, CATEGORY_IDS[1]), (256, CATEGORY_IDS[2]), (12345, CATEGORY_IDS[3])]


def _ids(h, w, salt):
    y, x = np.mgrid[0:h, 0:w]
    pick = np.where(y < 2, _hash(h, w, salt) % 8, ((y // 3) * 3 + x // 5 + salt) % 8)
    m = np.array(PANOPTIC_IDS, np.int64)[pick]
    m.flat[:3] = 0, 1, 16777215
    return m.astype(np.int32)


def id2rgb(ids):
    ids = ids.astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], -1).astype(np.uint8)


def panoptic_cases():
    """-> [(name, id map int32 [H][W] or uint8 [H][W][3], segments)]; one picture has no segment at all."""
    a, b, c = _ids(5, 7, 1), _ids(37, 53, 2), _ids(64, 33, 3)
    return [("i32_5x7", a, PANOPTIC_SEGMENTS), ("rgb_37x53", id2rgb(b), PANOPTIC_SEGMENTS), ("i32_37x53", b, PANOPTIC_SEGMENTS[:4]),
            ("rgb_5x7", id2rgb(a), PANOPTIC_SEGMENTS), ("rgb_64x33_none", id2rgb(c), [])]


# ---- instances
def _blobs(h, w, n, salt):
    """n disjoint masks: the pixels of an irregular tiling, every third pixel left as background."""
    y, x = np.mgrid[0:h, 0:w]
    gy = max(1, int(np.ceil(np.sqrt(n * h / w))))
    gx = -(-n // gy)
    jit = _hash(h, w, salt)
    cy = np.minimum((y * gy + (jit % 3).astype(np.int64) - 1).clip(0) // h, gy - 1)
    cx = np.minimum((x * gx + ((jit >> 3) % 3).astype(np.int64) - 1).clip(0) // w, gx - 1)
    owner = cy * gx + cx
    owner = np.where((jit >> 7) % 3 == 0, -1, owner)
    return np.stack([owner == m for m in range(n)]) if n else np.zeros((0, h, w), bool)


def instance_cases():
    """-> [(name, masks bool [n][H][W], disjoint)].  disjoint: the reference, which asserts it, can run the case."""
    out = []
    for h, w in ((37, 53), (64, 33), (5, 7), (480, 640)):
        for n in (0, 1, 11, 100):
            if (h, w) == (480, 640) and n in (1, 11):
                continue                                           # the large picture: the empty and the full table
            m = _blobs(h, w, n, 10 * h + n)
            if n >= 11:
                m[3] = False                                       # an empty mask among the others
                m[:, h - 1, w - 1] = False
                m[5] = False
                m[5, h - 1, w - 1] = True                          # a single pixel in the bottom-right corner
                m[7] = False
                m[:, 0, :2] = False
                m[:, 1, 0] = False
                m[7, 0, 0] = m[7, 0, 1] = m[7, 1, 0] = True        # sum x / n = 1 / 3: not exact in binary
            out.append(("n%d_%dx%d" % (n, h, w), m, True))
    z = np.zeros((3, 37, 53), bool)
    out.append(("allblack_37x53", z, True))                        # masks without a pixel: the reference's "pure black label"
    o = _blobs(37, 53, 11, 999)
    o[2, 5:30, 10:40] = True
    o[9, 20:37, 0:25] = True                                       # 2 and 9 overlap each other and the rest: the highest index wins
    out.append(("overlap_37x53", o, False))
    o = _blobs(5, 7, 4, 998)
    o[0] = True
    o[3, 1:4, 2:6] = True
    out.append(("overlap_5x7", o, False))
    return out


def geo_boxes(masks):
    """xyxy float32 boxes for `method="geo_center"`: the extent of each mask, a fixed box for an empty one."""
    n, h, w = masks.shape
    boxes = np.zeros((n, 4), np.float32)
    for m in range(n):
        ys, xs = np.nonzero(masks[m])
        boxes[m] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if len(xs) else (1, 2, 3, 5)
    return boxes


def roundtrip_masks():
    """Disjoint, non-empty masks of 64 x 96 whose cells are pairwise distinct and which cover the picture's non-background: what
    `instances(paint_instances(m))` must give back.  Every mask is a solid block of 8 x 8 pixels (64 >= the decoder's smallest area)."""
    h, w = 64, 96
    m = np.zeros((24, h, w), bool)
    for k in range(24):
        y0, x0 = 2 + (k // 6) * 16, 3 + (k % 6) * 16
        m[k, y0:y0 + 8 + k % 3, x0:x0 + 8 + k % 4] = True
    return m


# ---- pose
K = 17


def pose_boxes(W, H):
    """-> (joints float32 [5][17][3], visible float32 [5][17][3]) for a heat map of W x H:
    0 spread: mu < 5 on each axis, within 10 pixels of the right / bottom edges, fractions around .5, three invisible joints
    1 outside on all four sides: some rectangles still reach in, some only for the wide sigma, some not at all (weight 0)
    2 all joints invisible: a black picture
    3 two joints on one pixel, two more one pixel apart
    4 a cluster of spread 3: collisions everywhere"""
    j = np.zeros((5, K, 3), np.float32)
    v = np.ones((5, K, 3), np.float32)
    noise = _hash(5, K, 2, 7)
    fx, fy = (noise[..., 0] % 1000) / 1000.0, (noise[..., 1] % 1000) / 1000.0
    j[0, :, 0], j[0, :, 1] = fx[0] * (W - 1), fy[0] * (H - 1)
    j[0, :8, 0] = [0, 1.49, 2.5, 4.4, 4.5, W - 1, W - 3.5, W - 9.51]
    j[0, :8, 1] = [4.49, 0, H - 1, H - 2.5, 3.5, 2.2, H - 9.5, H - 6]
    v[0, [9, 12, 16]] = 0
    out_x = [-3, -8, -9.5, -10.49, -10.5, -20, W + 2, W + 4.4, W + 4.5, W + 8.4, W + 8.6, W + 30, W / 2, W / 3, 7, -5.5, W + 5.5]
    out_y = [H / 2, H / 3, 9, H - 9, 30.5, 40, 11, H / 2, 5, H - 4, 20, 21, -4.5, -9.49, H + 3.5, -7, H + 8.49]
    j[1, :, 0], j[1, :, 1] = out_x, out_y
    j[2, :, 0], j[2, :, 1] = fx[2] * (W - 1), fy[2] * (H - 1)
    v[2] = 0
    j[3, :, 0], j[3, :, 1] = fx[3] * (W - 1), fy[3] * (H - 1)
    j[3, 4, :2] = j[3, 11, :2] = (W / 2 + 0.25, H / 2 - 0.25)
    j[3, 6, :2], j[3, 2, :2] = (20, 30), (21, 30)
    j[4, :, 0], j[4, :, 1] = W / 2 + 3 * fx[4], H / 3 + 3 * fy[4]
    return j, v


POSE_SIZES = ((192, 256), (48, 64))                    # (W, H)


def pose_cases():
    """-> [(name, joints [B][17][3], visible [B][17][3], (W, H))]: B = 1 and 5 at both sizes."""
    out = []
    for W, H in POSE_SIZES:
        j, v = pose_boxes(W, H)
        out.append(("b1_%dx%d" % (H, W), j[:1], v[:1], (W, H)))
        out.append(("b5_%dx%d" % (H, W), j, v, (W, H)))
    return out


def input_digest():
    """One digest over every input of this file."""
    parts = [m for _, m in semantic_cases()] + semantic_bad_case() + [m for _, m, _ in panoptic_cases()]
    parts += [m for _, m, _ in instance_cases()] + [roundtrip_masks()]
    for _, j, v, _ in pose_cases():
        parts += [j, v]
    return digest(*parts)
