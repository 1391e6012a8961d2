"""Shared inputs of the class-agnostic instance decode tests: the synthetic painted pictures and the case lists.  TEST INFRASTRUCTURE.

A picture is what the `coco_pano_inst` task paints: every object filled with the colour of its location (the 4 x 4 global cell of its
centre, then the 20 x 20 local cell inside it), on black, then blurred and disturbed by Gaussian noise as a network's output is."""
import numpy as np

K = 6400                                  # colours of the default palette (16 global cells x 20 x 20 local cells)


def painted_picture(seed, h, w, n_obj=14, blur=1, noise=3.0):
    """-> uint8 [h][w][3].  Ellipses painted back to front in their location's colour, a (2 blur + 1)^2 box blur, noise, rounding."""
    from painter_amd.painter_engine import location_palette
    pal = location_palette()
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), np.float64)
    for _ in range(n_obj):
        cy, cx = rng.uniform(0.05, 0.95) * h, rng.uniform(0.05, 0.95) * w
        ry, rx = rng.uniform(0.06, 0.25) * h, rng.uniform(0.06, 0.25) * w
        gy, gx = int(cy * 4 / h), int(cx * 4 / w)
        ly, lx = int((cy * 4 / h - gy) * 20), int((cx * 4 / w - gx) * 20)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        img[inside] = pal[(gy * 4 + gx) * 400 + ly * 20 + lx]
    if blur:
        k = 2 * blur + 1
        pad = np.pad(img, ((blur, blur), (blur, blur), (0, 0)), mode="edge")
        img = sum(pad[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)) / (k * k)
    img = img + rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ---- the fixture's cases (tests/golden/painter_inst.npz): name -> (seed, height, width, thresholds, generator arguments).  Each was
# kept only because the unmodified reference and the host restatement agree on it mask for mask and its cuts are not ties
# (tests/golden/make_golden_painter_inst.py asserts it; its --search mode found the tie-heavy two).
FIXTURE = {
    "thr19_a": (1, 96, 128, [19.0], {}),
    "thr19_b": (2, 120, 160, [19.0], {}),
    "thr19_c": (3, 61, 83, [19.0], {}),                                               # 5063 pixels: no multiple of 32 or 64
    "thr10_19": (101, 72, 96, [10.0, 19.0], dict(n_obj=8)),
    "many": (5, 96, 128, [19.0], {}),                                                 # 3903 candidates: the nms_pre cut is active
    "few": (101, 60, 80, [5.0], dict(n_obj=28, blur=0, noise=1.5)),                   # 169 candidates
}

# ---- cases of the GPU tests against the host restatement alone (ties included): name -> (seed, h, w, thresholds, nms_pre, max_num)
DECODE = {
    "ties_thr5": (11, 60, 80, [5.0], 2000, 100),
    "ties_two_thr": (12, 48, 64, [10.0, 19.0], 2000, 100),
    "odd_size": (13, 61, 83, [19.0], 2000, 100),               # 5063 pixels: no multiple of 32 or 64
    "odd_caps": (14, 72, 96, [19.0], 300, 7),                   # caps that are no multiple of any tile
}


def fixture_picture(name):
    s, h, w, _, kw = FIXTURE[name]
    return painted_picture(s, h, w, **kw)


def decode_picture(name):
    s, h, w = DECODE[name][:3]
    return painted_picture(s, h, w)
