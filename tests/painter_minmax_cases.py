"""Shared inputs of the nearest-colour (minmax) instance decode tests.  TEST INFRASTRUCTURE.

The painted pictures are those of tests/painter_inst_cases.py; the constructed ones below aim at ties, the score's `max(., 1)` branch,
the palette capacity and sums beyond 2^24 / 2^32."""
import numpy as np

from tests.painter_inst_cases import painted_picture

# ---- the fixture's cases (tests/golden/painter_minmax.npz): name -> (seed, height, width, generator arguments): the same pictures as
# painter_inst_cases.FIXTURE under these names.  Each was kept only because the unmodified reference and the host statement agree on it
# in every stored array and its largest S_c is below 2^24 (tests/golden/make_golden_painter_minmax.py asserts both).
FIXTURE = {
    "thr19_a": (1, 96, 128, {}),                                                      # has pixels with a tied minimum
    "thr19_c": (3, 61, 83, {}),                                                       # 5063 pixels: no multiple of 32 or 64
    "few": (101, 60, 80, dict(n_obj=28, blur=0, noise=1.5)),
}

# ---- cases of the GPU tests against the host statement alone: name -> (seed, height, width, generator arguments)
DECODE = {
    "odd_37x53": (31, 37, 53, {}),                                                    # 1961 pixels: less than one statistics chunk
    "two_blocks_33x65": (32, 33, 65, dict(noise=6.0)),                                # 2145 pixels: one pixel row past 2048, very noisy
    "tile_64x64": (33, 64, 64, dict(n_obj=5)),                                        # 4096 pixels: whole blocks only
}


def fixture_picture(name):
    s, h, w, kw = FIXTURE[name]
    return painted_picture(s, h, w, **kw)


def decode_picture(name):
    s, h, w, kw = DECODE[name]
    return painted_picture(s, h, w, **kw)


def ties_case():
    """8 x 8 picture, palette of 4 rows + background with rows 1 and 3 equal, pixels equidistant between a row and black, between two rows,
    and exactly on the duplicated row.  -> (picture, palette with the background row)"""
    pal = np.array([[200, 100, 50], [40, 40, 40], [10, 250, 10], [40, 40, 40], [0, 0, 0]], np.float32)
    pic = np.zeros((8, 8, 3), np.uint8)
    pic[0] = (40, 40, 40)                        # rows 1 and 3 at distance 0: row 1
    pic[1] = (20, 20, 20)                        # 60 from rows 1 / 3 and 60 from black: row 1
    pic[2] = (100, 50, 25)                       # 175 from row 0 and 175 from black (115 from rows 1 / 3: they win)
    pic[3] = (30, 0, 30)                         # 60 from black, 60 from rows 1 / 3: row 1
    pic[4] = (120, 70, 45)                       # 115 from row 0; rows 1 / 3: 80 + 30 + 5 = 115: row 0 wins the tie
    pic[5, :4] = (5, 125, 5)                     # 135 from black, 135 from row 2: row 2
    pic[5, 4:] = (0, 0, 1)
    pic[6] = (41, 39, 40)
    pic[7, ::2] = (20, 20, 20)                   # alternating labels inside a wave
    pic[7, 1::2] = (255, 255, 255)
    return pic, pal


def exact_colours_case(palette, seed=5, h=24, w=40):
    """A picture of exact palette colours (every distance 0, so every score is exactly 1).  palette: with the background row."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(palette), 7, replace=False)
    idx = rows[rng.integers(0, len(rows), (h // 4, w // 4))].repeat(4, 0).repeat(4, 1)
    return np.asarray(palette)[idx].astype(np.uint8)


def capacity_case(seed=6):
    """16 x 16 picture and a random palette at the capacity: 16383 rows + background.  -> (picture, palette with the background row)"""
    rng = np.random.default_rng(seed)
    pal = np.concatenate([rng.integers(0, 256, (16383, 3)), np.zeros((1, 3), np.int64)]).astype(np.float32)
    pic = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    pic[0, :8] = pal[16382].astype(np.uint8)     # the last row before the background and the background itself are reached
    pic[1, :8] = 0
    return pic, pal
