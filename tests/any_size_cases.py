"""The cases of the any-input-size fixtures (tests/golden/painter_any_size*.npz): a model built at one size, run at another (not a test).
Shared by tests/golden/make_golden_any_size.py, tests/test_any_size_cpu.py and tests/test_any_size_gpu.py, so that the fixtures hold only
seeds and outputs."""
import dataclasses

from oracle import painter_oracle as O

BATCH = 2
FP32_GATE = 1e-3          # the project's north-star gate: worst relative error of the fp32 build against the unmodified reference

# name -> (what the model is built as, parameter seed, input seed, (H, W) of the run, the fixture file that holds the fp32 pred)
CASES = {
    "A": ("small", 51, 61, (160, 80), "painter_any_size.npz"),         # 10 x 5: odd Wp, an 18-key tail tile
    "B": ("small", 52, 62, (96, 48), "painter_any_size.npz"),          # 6 x 3: L = 18 < 32, the tables shrink
    "C": ("small", 53, 63, (192, 96), "painter_any_size.npz"),         # 12 x 6: Wp % 4 != 0
    "D": ("small", 54, 64, (256, 128), "painter_any_size_df.npz"),     # 16 x 8: an aligned grid -- the existing kernels, resized tables only
    "F": ("h14", 55, 65, (140, 70), "painter_any_size_df.npz"),        # 10 x 5 at patch 14, head_dim 80, built at (112, 56)
}
BF16_FILE = "painter_any_size_bf16.npz"


def config(name):
    """The OracleConfig the case's model is BUILT with."""
    return O.small_config() if CASES[name][0] == "small" else O.h14_small_config(depth=24)


def run_config(name):
    """The same with the run-time size as img_size: what O.synthetic_batch needs to draw the inputs (never used to draw parameters)."""
    return dataclasses.replace(config(name), img_size=CASES[name][3])


def inputs(name):
    """-> (imgs, tgts, mask int32 [B, L], valid) at the run-time size, bottom-half mask."""
    return O.synthetic_batch(run_config(name), BATCH, CASES[name][2], "half")
