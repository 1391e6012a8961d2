"""The training step (ViT-L 896 x 448, B = 8, bf16, train mode) with the masks real training draws, for the A/B of the live-row decoder
backward (pa_debug_set knob 17).  bench.py's bottom-half mask is the favourable case: its live rows are contiguous.

    python tools/decoder_rows_ab.py {on|off} [--mask block|half] [--steps 20] [--warmup 3] [--seed 7]

One process = one setting; alternate fresh processes for an A/B.  --mask block: every sample gets its own mask from
painter_amd.masking_generator with train_painter_vit_large.sh's settings (784 of 1568 patches, blocks of 16 .. 392), seeded.  Prints
`label ms_per_step live_rows`."""
import argparse
import random
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from painter_amd import models_painter, ops  # noqa: E402
from painter_amd.masking_generator import MaskingGenerator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("switch", choices=["on", "off"])
    ap.add_argument("--mask", default="block", choices=["block", "half"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda")
    ops.decoder_rows(2 if a.switch == "on" else 1)
    m = models_painter.painter_vit_large_patch16_input896x448(compute_dtype="bf16")
    bench.randomize_parameters(m, seed=1)
    m = m.to(dev).train()
    c = m._cfg
    imgs, tgts, mask, valid = bench.synthetic_inputs(8, c.H, c.W, c.L, 1234, dev)
    if a.mask == "block":
        random.seed(a.seed)
        np.random.seed(a.seed)
        g = MaskingGenerator((c.Hp, c.Wp), c.L // 2, min_num_patches=16, max_num_patches=c.L // 4)
        mask = torch.from_numpy(np.stack([g() for _ in range(8)])).to(dev).reshape(mask.shape).to(mask.dtype)
    _, _, count = ops.live_rows(mask.reshape(8, c.L).to(torch.uint8).contiguous(), 8, c.Hp, c.Wp)
    torch.manual_seed(1234)

    def step():
        for p in m.parameters():
            p.grad = None
        loss, _, _ = m(imgs, tgts, bool_masked_pos=mask, valid=valid)
        loss.backward()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    print("%s_%s %.3f %d" % (a.mask, a.switch, e0.elapsed_time(e1) / a.steps, int(count.item())), flush=True)


if __name__ == "__main__":
    main()
