"""How many (block, branch, sample) units the seeded steps of bench.py really drop (DropPath factor 0), i.e. how much attention / MLP branch
work DropPath skipping removes from them -- the number to set the per-family times of a kernel profile against.

    python tools/droppath_units.py [--steps 20] [--warmup 3] [--batch 8]

Replays bench.py's draws: torch.manual_seed(1234) (rank 0), then one models_painter.Painter._drop_scales() call per step, warm-up steps
included.  Needs the GPU (the draws come from the device generator); the model itself stays on the host."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import models_painter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
model = models_painter.painter_vit_large_patch16_input896x448_win_dec64_8glb_sl1(compute_dtype="bf16").train()
torch.manual_seed(1234)
total = sum((2 * args.batch if i <= model._cfg.merge_idx else args.batch) * 2 for i in range(len(model.blocks)))
expect = sum((2 * args.batch if i <= model._cfg.merge_idx else args.batch) * 2 * float(b.drop_path_prob) for i, b in enumerate(model.blocks))
rows = []
for s in range(args.warmup + args.steps):
    ds = model._drop_scales(args.batch, dev)
    a = sum(int((p[0] == 0).sum()) for p in ds if p[0] is not None)
    m = sum(int((p[1] == 0).sum()) for p in ds if p[1] is not None)
    rows.append((a, m))
    print("step %2d%s: attention branch %2d  MLP branch %2d  of %d units each" % (s, " (warm-up)" if s < args.warmup else "", a, m, total // 2))
timed = rows[args.warmup:]
ta, tm = sum(r[0] for r in timed) / len(timed), sum(r[1] for r in timed) / len(timed)
aa, am = sum(r[0] for r in rows) / len(rows), sum(r[1] for r in rows) / len(rows)
print("timed steps : attention %.2f (%.2f %%)  MLP %.2f (%.2f %%)  both %.2f of %d units (%.2f %%)"
      % (ta, 200 * ta / total, tm, 200 * tm / total, ta + tm, total, 100 * (ta + tm) / total))
print("all steps   : attention %.2f (%.2f %%)  MLP %.2f (%.2f %%)  both %.2f of %d units (%.2f %%)"
      % (aa, 200 * aa / total, am, 200 * am / total, aa + am, total, 100 * (aa + am) / total))
print("expectation : %.2f of %d units (%.2f %%)" % (expect, total, 100 * expect / total))
