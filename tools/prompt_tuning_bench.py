"""In-context (prompt) tuning cost: SegGPT ViT-L 896 x 448, bf16, train mode, N = 8, frozen model, learnable prompt image / target pair
(the top half of every sample's imgs / tgts) -- forward + backward per step, against an ordinary training step (every parameter trainable,
forward + backward, as bench.py times it) in the same process, and pa_patch_embed_dgrad alone at that shape.  Prints one JSON line.

    python tools/prompt_tuning_bench.py [--steps 20] [--warmup 5] [--only tune|train|kernel]

Under `rocprofv3 --kernel-trace --stats -- python tools/prompt_tuning_bench.py --only tune --steps 2 --warmup 1` the frozen step shows no
weight-gradient GEMM, no conv3x3_wgrad and none of the parameter-gradient reductions."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from painter_amd import models_seggpt, ops  # noqa: E402


def lib_sha16():
    with open(os.path.join(ROOT, "painter_amd", "lib", "libpainter_hip.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--only", choices=("tune", "train", "kernel"), default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    m = models_seggpt.seggpt_vit_large_patch16_input896x448(compute_dtype="bf16").cuda().train()
    N, (H, W) = a.n, (m._cfg.H, m._cfg.W)
    g = torch.Generator(device="cuda").manual_seed(1)
    imgs = torch.randn(N, 3, H, W, device="cuda", generator=g)
    tgts = torch.randn(N, 3, H, W, device="cuda", generator=g)
    L = m.patch_embed.num_patches
    mask = torch.zeros(1, L, device="cuda")
    mask[:, L // 2:] = 1
    valid = torch.ones_like(tgts)
    seg_type = torch.ones(N, 1, device="cuda")
    out = {"metric": "prompt_tuning", "model": "seggpt_vit_large_patch16_input896x448", "n": N, "dtype": "bf16", "mode": "train",
           "steps": a.steps, "warmup": a.warmup, "build": {"lib_sha16": lib_sha16()}}

    if a.only in (None, "train"):
        def train_step():
            for p in m.parameters():
                p.grad = None
            m._hot.relpos_stale()
            loss, _, _ = m(imgs, tgts, mask, valid, seg_type, -1)
            loss.backward()
        out["train_step_ms"] = timed(train_step, a.steps, a.warmup)

    if a.only in (None, "tune"):
        for p in m.parameters():
            p.grad = None
            p.requires_grad_(False)
        prompt = torch.stack([imgs[0, :, :H // 2], tgts[0, :, :H // 2]]).clone().requires_grad_(True)
        q_img, q_tgt = imgs[:, :, H // 2:], tgts[:, :, H // 2:]

        def tune_step():
            prompt.grad = None
            xi = torch.cat([prompt[0].expand(N, -1, -1, -1), q_img], dim=2)
            xt = torch.cat([prompt[1].expand(N, -1, -1, -1), q_tgt], dim=2)
            loss, _, _ = m(xi, xt, mask, valid, seg_type, -1)
            loss.backward()
        out["tune_step_ms"] = timed(tune_step, a.steps, a.warmup)

    if a.only in (None, "kernel"):
        c = m._cfg
        dpe = (torch.randn(2 * N * c.L, c.D, device="cuda", generator=g) * 1e-2).to(torch.bfloat16)
        w = m._hot.w_patch(dict(m.named_parameters()))
        add = torch.randn_like(tgts)
        out["patch_embed_dgrad_us"] = 1e3 * timed(lambda: ops.patch_embed_dgrad(dpe, w, N, c.Hp, c.Wp, c.P, c.D, addend=add), 50, 5)
    if "train_step_ms" in out and "tune_step_ms" in out:
        out["tune_over_train"] = out["tune_step_ms"] / out["train_step_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
