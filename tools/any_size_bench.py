"""Measure the forward at a run-time input size other than the constructed one on one MI355X, one process, the two timed
variants of every comparison alternating, medians of >= 20 runs with the spread:

  (a) attention alone -- pa_attn_any_fwd at 70 x 35 tokens (1120 x 560: Painter/eval/coco_panoptic/eval.sh), ViT-L heads, B = 8, bf16,
      against the design it replaces: the existing forward (ops.attn_fwd, reported by kernel family) on the grid PADDED to 72 x 36.  The
      native kernel must not be slower, or padding would have been the cheaper design.  Its rate per (query, key) pair is printed beside
      generation 3 at the constructed 56 x 28.
  (b) the whole model -- the ViT-L forward at 1120 x 560, B = 1 and 8, bf16, against the oracle's torch op sequence under bf16 autocast
      on the same GPU.  Reported only.

    python tools/any_size_bench.py [--runs 20 --iters 5 --skip-model] -> lines per comparison, then one JSON line

--grad measures the BACKWARD at that size instead, same conventions:
  (a) attention backward alone -- pa_attn_any_bwd (Delta, dQ + dG, dK / dV, table contraction) at 70 x 35, B = 8, 16 heads, bf16, beside
      the existing backward (ops.attn_bwd, reported by kernel family) on the grid padded to 72 x 36 -- another function, a cost yardstick
      only, and one pa_attn_bwd may refuse (its dK / dV kernel's table tile ends at Hp + Wp = 94 for head_dim 64): the refusal is then
      what the log records -- and beside the existing backward at the constructed 56 x 28, by its rate per (query, key) pair.
  (b) the ViT-L forward + backward at 1120 x 560 (grad_at_any_size), bf16, B = 1 and the largest B of 8, 4, 2 that fits, beside the
      oracle's torch op sequence under bf16 autocast with autograd on the same GPU.  Reported only.

(c), the bench.py line against the parent commit, needs the parent's tree and is taken by alternating fresh processes of the two trees;
its log is filed beside this one."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import painter_oracle as O                          # noqa: E402
from painter_amd import models_painter, ops, ops_anysize        # noqa: E402

BF16 = torch.bfloat16


def events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternate(legs, runs, iters):
    """legs: {name: fn}.  Every leg warmed up, then `runs` rounds in which the legs take turns -> {name: dict(median, min, max)} in ms."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            t[k].append(events_ms(fn, iters))
    return {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in t.items()}


def operands(B, H, Hp, Wp, hd=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    L = Hp * Wp
    qkv = torch.randn((B * L, 3 * H * hd), generator=g).to(BF16).cuda()
    rel_h = (0.2 * torch.randn((2 * Hp - 1, hd), generator=g)).cuda()
    rel_w = (0.2 * torch.randn((2 * Wp - 1, hd), generator=g)).cuda()
    return qkv, ops.relpos_pack(rel_h, rel_w, Hp, Wp, BF16)


def attention(runs, iters, B=8, H=16):
    scale = 0.125
    q_any, r_any = operands(B, H, 70, 35)
    q_pad, r_pad = operands(B, H, 72, 36)
    q_g3, r_g3 = operands(B, H, 56, 28)
    c0 = ops.attn_launch_counts()["fwd"]
    ops.attn_fwd(q_pad, r_pad, B, 72 * 36, H, 72, 36, scale)
    c1 = ops.attn_launch_counts()["fwd"]
    ops.attn_fwd(q_g3, r_g3, B, 56 * 28, H, 56, 28, scale)
    c2 = ops.attn_launch_counts()["fwd"]
    family = lambda a, b: ("generation 1", "generation 2", "generation 3")[[y - x for x, y in zip(a, b)].index(1)]
    legs = {"attn_any_70x35": lambda: ops_anysize.attn_any_fwd(q_any, r_any, B, 2450, H, 70, 35, scale),
            "attn_fwd_padded_72x36": lambda: ops.attn_fwd(q_pad, r_pad, B, 2592, H, 72, 36, scale),
            "attn_fwd_56x28": lambda: ops.attn_fwd(q_g3, r_g3, B, 1568, H, 56, 28, scale)}
    res = alternate(legs, runs, iters)
    pairs = {"attn_any_70x35": B * H * 2450 ** 2, "attn_fwd_padded_72x36": B * H * 2450 ** 2, "attn_fwd_56x28": B * H * 1568 ** 2}
    for k, v in res.items():
        v["useful_pairs_per_ns"] = round(pairs[k] / (v["median"] * 1e6), 2)          # (the padded leg: the 70 x 35 pairs it was run for)
    res["attn_fwd_padded_72x36"]["kernels"], res["attn_fwd_56x28"]["kernels"] = family(c0, c1), family(c1, c2)
    a, p = res["attn_any_70x35"], res["attn_fwd_padded_72x36"]
    res["native_over_padded_median"] = round(a["median"] / p["median"], 3)
    res["native_not_slower_beyond_the_spread"] = bool(a["median"] <= p["median"] or a["min"] <= p["max"])
    return res


def attention_bwd(runs, iters, B=8, H=16):
    scale = 0.125
    legs, res_extra = {}, {}
    for name, (Hp, Wp) in (("attn_any_bwd_70x35", (70, 35)), ("attn_bwd_padded_72x36", (72, 36)), ("attn_bwd_56x28", (56, 28))):
        L = Hp * Wp
        g = torch.Generator().manual_seed(3)
        qkv = torch.randn((B * L, 3 * H * 64), generator=g).to(BF16).cuda()
        dout = torch.randn((B * L, H * 64), generator=g).to(BF16).cuda()
        rel_h, rel_w = (0.2 * torch.randn((2 * Hp - 1, 64), generator=g)).cuda(), (0.2 * torch.randn((2 * Wp - 1, 64), generator=g)).cuda()
        rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, BF16), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, BF16)
        if name.startswith("attn_any"):
            out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)
            legs[name] = lambda a=(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale): ops_anysize.attn_any_bwd(*a)
            continue
        out, lse, tables = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale, need_tables=True)
        c0 = ops.attn_launch_counts()["bwd"]
        try:
            ops.attn_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale, tables=tables)
        except RuntimeError as e:          # (72 x 36: the generic dK / dV kernel's table tile holds Hp + Wp <= 94 at head_dim 64)
            res_extra[name] = {"refused": str(e)}
            continue
        c1 = ops.attn_launch_counts()["bwd"]
        res_extra[name] = {"kernels": ("generation 1", "generation 2", "generation 3")[[y - x for x, y in zip(c0, c1)].index(1)]}
        legs[name] = lambda a=(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale), t=tables: ops.attn_bwd(*a, tables=t)
    res = alternate(legs, runs, iters)
    pairs = {"attn_any_bwd_70x35": B * H * 2450 ** 2, "attn_bwd_padded_72x36": B * H * 2450 ** 2, "attn_bwd_56x28": B * H * 1568 ** 2}
    for k, v in res.items():
        v["useful_pairs_per_ns"] = round(pairs[k] / (v["median"] * 1e6), 2)
    for k, v in res_extra.items():
        res.setdefault(k, {}).update(v)
    if "median" in res.get("attn_bwd_padded_72x36", {}):
        res["native_over_padded_median"] = round(res["attn_any_bwd_70x35"]["median"] / res["attn_bwd_padded_72x36"]["median"], 3)
    return res


def model_grad(runs, iters, batches=(1, 8)):
    cfg = O.vit_large_config()
    run = dataclasses.replace(cfg, img_size=(1120, 560))
    m = models_painter.painter_vit_large_patch16_input896x448_win_dec64_8glb_sl1(compute_dtype="bf16")
    P = O.random_params(cfg, 1)
    m.load_state_dict(P, strict=True)
    m = m.cuda().eval().grad_at_any_size(True)
    Pd = {k: v.cuda().requires_grad_(True) for k, v in P.items()}
    out = {}
    for B in batches:
        while B > 1:                                    # the largest batch at which both legs fit
            try:
                imgs, tgts, mask, valid = (t.cuda() for t in O.synthetic_batch(run, B, 2, "half"))
                with torch.autocast("cuda", dtype=BF16):
                    O.forward(Pd, cfg, imgs, tgts, mask, valid.clone())[0].backward()
                break
            except torch.cuda.OutOfMemoryError:
                B //= 2
                torch.cuda.empty_cache()
        imgs, tgts, mask, valid = (t.cuda() for t in O.synthetic_batch(run, B, 2, "half"))
        mb = mask.reshape(B, 70, 35)

        def ours():
            m.zero_grad(set_to_none=True)
            m(imgs, tgts, bool_masked_pos=mb, valid=valid)[0].backward()

        def oracle():
            for p in Pd.values():
                p.grad = None
            with torch.autocast("cuda", dtype=BF16):
                loss = O.forward(Pd, cfg, imgs, tgts, mask, valid.clone())[0]
            loss.backward()
        res = alternate({"painter_amd_ms": ours, "torch_ops_bf16_autocast_ms": oracle}, runs, iters if B == 1 else 1)
        res["speedup_median"] = round(res["torch_ops_bf16_autocast_ms"]["median"] / res["painter_amd_ms"]["median"], 2)
        out["B%d" % B] = res
        print("model forward + backward 1120x560 B=%d: %s" % (B, json.dumps(res)), flush=True)
    return out


def model(runs, iters, batches=(1, 8)):
    cfg = O.vit_large_config()
    run = dataclasses.replace(cfg, img_size=(1120, 560))
    m = models_painter.painter_vit_large_patch16_input896x448_win_dec64_8glb_sl1(compute_dtype="bf16")
    P = O.random_params(cfg, 1)
    m.load_state_dict(P, strict=True)
    m = m.cuda().eval()
    Pd = {k: v.cuda() for k, v in P.items()}
    out = {}
    for B in batches:
        imgs, tgts, mask, valid = (t.cuda() for t in O.synthetic_batch(run, B, 2, "half"))
        mb = mask.reshape(B, 70, 35)

        def ours():
            with torch.no_grad():
                m(imgs, tgts, bool_masked_pos=mb, valid=valid)

        def oracle():
            with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
                O.forward(Pd, cfg, imgs, tgts, mask, valid.clone())
        res = alternate({"painter_amd_ms": ours, "torch_ops_bf16_autocast_ms": oracle}, runs, iters if B == 1 else max(1, iters // 2))
        res["speedup_median"] = round(res["torch_ops_bf16_autocast_ms"]["median"] / res["painter_amd_ms"]["median"], 2)
        out["B%d" % B] = res
        print("model 1120x560 B=%d: %s" % (B, json.dumps(res)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--grad", action="store_true", help="the backward at that size (DESIGN.md 4.22) instead of the forward")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("any_size_bench: needs the MI355X (nothing here is measured on a CPU)")
    assert a.runs >= 20, "medians of at least 20 runs"
    summary = {"what": "forward at 1120 x 560 on the 896 x 448 ViT-L (70 x 35 tokens)", "device": torch.cuda.get_device_name(0),
               "runs": a.runs, "iters": a.iters}
    if a.grad:
        summary["what"] = "forward + backward at 1120 x 560 on the 896 x 448 ViT-L (70 x 35 tokens)"
        summary["attention_bwd_B8_H16_bf16_ms"] = attention_bwd(a.runs, a.iters)
        print("attention backward: %s" % json.dumps(summary["attention_bwd_B8_H16_bf16_ms"]), flush=True)
        if not a.skip_model:
            summary["model_fwd_bwd_bf16"] = model_grad(a.runs, a.iters)
        print(json.dumps(summary))
        return
    summary["attention_B8_H16_bf16_ms"] = attention(a.runs, a.iters)
    print("attention: %s" % json.dumps(summary["attention_B8_H16_bf16_ms"]), flush=True)
    if not a.skip_model:
        summary["model_bf16"] = model(a.runs, a.iters)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
