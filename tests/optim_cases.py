"""Shared pieces of the optimizer kernel tests (tests/test_optim_kernels_gpu.py, tests/test_optim_cpu.py) -- a plain helper module.

Reference: torch.optim.AdamW(foreach=False) + torch.nn.utils.clip_grad_norm_ on float64 CPU copies of the same fp32 inputs; the
gradients are divided by the loss scale in float64.  Nothing of the arithmetic is restated here.

Yardstick: the very same loop on fp32 CPU copies, i.e. what torch's own fp32 AdamW loses against float64 on these inputs.  It is
recomputed on every run (deterministic, milliseconds at these sizes).

Error measure: max|a - b| / max|b|, per tensor and per quantity (parameter, exp_avg, exp_avg_sq).
Gate of a case, per quantity: 2 x the largest yardstick error of that quantity over the case's tensors, never below 2^-22.
  factor 2: the kernel's fp32 operation order (fma contraction, reciprocal square root of the bias correction, unscale and clip
            folded into one factor) is as valid as torch's but not the same;
  floor:    two ulps (2 x 2^-23) of the tensor's largest entry -- what two differently rounded fp32 results can differ by.
"""
import torch

FLOOR = 2.0 ** -22
GUARD = 1.0e30                       # fills the elements between the views of a flat buffer
QUANTITIES = ("p", "exp_avg", "exp_avg_sq")
LENGTHS = (1, 3, 4, 5, 8191, 8192, 8193, 16385)          # a chunk is 8192 elements: tails, exact chunks, a second chunk
# element offsets mod 4 of the views of (p, g, m, v) in their flat buffers, one residue per tensor (cycled)
ALIGN_CLASSES = {
    "none": dict(p=(0,), g=(0,), m=(0,), v=(0,)),
    "g": dict(p=(0,), g=(3, 1, 2), m=(0,), v=(0,)),                      # what a flattened gradient bucket produces
    "p": dict(p=(1, 2, 3), g=(0,), m=(0,), v=(0,)),
    "mv": dict(p=(0,), g=(0,), m=(2, 3, 1), v=(3, 1, 2)),
    "all": dict(p=(1, 2, 3), g=(2, 3, 1), m=(3, 1, 2), v=(1, 3, 3)),
}
# the decoder_pred bucket in the order the engine hands it to the gradient all-reduce: (name, elements)
DECODER_PRED_BUCKET = (("decoder_pred.1.weight", 64), ("decoder_pred.1.bias", 64), ("decoder_pred.3.weight", 192),
                       ("decoder_pred.3.bias", 3), ("decoder_pred.0.weight", 36864), ("decoder_pred.0.bias", 64))


# ---------------------------------------------------------------------------------------------------------------- layouts
def flat_layout(lengths, residues, gap=4):
    """Element offsets of views of the given lengths in one flat buffer: view i starts at an offset = residues[i % len] mod 4, at least
    `gap` guard elements lie before, between and after the views.  -> (offsets, total elements)."""
    offs, pos = [], gap
    for i, n in enumerate(lengths):
        pos += (residues[i % len(residues)] - pos) % 4
        offs.append(pos)
        pos += n + gap
    return offs, pos


def guarded_views(lengths, residues, device="cpu", fill=GUARD):
    """-> (flat fp32 buffer filled with `fill`, its views per flat_layout, bool mask of the guard elements)."""
    offs, total = flat_layout(lengths, residues)
    buf = torch.full((total,), fill, dtype=torch.float32, device=device)
    guard = torch.ones(total, dtype=torch.bool, device=device)
    views = []
    for o, n in zip(offs, lengths):
        views.append(buf[o:o + n])
        guard[o:o + n] = False
    return buf, views, guard


def bucket_views(tensors):
    """Flatten a bucket of gradients the way the gradient all-reduce does: one torch.cat message, the tensors replaced by views."""
    flat = torch.cat([t.reshape(-1) for t in tensors])
    views, off = [], 0
    for t in tensors:
        views.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    return flat, views


def painter_shaped_groups(depth=24, cap=20000, base_lr=1e-3, layer_decay=0.75, weight_decay=0.05):
    """Parameter names and ranks of the small Painter configuration at `depth`, every tensor cut to at most `cap` elements (the cut
    sizes walk through the four residues mod 4), sorted into layer-decay groups: layer id 0 for everything in front of the blocks,
    i + 1 for `blocks.<i>.`, depth + 1 for the rest; one-dimensional tensors are not decayed.
    -> (names, sizes, group index per tensor, [(lr, weight_decay)] per group)."""
    from oracle import painter_oracle as O
    import dataclasses
    shapes = O.param_shapes(dataclasses.replace(O.small_config(), depth=depth))
    names, sizes, gidx, groups, key_of = [], [], [], [], {}
    ncut, seen_blocks = 0, False
    for name, shape in shapes.items():
        n = 1
        for s in shape:
            n *= s
        if n > cap:
            n, ncut = cap - ncut % 4, ncut + 1
        if name.startswith("blocks."):
            layer, seen_blocks = int(name.split(".")[1]) + 1, True
        else:
            layer = depth + 1 if seen_blocks else 0
        decay = len(shape) > 1
        key = (layer, decay)
        if key not in key_of:
            key_of[key] = len(groups)
            groups.append((base_lr * layer_decay ** (depth + 1 - layer), weight_decay if decay else 0.0))
        names.append(name)
        sizes.append(n)
        gidx.append(key_of[key])
    return names, sizes, gidx, groups


# ---------------------------------------------------------------------------------------------------------------- reference
def torch_adamw_loop(params, group_of, groups, steps, *, dtype, betas=(0.9, 0.95), eps=1e-8, scale=1.0, max_norm=None):
    """torch.optim.AdamW(foreach=False) driven like the training loop drives it, on CPU copies of `params` in `dtype`.
    params: fp32 tensors; group_of[i]: group index of tensor i; groups: [(lr, weight_decay)].
    steps: one entry per step, dict(grads=[fp32 tensor or None per parameter, still multiplied by `scale`],
                                    skip=bool (the scaler found inf/nan: no update), lrs=[lr per group] or None).
    -> dict(p=[...], exp_avg=[...], exp_avg_sq=[...], step=[float per parameter]) in `dtype`."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    pg = [{"params": [ps[i] for i in range(len(ps)) if group_of[i] == gi], "lr": lr, "weight_decay": wd} for gi, (lr, wd) in enumerate(groups)]
    slots = [gi for gi, g in enumerate(pg) if g["params"]]                  # torch refuses an empty group
    opt = torch.optim.AdamW([pg[gi] for gi in slots], lr=1e-3, betas=betas, eps=eps, foreach=False)
    for st in steps:
        if st.get("lrs") is not None:
            for k, gi in enumerate(slots):
                opt.param_groups[k]["lr"] = st["lrs"][gi]
        if st.get("skip"):
            continue
        for p, g in zip(ps, st["grads"]):
            p.grad = None if g is None else g.detach().cpu().to(dtype) / scale
        live = [p for p in ps if p.grad is not None]
        if max_norm is not None and live:
            torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False)
        opt.step()
    out = {"p": [p.detach() for p in ps], "exp_avg": [], "exp_avg_sq": [], "step": []}
    for p in ps:
        s = opt.state.get(p, {})
        out["exp_avg"].append(s["exp_avg"] if s else torch.zeros_like(p.detach()))
        out["exp_avg_sq"].append(s["exp_avg_sq"] if s else torch.zeros_like(p.detach()))
        out["step"].append(float(s["step"]) if s else 0.0)
    return out


def rel_err(a, b):
    """max|a - b| / max|b| in float64 (the absolute error where b is all zero)."""
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    if a.numel() == 0:
        return 0.0
    d, s = float((a - b).abs().max()), float(b.abs().max())
    return d / s if s > 0 else d


def reference_and_gates(params, group_of, groups, steps, **kw):
    """-> (float64 result, {quantity: gate}, {quantity: yardstick}): the float64 loop, and the gates from the fp32 loop's own error."""
    ref = torch_adamw_loop(params, group_of, groups, steps, dtype=torch.float64, **kw)
    f32 = torch_adamw_loop(params, group_of, groups, steps, dtype=torch.float32, **kw)
    yard = {q: max(rel_err(a, b) for a, b in zip(f32[q], ref[q])) for q in QUANTITIES}
    return ref, {q: max(2.0 * yard[q], FLOOR) for q in QUANTITIES}, yard


def check_against(label, got, ref, gates, yard):
    """got: dict like torch_adamw_loop's with the device results.  Prints the device error next to the yardstick, then asserts."""
    errs = {q: max(rel_err(a, b) for a, b in zip(got[q], ref[q])) for q in QUANTITIES}
    print("%s: " % label + "; ".join("%s device %.3e yardstick %.3e gate %.3e" % (q, errs[q], yard[q], gates[q]) for q in QUANTITIES))
    for q in QUANTITIES:
        worst = max(range(len(ref[q])), key=lambda i: rel_err(got[q][i], ref[q][i]))
        assert errs[q] <= gates[q], "%s: %s of tensor %d is off by %.3e (gate %.3e, yardstick %.3e)" % (label, q, worst, errs[q], gates[q], yard[q])
    if "step" in got:
        assert [float(s) for s in got["step"]] == ref["step"], (label, got["step"], ref["step"])
    return errs
