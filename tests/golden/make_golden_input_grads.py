"""Generate tests/golden/input_grads.npz: gradients w.r.t. the INPUT images of the UNMODIFIED reference, on CPU in fp32.

Run in the build container only (needs the reference tree):

    python tests/golden/make_golden_input_grads.py            # small cases (seconds)
    python tests/golden/make_golden_input_grads.py --vitl     # + ViT-L 896x448 B=1 (minutes, ~14 GB RSS)

Inputs: tests/input_grads_cases.py; parameters: oracle.painter_oracle.random_params(cfg, seed) (make_golden.py's recipe).
Per case: loss, d imgs, d tgts (full tensors, or every SAMPLE_STRIDE-th / VITL_STRIDE-th element of the flattened tensor):
  painter/       Painter small_config, B = 2, random mask, the ignore rule hitting sample 1; full tensors
  painter_pred/  the same with the objective loss + (pred_patch * r).sum(): samples + every parameter gradient's digests (make_golden.py)
  seggpt/        SegGPT small_config, N = 3, merge_between_batch = 0: samples
  h14/           patch 14 (h14_small_config, depth 24): full tensors
  vitl/          ViT-L B = 1 (--vitl): samples
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import input_grads_cases as C          # noqa: E402
from tests.golden import make_golden as MG         # noqa: E402


def run(cfg, seed_p, imgs, tgts, mask, valid, seg_type=None, merge=-1, r=None):
    """-> (loss, d imgs, d tgts, model) of the reference with imgs / tgts as leaves that require grad."""
    model, _ = MG.build_reference(cfg, seed_p)
    model.eval()
    for p in model.parameters():
        p.grad = None
    xi = imgs.clone().requires_grad_(True)
    xt = tgts.clone().requires_grad_(True)
    B = imgs.shape[0]
    if cfg.seggpt:
        loss, pred, _ = model(xi, xt, mask, valid.clone(), seg_type, merge)
    else:
        loss, pred, _ = model(xi, xt, bool_masked_pos=mask.reshape(B, *cfg.grid), valid=valid.clone())
    obj = loss if r is None else loss + (pred * r).sum()
    obj.backward()
    return loss.item(), xi.grad.detach(), xt.grad.detach(), model


def store(out, prefix, loss, gi, gt, stride=0):
    out[prefix + "loss"] = np.float64(loss)
    if stride:
        out[prefix + "dimgs_sample"] = gi.reshape(-1)[::stride].numpy()
        out[prefix + "dtgts_sample"] = gt.reshape(-1)[::stride].numpy()
        out[prefix + "stride"] = np.int64(stride)
        out[prefix + "dimgs_norm"] = np.float64(gi.double().norm())
        out[prefix + "dtgts_norm"] = np.float64(gt.double().norm())
    else:
        out[prefix + "dimgs"] = gi.numpy()
        out[prefix + "dtgts"] = gt.numpy()


def digests(model, out, prefix):
    """make_golden.py's gradient digests (norm, sum, probe dot, every 997th element) without the full small tensors (size)."""
    names, norms, sums, dots = [], [], [], []
    for name, p in model.named_parameters():
        g = p.grad.detach().float().reshape(-1)
        names.append(name)
        norms.append(float(g.double().norm()))
        sums.append(float(g.double().sum()))
        dots.append(float((g.double() * MG.probe_vector(name, g.numel()).double()).sum()))
        out[f"{prefix}grad_sample/{name}"] = g[::MG.GRAD_STRIDE].clone().numpy()
    out[prefix + "grad_names"] = np.array(names)
    out[prefix + "grad_norm"] = np.array(norms, dtype=np.float64)
    out[prefix + "grad_sum"] = np.array(sums, dtype=np.float64)
    out[prefix + "grad_dot"] = np.array(dots, dtype=np.float64)
    out[prefix + "grad_sample_stride"] = np.int64(MG.GRAD_STRIDE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vitl", action="store_true", help="also the ViT-L B = 1 case")
    args = ap.parse_args()
    torch.set_num_threads(os.cpu_count())
    path = os.path.join(HERE, "input_grads.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    loss, gi, gt, _ = run(cfg, sp, imgs, tgts, mask, valid)
    store(out, "painter/", loss, gi, gt)
    r = C.pred_probe(cfg, imgs.shape[0])
    loss, gi, gt, model = run(cfg, sp, imgs, tgts, mask, valid, r=r)
    store(out, "painter_pred/", loss, gi, gt, stride=C.SAMPLE_STRIDE)
    digests(model, out, "painter_pred/")
    cfg, sp, imgs, tgts, mask, valid, seg_type, merge = C.seggpt_case()
    loss, gi, gt, _ = run(cfg, sp, imgs, tgts, mask, valid, seg_type, merge)
    store(out, "seggpt/", loss, gi, gt, stride=C.SAMPLE_STRIDE)
    cfg, sp, imgs, tgts, mask, valid = C.h14_case()
    loss, gi, gt, _ = run(cfg, sp, imgs, tgts, mask, valid)
    store(out, "h14/", loss, gi, gt)
    if args.vitl:
        cfg, sp, imgs, tgts, mask, valid = C.vitl_case()
        loss, gi, gt, _ = run(cfg, sp, imgs, tgts, mask, valid)
        store(out, "vitl/", loss, gi, gt, stride=C.VITL_STRIDE)
    np.savez_compressed(path, **out)
    print("input_grads.npz", {k: float(v) for k, v in out.items() if k.endswith("loss")}, "%.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
