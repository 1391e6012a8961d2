"""The CPU oracle's gradients w.r.t. the input images against the unmodified reference's (tests/golden/input_grads.npz, written by
tests/golden/make_golden_input_grads.py): pins the oracle in the direction the GPU tests of tests/test_input_grads_gpu.py use it."""
import torch

from oracle import painter_oracle as O
from tests import golden_util as G
from tests import input_grads_cases as C


def _oracle(cfg, seed_p, imgs, tgts, mask, valid, seg_type=None, merge=-1, r=None):
    P = {k: v.clone().requires_grad_(True) for k, v in O.random_params(cfg, seed_p).items()}
    xi = imgs.clone().requires_grad_(True)
    xt = tgts.clone().requires_grad_(True)
    if cfg.seggpt:
        n, L = imgs.shape[0], cfg.grid[0] * cfg.grid[1]
        loss, pred, _ = O.forward(P, cfg, xi, xt, mask.bool().expand(n, L), valid.clone(), seg_type, merge)
    else:
        loss, pred, _ = O.forward(P, cfg, xi, xt, mask, valid.clone())
    obj = loss if r is None else loss + (pred * r).sum()
    obj.backward()
    return loss.item(), xi.grad, xt.grad, P


def _check(fx, prefix, loss, gi, gt, tol=1e-4):
    ref = float(fx[prefix + "loss"])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (prefix, loss, ref)
    if prefix + "stride" in fx.files:
        s = int(fx[prefix + "stride"])
        pairs = [(gi.reshape(-1)[::s], fx[prefix + "dimgs_sample"]), (gt.reshape(-1)[::s], fx[prefix + "dtgts_sample"])]
        assert abs(float(gi.double().norm()) / float(fx[prefix + "dimgs_norm"]) - 1) < tol
        assert abs(float(gt.double().norm()) / float(fx[prefix + "dtgts_norm"]) - 1) < tol
    else:
        pairs = [(gi, fx[prefix + "dimgs"]), (gt, fx[prefix + "dtgts"])]
    for a, b in pairs:
        assert float(torch.as_tensor(b).abs().max()) > 0.0, prefix
        e = G.rel_fro(a, b)
        assert e < tol, (prefix, e)


def test_oracle_input_grads_painter_with_ignore_rule():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    loss, gi, gt, _ = _oracle(cfg, sp, imgs, tgts, mask, valid)
    _check(fx, "painter/", loss, gi, gt)
    # samples meet only in the loss: the ignored one (valid := 0) gets no gradient at all, the other one does
    assert float(gi[1].abs().max()) == 0.0 and float(gt[1].abs().max()) == 0.0
    assert float(gi[0].abs().max()) > 0.0 and float(gt[0].abs().max()) > 0.0


def test_oracle_input_and_parameter_grads_with_a_pred_objective():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    loss, gi, gt, P = _oracle(cfg, sp, imgs, tgts, mask, valid, r=C.pred_probe(cfg, imgs.shape[0]))
    _check(fx, "painter_pred/", loss, gi, gt)
    G.check_grad_digests(fx, "painter_pred/", [(n, p.grad) for n, p in P.items()], 1e-4, 1e-4, 1e-4, sample_rtol=1e-3)


def test_oracle_input_grads_seggpt_feature_ensemble():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid, seg_type, merge = C.seggpt_case()
    loss, gi, gt, _ = _oracle(cfg, sp, imgs, tgts, mask, valid, seg_type, merge)
    _check(fx, "seggpt/", loss, gi, gt)


def test_oracle_input_grads_patch14():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid = C.h14_case()
    loss, gi, gt, _ = _oracle(cfg, sp, imgs, tgts, mask, valid)
    _check(fx, "h14/", loss, gi, gt)
