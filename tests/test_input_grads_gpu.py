"""Gradients w.r.t. the input images and the returned prediction, and frozen-model backward (in-context / prompt tuning):
  the two kernels alone (pa_patch_embed_dgrad, pa_pred_bwd) against fp64, the whole model against the unmodified reference's input
  gradients (tests/golden/input_grads.npz) and the CPU oracle, frozen and partly frozen parameters, and a prompt-tuning loop."""
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import painter_oracle as O
from tests import golden_util as G
from tests import input_grads_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import models_painter, models_seggpt, ops
    from painter_amd import optim as pa_optim


def build(cfg, seed, dtype):
    cls = models_seggpt.SegGPT if cfg.seggpt else models_painter.Painter
    m = cls(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
            drop_path_rate=0.1, window_size=14, qkv_bias=True, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6),
            window_block_indexes=(), residual_block_indexes=[], use_rel_pos=True, out_feature="last_feat",
            decoder_embed_dim=cfg.decoder_embed_dim, loss_func=cfg.loss_func, compute_dtype=dtype,
            **({} if cfg.depth == 24 else {"feature_taps": cfg.taps}))
    P = O.random_params(cfg, seed)
    m.load_state_dict(P, strict=True)
    return m.cuda().eval(), P


def run(m, cfg, imgs, tgts, mask, valid, seg_type=None, merge=-1, r=None, grad_imgs=True, grad_tgts=True):
    """-> (loss, pred_patch, d imgs, d tgts) through the module; parameter gradients are left in p.grad."""
    for p in m.parameters():
        p.grad = None
    xi = imgs.cuda().requires_grad_(grad_imgs)
    xt = tgts.cuda().requires_grad_(grad_tgts)
    if cfg.seggpt:
        loss, pred, _ = m(xi, xt, mask.cuda(), valid.clone().cuda(), seg_type.cuda(), merge)
    else:
        loss, pred, _ = m(xi, xt, bool_masked_pos=mask.reshape(imgs.shape[0], *cfg.grid).cuda(), valid=valid.clone().cuda())
    obj = loss if r is None else loss + (pred * r.cuda()).sum()
    obj.backward()
    torch.cuda.synchronize()
    return loss.detach(), pred.detach(), xi.grad, xt.grad


def oracle(cfg, seed_p, imgs, tgts, mask, valid, seg_type=None, merge=-1, r=None, autocast=False):
    P = {k: v.clone().requires_grad_(True) for k, v in O.random_params(cfg, seed_p).items()}
    xi = imgs.clone().requires_grad_(True)
    xt = tgts.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        if cfg.seggpt:
            n, L = imgs.shape[0], cfg.grid[0] * cfg.grid[1]
            loss, pred, _ = O.forward(P, cfg, xi, xt, mask.bool().expand(n, L), valid.clone(), seg_type, merge)
        else:
            loss, pred, _ = O.forward(P, cfg, xi, xt, mask, valid.clone())
        obj = loss if r is None else loss + (pred.float() * r).sum()
    obj.backward()
    return float(loss), xi.grad.float(), xt.grad.float(), P


# ------------------------------------------------------------------------------------------------ kernels alone
def _dgrad_ref(dpe, w, B, Hp, Wp, P):
    """fp64 dPE . Wp, folded back to images (the conv's input gradient), x stream and y stream."""
    K = 3 * P * P
    cols = dpe.double().cpu() @ w.double().cpu()[:, :K]
    L = Hp * Wp
    out = []
    for s in range(2):
        c = cols[s * B * L:(s + 1) * B * L].reshape(B, L, K).transpose(1, 2)
        out.append(F.fold(c, (Hp * P, Wp * P), kernel_size=P, stride=P))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,Hp,Wp,P,D", [(2, 56, 28, 16, 1024), (2, 8, 4, 14, 160), (2, 8, 4, 16, 128)])
def test_patch_embed_dgrad_kernel_vs_fp64(dtype, B, Hp, Wp, P, D):
    """ViT-L shape (bf16: the gemm256 path; fp32: the generic engine), patch 14 (generic, padded K), the small model's shape."""
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(3)
    R = 2 * B * Hp * Wp
    dpe = (torch.randn(R, D, generator=g) * 1e-2).to(T).cuda()
    wf = (torch.randn(D, 3, P, P, generator=g) / (3 * P * P) ** 0.5).cuda()
    w = ops.patch_weight_pack(wf, T, P)
    di, dt = ops.patch_embed_dgrad(dpe, w, B, Hp, Wp, P, D)
    torch.cuda.synchronize()
    ri, rt = _dgrad_ref(dpe, w, B, Hp, Wp, P)
    ei, et = G.rel_err(di.cpu(), ri), G.rel_err(dt.cpu(), rt)
    print("pa_patch_embed_dgrad %s B=%d %dx%d P=%d D=%d: rel-max %.2e / %.2e" % (dtype, B, Hp, Wp, P, D, ei, et))
    assert ei < 1e-5 and et < 1e-5, (ei, et)
    # addend: d tgts = dcols + alpha * addend, exactly the fp32 sum; the x stream unchanged; two launches give the same bits
    add = torch.randn(dt.shape, generator=g).cuda()
    di2, dt2 = ops.patch_embed_dgrad(dpe, w, B, Hp, Wp, P, D, addend=add, alpha=-1.0)
    assert torch.equal(di2, di) and torch.equal(dt2, dt - add)
    di3, dt3 = ops.patch_embed_dgrad(dpe, w, B, Hp, Wp, P, D, addend=add, alpha=-1.0)
    assert torch.equal(di3, di2) and torch.equal(dt3, dt2)
    # one stream alone: the same bits
    only_i, none_t = ops.patch_embed_dgrad(dpe, w, B, Hp, Wp, P, D, want_tgts=False)
    none_i, only_t = ops.patch_embed_dgrad(dpe, w, B, Hp, Wp, P, D, want_imgs=False)
    assert none_t is None and none_i is None and torch.equal(only_i, di) and torch.equal(only_t, dt)


@pytest.mark.parametrize("with_loss,with_patch", [(True, True), (True, False), (False, True)])
def test_pred_bwd_kernel_vs_fp64(with_loss, with_patch):
    cfg = O.small_config()
    B, (Hp, Wp), P = 2, cfg.grid, cfg.patch_size
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, B, 61, "random")
    g = torch.Generator().manual_seed(62)
    pred = (tgts + 0.02 * torch.randn(tgts.shape, generator=g)).cuda()
    tgts_d, valid_d = tgts.cuda(), (torch.rand(tgts.shape, generator=g) > 0.1).float().cuda()
    mask_u8 = mask.bool().contiguous().view(torch.uint8).cuda()
    loss_out = ops.loss_fwd(pred, tgts_d, valid_d, mask_u8, P, ignore_rule=False, eps_den=1e-2, kind="smoothl1")
    dloss = torch.tensor([0.75], device="cuda") if with_loss else None
    dpatch = (torch.randn(B, Hp * Wp, 3 * P * P, generator=g)).cuda() if with_patch else None
    dpred, dpl = ops.pred_bwd(pred, tgts_d, valid_d, mask_u8, dloss, loss_out, dpatch, P, "smoothl1", want_loss_term=with_loss)
    torch.cuda.synchronize()
    ref = torch.zeros(pred.shape, dtype=torch.float64)
    if with_loss:
        lterm = ops.loss_bwd(pred, tgts_d, valid_d, mask_u8, dloss, loss_out, P, "smoothl1")
        assert torch.equal(dpl, lterm)                       # the loss term is pa_loss_bwd's, bit for bit
        ref += lterm.double().cpu()
    if with_patch:
        ref += O.unpatchify(dpatch.double().cpu(), P)
    e = G.rel_err(dpred.cpu(), ref)
    assert e < 1e-6, e
    if with_loss and not with_patch:
        assert torch.equal(dpred, dpl)


# ------------------------------------------------------------------------------------------------ whole model, fp32 build
def _check_vs_fixture(fx, prefix, loss, gi, gt, tol=1e-3):
    ref = float(fx[prefix + "loss"])
    assert abs(float(loss) - ref) < 1e-4 * abs(ref), (prefix, float(loss), ref)
    gi, gt = gi.detach().float().cpu(), gt.detach().float().cpu()
    if prefix + "stride" in fx.files:
        s = int(fx[prefix + "stride"])
        pairs = [(gi.reshape(-1)[::s], fx[prefix + "dimgs_sample"]), (gt.reshape(-1)[::s], fx[prefix + "dtgts_sample"])]
    else:
        pairs = [(gi, fx[prefix + "dimgs"]), (gt, fx[prefix + "dtgts"])]
    errs = [G.rel_err(a, b) for a, b in pairs]
    print("%s fp32 build vs reference: d imgs %.2e, d tgts %.2e (rel-max)" % (prefix, errs[0], errs[1]))
    assert max(errs) < tol, (prefix, errs)


def test_fp32_input_grads_painter_and_pred_objective_vs_reference_and_oracle():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    m, _ = build(cfg, sp, "fp32")
    loss, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid)
    _check_vs_fixture(fx, "painter/", loss, gi, gt)
    lo, oi, ot, _ = oracle(cfg, sp, imgs, tgts, mask, valid)
    assert G.rel_err(gi.cpu(), oi) < 1e-3 and G.rel_err(gt.cpu(), ot) < 1e-3
    r = C.pred_probe(cfg, imgs.shape[0])
    loss, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid, r=r)
    _check_vs_fixture(fx, "painter_pred/", loss, gi, gt)
    G.check_grad_digests(fx, "painter_pred/", [(n, p.grad) for n, p in m.named_parameters()], 1e-3, 1e-3, 1e-3)


def test_fp32_input_grads_seggpt_ensemble_and_patch14_vs_reference():
    fx = G.load("input_grads.npz")
    cfg, sp, imgs, tgts, mask, valid, seg_type, merge = C.seggpt_case()
    m, _ = build(cfg, sp, "fp32")
    loss, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid, seg_type, merge)
    _check_vs_fixture(fx, "seggpt/", loss, gi, gt)
    cfg, sp, imgs, tgts, mask, valid = C.h14_case()
    m, _ = build(cfg, sp, "fp32")
    loss, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid)
    _check_vs_fixture(fx, "h14/", loss, gi, gt)


def test_fp32_input_grads_vit_large_vs_reference():
    fx = G.load("input_grads.npz")
    if "vitl/loss" not in fx.files:
        pytest.fail("tests/golden/input_grads.npz lacks the ViT-L case (make_golden_input_grads.py --vitl)")
    cfg, sp, imgs, tgts, mask, valid = C.vitl_case()
    m, _ = build(cfg, sp, "fp32")
    loss, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid)
    _check_vs_fixture(fx, "vitl/", loss, gi, gt)


# ------------------------------------------------------------------------------------------------ bf16 build
def test_bf16_input_grads_within_the_oracles_own_bf16_deviation():
    """Gate: relative Frobenius error <= 1.25 x the oracle's own CPU bf16-autocast deviation on the same case (both against the fp32
    oracle).  Rel-max: <= 1e-1 for d imgs.  d tgts carries the loss's direct term, smooth-L1'(pred - tgts) with beta = 0.01: a pixel whose
    |pred - tgts| lies near or inside 0.01 flips that term by up to its full size under any bf16 rounding of pred -- the oracle's own bf16
    run shows the same rel-max (measured: 0.94 for the HIP build on this case) -- so its rel-max is gated at 1.25 x the oracle's own."""
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    m, _ = build(cfg, sp, "bf16")
    _, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid)
    _, oi, ot, _ = oracle(cfg, sp, imgs, tgts, mask, valid)
    _, ai, at, _ = oracle(cfg, sp, imgs, tgts, mask, valid, autocast=True)
    for name, got, ref, yard in (("d imgs", gi, oi, ai), ("d tgts", gt, ot, at)):
        e, y, emax, ymax = G.rel_fro(got.cpu(), ref), G.rel_fro(yard, ref), G.rel_err(got.cpu(), ref), G.rel_err(yard, ref)
        print("bf16 build %s: rel-Frobenius %.3e (oracle's own bf16 autocast: %.3e), rel-max %.3e (oracle's own: %.3e)" % (name, e, y, emax, ymax))
        assert e <= 1.25 * y, (name, e, y)
        assert emax <= (1e-1 if name == "d imgs" else 1.25 * ymax), (name, emax, ymax)


# ------------------------------------------------------------------------------------------------ frozen parameters
def _counting(monkeypatch):
    calls = {"linear_wgrad": 0, "conv3x3_wgrad": 0, "patch_embed_wgrad": 0, "attn_bwd_relpos": 0}
    for name in calls:
        orig = getattr(ops, name)

        def wrap(*a, _o=orig, _n=name, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    return calls


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_frozen_model_input_grads_same_bits_and_no_parameter_work(dtype, monkeypatch):
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    m, _ = build(cfg, sp, dtype)
    r = C.pred_probe(cfg, imgs.shape[0])
    _, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid, r=r)
    full = {n: p.grad.clone() for n, p in m.named_parameters()}
    calls = _counting(monkeypatch)
    for p in m.parameters():
        p.requires_grad_(False)
    _, _, fi, ft = run(m, cfg, imgs, tgts, mask, valid, r=r)
    assert torch.equal(fi, gi) and torch.equal(ft, gt)
    assert all(p.grad is None for p in m.parameters())
    assert calls == {"linear_wgrad": 0, "conv3x3_wgrad": 0, "patch_embed_wgrad": 0, "attn_bwd_relpos": 0}, calls
    # partly frozen: exactly the trainable parameters get gradients, with the bits of the all-trainable run
    for prefix in ("decoder_", "blocks.23."):
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith(prefix))
        _, _, pi, pt = run(m, cfg, imgs, tgts, mask, valid, r=r)
        assert torch.equal(pi, gi) and torch.equal(pt, gt), prefix
        for n, p in m.named_parameters():
            if n.startswith(prefix):
                assert p.grad is not None and torch.equal(p.grad, full[n]), n
            else:
                assert p.grad is None, n


def test_nothing_else_moved():
    """Loss, pred and every parameter gradient are bit-identical whether or not imgs / tgts require grad; no input gradient unless asked;
    a forward under no_grad saves nothing."""
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    m, _ = build(cfg, sp, "bf16")
    l0, p0, gi, gt = run(m, cfg, imgs, tgts, mask, valid, grad_imgs=False, grad_tgts=False)
    g0 = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert gi is None and gt is None
    l1, p1, gi, gt = run(m, cfg, imgs, tgts, mask, valid)
    assert gi is not None and gt is not None
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    assert all(torch.equal(p.grad, g0[n]) for n, p in m.named_parameters())
    _, _, gi, gt = run(m, cfg, imgs, tgts, mask, valid, grad_imgs=False)
    assert gi is None and gt is not None
    seen = []
    orig = m._hot.forward

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out[3])
        return out
    m._hot.forward = spy
    with torch.no_grad():
        loss, pred, _ = m(imgs.cuda().requires_grad_(True), tgts.cuda(), bool_masked_pos=mask.reshape(2, *cfg.grid).cuda(), valid=valid.clone().cuda())
    del m._hot.forward
    S = seen[0]
    assert not S.need_grad and S.blocks == [] and S.taps == [] and S.cols is None and not hasattr(S, "concat")
    assert pred.grad_fn is None and loss.grad_fn is None


def test_pred_patch_is_differentiable_and_double_backward_raises():
    cfg, sp, imgs, tgts, mask, valid = C.painter_case()
    m, _ = build(cfg, sp, "fp32")
    xi = imgs.cuda().requires_grad_(True)
    loss, pred, _ = m(xi, tgts.cuda(), bool_masked_pos=mask.reshape(2, *cfg.grid).cuda(), valid=valid.clone().cuda())
    assert pred.grad_fn is not None
    (g,) = torch.autograd.grad(pred.square().sum(), xi, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ------------------------------------------------------------------------------------------------ in-context tuning
def test_in_context_tuning_frozen_seggpt_learnable_prompt():
    """Frozen SegGPT (N = 3, feature ensemble), one learnable prompt image / target pair (the top half of every sample's imgs / tgts);
    five painter_amd.optim.AdamW steps lower the loss; the first step's prompt gradient matches the oracle (fp32 build)."""
    cfg, sp, imgs, tgts, mask, valid, seg_type, merge = C.seggpt_case()
    m, P = build(cfg, sp, "fp32")
    for p in m.parameters():
        p.requires_grad_(False)
    N, H = imgs.shape[0], cfg.img_size[0]
    prompt = torch.stack([imgs[0, :, :H // 2], tgts[0, :, :H // 2]]).cuda().requires_grad_(True)       # [2, 3, H/2, W]
    q_img, q_tgt = imgs[:, :, H // 2:].cuda(), tgts[:, :, H // 2:].cuda()
    opt = pa_optim.AdamW([prompt], lr=2e-2, weight_decay=0.0)

    def step():
        opt.zero_grad()
        xi = torch.cat([prompt[0].expand(N, -1, -1, -1), q_img], dim=2)
        xt = torch.cat([prompt[1].expand(N, -1, -1, -1), q_tgt], dim=2)
        loss, _, _ = m(xi, xt, mask.cuda(), valid.clone().cuda(), seg_type.cuda(), merge)
        loss.backward()
        return float(loss)

    losses = [step()]
    g0 = prompt.grad.detach().cpu().clone()
    # the oracle's gradient w.r.t. the same prompt
    Po = {k: v.clone() for k, v in P.items()}
    pr = prompt.detach().cpu().clone().requires_grad_(True)
    xi = torch.cat([pr[0].expand(N, -1, -1, -1), imgs[:, :, H // 2:]], dim=2)
    xt = torch.cat([pr[1].expand(N, -1, -1, -1), tgts[:, :, H // 2:]], dim=2)
    lo, _, _ = O.forward(Po, cfg, xi, xt, mask.bool().expand(N, -1), valid.clone(), seg_type, merge)
    lo.backward()
    e = G.rel_err(g0, pr.grad)
    assert abs(losses[0] - float(lo)) < 1e-4 * abs(float(lo)) and e < 1e-3, (losses[0], float(lo), e)
    for _ in range(5):
        opt.step()
        losses.append(step())
    print("in-context tuning, frozen SegGPT: losses %s, first prompt gradient vs oracle rel-max %.2e" % (["%.5f" % x for x in losses], e))
    assert losses[-1] < losses[0], losses
    assert all(p.grad is None for p in m.parameters())
