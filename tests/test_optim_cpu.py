"""CPU: the optimizer oracle (oracle/optim_oracle.py) pinned against torch.optim.AdamW + clip_grad_norm_ + the GradScaler skip
rule, i.e. against the very objects the reference uses (main_train.py:348, util/misc.py:256-268)."""
import torch

from oracle import optim_oracle as OO
from tests import optim_cases as C


def _setup(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (33,), (4, 3, 2, 2), (129,)]
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (10.0 if k == 1 else 0.3) for s in shapes] for k in range(4)]
    cfg = [(1e-3, 0.05), (5e-4, 0.0), (1e-3 * 0.75, 0.05), (2e-4, 0.0)]          # (lr * lr_scale, weight decay) per tensor
    return params, grads, cfg


def test_oracle_matches_torch_adamw_with_unscale_and_clip():
    params, grads, cfg = _setup(0)
    ref_p = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(ref_p, cfg)], lr=1e-3, betas=(0.9, 0.95))
    ora_p = [p.clone() for p in params]
    state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in params]
    scale, clip = 1024.0, 3.0
    for k in range(4):
        for p, g in zip(ref_p, grads[k]):
            p.grad = (g * scale).clone()
        # reference sequence: unscale_, clip_grad_norm_, step
        for p in ref_p:
            p.grad.div_(scale)
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_p, clip)
        opt.step()
        norm, skipped = OO.scaled_clipped_step(ora_p, [g * scale for g in grads[k]], state, cfg, scale, clip, 0.9, 0.95, 1e-8)
        assert not skipped
        assert abs(float(norm) - float(ref_norm)) <= 1e-5 * float(ref_norm)
        for a, b in zip(ora_p, ref_p):
            assert torch.allclose(a, b.detach(), rtol=1e-6, atol=1e-7)
    for st, p in zip(state, ref_p):
        assert torch.allclose(st["exp_avg"], opt.state[p]["exp_avg"], rtol=1e-6, atol=1e-8)
        assert torch.allclose(st["exp_avg_sq"], opt.state[p]["exp_avg_sq"], rtol=1e-6, atol=1e-10)
        assert int(st["step"]) == int(opt.state[p]["step"])


def test_oracle_skips_on_non_finite_gradient():
    params, grads, cfg = _setup(1)
    ora_p = [p.clone() for p in params]
    state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in params]
    bad = [g.clone() for g in grads[0]]
    bad[2].view(-1)[3] = float("inf")
    _, skipped = OO.scaled_clipped_step(ora_p, bad, state, cfg, 1.0, 3.0)
    assert skipped and all(torch.equal(a, b) for a, b in zip(ora_p, params)) and all(st["step"] == 0 for st in state)


def test_float64_loop_and_oracle_keep_one_step_count_per_parameter():
    """Two parameters in one group, lr 1e-2, betas (0.9, 0.95), constant gradient 0.3; the second gets its first gradient in step 5.
    torch.optim.AdamW counts its steps per parameter: the late one is at its own step 1 and moves by exactly lr, to 0.99 -- a count
    shared by the group (5) would leave it at 0.99481.  The helper's float64 loop (the GPU tests' reference) and the oracle agree."""
    params = [torch.ones(5), torch.ones(5)]
    grad = torch.full((5,), 0.3)
    steps = [dict(grads=[grad, None if k < 4 else grad]) for k in range(5)]
    ref = C.torch_adamw_loop(params, [0, 0], [(1e-2, 0.0)], steps, dtype=torch.float64)
    assert ref["step"] == [5.0, 1.0]
    assert abs(float(ref["p"][1][0]) - 0.99) < 1e-9
    bc1, bc2 = 1.0 - 0.9 ** 5, 1.0 - 0.95 ** 5
    shared = 1.0 - 1e-2 / bc1 * (0.1 * 0.3) / ((0.05 * 0.09) ** 0.5 / bc2 ** 0.5 + 1e-8)
    assert abs(shared - 0.99481) < 1e-5 and abs(float(ref["p"][1][0]) - shared) > 4e-3       # the two readings are far apart
    ora_p = [p.clone() for p in params]
    state = [dict(step=0, exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5)) for _ in params]
    for st in steps:
        norm, skipped = OO.scaled_clipped_step(ora_p, st["grads"], state, [(1e-2, 0.0)] * 2, 1.0, None, 0.9, 0.95, 1e-8)
        assert not skipped
    assert [float(s["step"]) for s in state] == ref["step"]
    for a, b in zip(ora_p, ref["p"]):
        assert C.rel_err(a, b) <= 2e-7
    # a parameter that never has a gradient stays as it was, without state; the norm is taken over the live gradients only
    ref = C.torch_adamw_loop(params, [0, 0], [(1e-2, 0.05)], [dict(grads=[grad * 128, None])] * 2, dtype=torch.float64, scale=128.0, max_norm=0.05)
    assert ref["step"] == [2.0, 0.0] and torch.equal(ref["p"][1], params[1].double()) and not ref["exp_avg_sq"][1].any()
    ora_p = [p.clone() for p in params]
    state = [dict(step=0, exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5)) for _ in params]
    norm, _ = OO.scaled_clipped_step(ora_p, [grad * 128, None], state, [(1e-2, 0.05)] * 2, 128.0, 0.05, 0.9, 0.95, 1e-8)
    assert abs(float(norm) - 0.3 * 5 ** 0.5) < 1e-6 and torch.equal(ora_p[1], params[1]) and state[1]["step"] == 0
    # a skipped step and a changed learning rate are honoured by the loop
    a = C.torch_adamw_loop(params, [0, 1], [(1e-2, 0.0), (1e-3, 0.0)], [dict(grads=[grad, grad]), dict(skip=True), dict(grads=[grad, grad], lrs=[0.0, 1e-3])],
                           dtype=torch.float64)
    assert a["step"] == [2.0, 2.0] and abs(float(a["p"][0][0]) - 0.99) < 1e-9 and abs(float(a["p"][1][0]) - 0.998) < 1e-9


def test_layout_builders_produce_the_offsets_they_claim():
    for name, cls in C.ALIGN_CLASSES.items():
        for q in "pgmv":
            offs, total = C.flat_layout(C.LENGTHS, cls[q])
            buf, views, guard = C.guarded_views(C.LENGTHS, cls[q])
            assert buf.data_ptr() % 16 == 0 and buf.numel() == total
            end = 0
            for i, (o, n, v) in enumerate(zip(offs, C.LENGTHS, views)):
                assert o % 4 == cls[q][i % len(cls[q])] and o >= end + 4 and v.numel() == n and v.is_contiguous()
                assert v.data_ptr() == buf.data_ptr() + 4 * o and v.data_ptr() % 16 == 4 * (o % 4)
                end = o + n
            assert total >= end + 4
            assert int(guard.sum()) == total - sum(C.LENGTHS) and bool((buf[guard] == C.GUARD).all()) and not guard[offs[-1]]
        res = [set(r % 4 for r in cls[q]) for q in "pgmv"]
        want = {"none": [{0}] * 4, "g": [{0}, {1, 2, 3}, {0}, {0}], "p": [{1, 2, 3}, {0}, {0}, {0}], "mv": [{0}, {0}, {1, 2, 3}, {1, 2, 3}]}
        assert res == want[name] if name in want else all(0 not in r for r in res)
    # the unaligned classes put a view of every length class at a non-zero residue, and a second chunk at an unaligned address
    offs, _ = C.flat_layout(C.LENGTHS, C.ALIGN_CLASSES["g"]["g"])
    assert all(o % 4 != 0 for o in offs) and (offs[C.LENGTHS.index(16385)] + 8192) % 4 != 0
    # the decoder_pred bucket: offsets of the flat message as the all-reduce builds it
    grads = [torch.zeros(n) for _, n in C.DECODER_PRED_BUCKET]
    flat, views = C.bucket_views(grads)
    assert [(v.data_ptr() - flat.data_ptr()) // 4 for v in views] == [0, 64, 128, 320, 323, 37187] and flat.numel() == 37251
    names = [n for n, _ in C.DECODER_PRED_BUCKET]
    for n, v in zip(names, views):
        assert (v.data_ptr() % 16 == 12) == (n in ("decoder_pred.0.weight", "decoder_pred.0.bias")), n
    # the layer-decay groups of the reference's shape: 26 layer ids x {decay, no decay}
    names, sizes, gidx, groups = C.painter_shaped_groups()
    assert len(groups) == 52 and len(names) == 352 and max(sizes) == 20000
    assert {s % 4 for s in sizes} == {0, 1, 2, 3} and any(s % 8192 == 0 for s in sizes)
    lrs = sorted({round(lr / 1e-3, 12) for lr, _ in groups})
    assert len(lrs) == 26 and abs(lrs[0] - 0.75 ** 25) < 1e-12 and lrs[-1] == 1.0
    by = dict(zip(names, gidx))
    assert groups[by["blocks.0.attn.qkv.weight"]] == (1e-3 * 0.75 ** 24, 0.05) and groups[by["blocks.23.norm1.bias"]] == (1e-3 * 0.75, 0.0)
    assert groups[by["pos_embed"]] == (1e-3 * 0.75 ** 25, 0.05) and groups[by["decoder_pred.3.bias"]] == (1e-3, 0.0)


def test_state_dict_hands_out_copies_and_keeps_the_live_step_views():
    """Host side of painter_amd.optim.AdamW (no kernel runs): state[p]["step"] is a view of the optimizer's one step array before and
    after state_dict(), a second state_dict() sees counts advanced in between, and growing the array keeps the counts."""
    from painter_amd import optim as PO
    ps = [torch.nn.Parameter(torch.ones(3)) for _ in range(70)]
    opt = PO.AdamW([{"params": ps[:3]}], lr=1e-3)
    opt._assign_slots(ps[:3])
    opt._steps[:3] = torch.tensor([3.0, 2.0, 1.0])
    sd1 = opt.state_dict()
    opt._steps[:3] += 5                                                    # what the kernel does
    sd2 = opt.state_dict()
    assert [float(sd1["state"][i]["step"]) for i in range(3)] == [3.0, 2.0, 1.0]
    assert [float(sd2["state"][i]["step"]) for i in range(3)] == [8.0, 7.0, 6.0]
    base = opt._steps.untyped_storage().data_ptr()
    assert all(opt.state[p]["step"].untyped_storage().data_ptr() == base and opt.state[p]["step"].dim() == 0 for p in ps[:3])
    assert all(sd2["state"][i]["step"].untyped_storage().data_ptr() != base for i in range(3))
    opt.add_param_group({"params": ps[3:]})
    opt._assign_slots(ps[3:])                                              # 70 > 64: reallocate, copy, re-point
    base = opt._steps.untyped_storage().data_ptr()
    assert opt._steps.numel() == 128 and all(opt.state[p]["step"].untyped_storage().data_ptr() == base for p in ps)
    assert [float(opt.state[p]["step"]) for p in ps[:4]] == [8.0, 7.0, 6.0, 0.0]
    ref = torch.optim.AdamW([{"params": ps[:3]}, {"params": ps[3:]}], lr=1e-3)
    ref.load_state_dict(opt.state_dict())
    assert [float(ref.state[p]["step"]) for p in ps[:4]] == [8.0, 7.0, 6.0, 0.0]
