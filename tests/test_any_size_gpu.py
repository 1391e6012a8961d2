"""The forward at a run-time input size other than the constructed one (csrc/attn_any.hip, include/painter_anysize.h,
painter_amd/ops_anysize.py, HotPath.grid): the any-grid attention forward and the rel-pos table resize against float64 statements, and
the whole model against the UNMODIFIED reference at that size (tests/golden/painter_any_size*.npz) and the oracle in fp64 on the device.

What the issue's list of refusals calls "W % 4 != 0" is tested as "not a whole number of patches": with H == 2W and W a multiple of the
patch size, W % 4 != 0 happens exactly for patch 14 with an odd Wp -- which is fixture case F (140 x 70), and that case runs: no forward
kernel needs the alignment there (HotPath.grid says which reads are vectorised)."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import painter_oracle as O
from tests import any_size_cases as C
from tests import golden_util as G
from tests.guard_bands import CountingLib

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops, ops_anysize
    from tests.test_kernels_gpu import attn_reference, gen, relerr
    from tests.test_model_gpu import build

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
# the gates of tests/test_kernels_gpu.py::test_attn_fwd
OUT_GATE = {F32: 2e-5, BF16: 1.2e-2}
LSE_GATE = {F32: 1e-5, BF16: 2e-3}


# ------------------------------------------------------------------------------------------------ attention, kernel level
def _operands(T, B, H, Hp, Wp, hd, seed=1):
    L = Hp * Wp
    qkv = gen((B * L, 3 * H * hd), seed, 1.0, T)
    rel_h = gen((2 * Hp - 1, hd), seed + 1, 0.2)
    rel_w = gen((2 * Wp - 1, hd), seed + 2, 0.2)
    return qkv, ops.relpos_pack(rel_h, rel_w, Hp, Wp, T)


def _check(T, qkv, rcat, out, lse, B, H, Hp, Wp, scale):
    L = Hp * Wp
    ref, lse_ref = attn_reference(qkv, rcat[: 2 * Hp - 1], rcat[2 * Hp - 1: 2 * Hp + 2 * Wp - 2], B, L, H, Hp, Wp, scale)
    e_o, e_l = relerr(out.float(), ref), relerr(lse, lse_ref)
    print("attn_any %s B=%d H=%d %dx%d hd=%d: out %.2e lse %.2e" % (str(T)[6:], B, H, Hp, Wp, rcat.shape[1], e_o, e_l))
    assert e_l < LSE_GATE[T] and e_o < OUT_GATE[T], (e_o, e_l)
    return ref


GRIDS = [(2, 2, 2, 1, 64), (2, 2, 6, 3, 64), (1, 2, 3, 11, 64), (2, 2, 10, 5, 64), (2, 2, 12, 6, 64), (2, 2, 70, 35, 64),
         (2, 2, 10, 5, 80), (1, 2, 70, 35, 80),
         (2, 2, 8, 4, 64), (2, 2, 16, 8, 64)]          # the last two: grids the old generations take as well


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,Hp,Wp,hd", GRIDS)
def test_attn_any_vs_float64(T, B, H, Hp, Wp, hd):
    L = Hp * Wp
    scale = hd ** -0.5
    qkv, rcat = _operands(T, B, H, Hp, Wp, hd)
    n0, c0 = ops_anysize.attn_any_launches(), ops.attn_launch_counts()
    out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)
    assert ops_anysize.attn_any_launches() == n0 + 1 and ops.attn_launch_counts() == c0       # its own counter; the old slots do not move
    assert out.shape == (B * L, H * hd) and lse.shape == (B * H, L)
    _check(T, qkv, rcat, out, lse, B, H, Hp, Wp, scale)
    if ops_anysize.attn_fwd_takes(L, Hp, Wp):
        old, old_lse = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)
        _check(T, qkv, rcat, old, old_lse, B, H, Hp, Wp, scale)
    else:
        with pytest.raises(RuntimeError):               # pa_attn_fwd keeps its refusal
            ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hp,Wp,hd", [(10, 5, 64), (70, 35, 64), (3, 11, 80)])
def test_attn_any_largest_logit_on_the_last_key(T, Hp, Wp, hd):
    """Key L - 1 sits in the partial tail tile and carries every query's largest logit by ~40 (the bias of an unscaled q spreads the
    others over +-8): the output is its V row, so a kernel that drops, misplaces or zeroes the last key cannot pass."""
    B, H, L = 1, 2, Hp * Wp
    scale = hd ** -0.5
    qkv, rcat = _operands(T, B, H, Hp, Wp, hd, seed=11)
    v = qkv.view(B * L, 3, H, hd)
    v[:, 0, :, 0] = 3.0                                        # every query
    v[:, 1, :, 0] = 0.0
    v[L - 1, 1, :, 0] = 40.0 / (3.0 * scale)                   # key L - 1: + 40 on every logit
    out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)
    ref = _check(T, qkv, rcat, out, lse, B, H, Hp, Wp, scale)
    last_v = qkv.view(B * L, 3, H * hd)[L - 1, 2].double()
    assert float((ref - last_v[None]).abs().max()) < 1e-2 * float(last_v.abs().max())         # (the case is what it claims to be)
    assert float((out.double() - last_v[None]).abs().max()) < 2e-2 * float(last_v.abs().max())


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hp,Wp,hd", [(10, 5, 64), (10, 5, 80), (3, 11, 64)])
def test_attn_any_poisoned_neighbour(T, Hp, Wp, hd):
    """B = 2 with sample 1 all NaN: the keys behind sample 0's last key are sample 1's first tokens, physically.  Sample 0 must come out
    finite and bit-equal to its B = 1 run (where those rows are not the caller's memory at all)."""
    H, L = 2, Hp * Wp
    scale = hd ** -0.5
    one, rcat = _operands(T, 1, H, Hp, Wp, hd, seed=21)
    two = torch.cat([one, torch.full_like(one, float("nan"))])
    o1, l1 = ops_anysize.attn_any_fwd(one, rcat, 1, L, H, Hp, Wp, scale)
    o2, l2 = ops_anysize.attn_any_fwd(two, rcat, 2, L, H, Hp, Wp, scale)
    assert torch.isfinite(o2[:L].float()).all() and torch.isfinite(l2[:H]).all()
    assert torch.equal(o2[:L], o1) and torch.equal(l2[:H], l1)
    assert torch.isnan(o2[L:].float()).all()                  # (and sample 1 is what it was given)


# ------------------------------------------------------------------------------------------------ rel-pos table resize
def resize_statement(t, n_dst):
    """F.interpolate(mode="linear", align_corners=False) along dim 0 of t [n_src, hd], in float64."""
    t = t.double()
    n_src = t.shape[0]
    j = torch.arange(n_dst, dtype=torch.float64)
    s = (n_src / n_dst * (j + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_src - 1)
    i1 = (i0 + 1).clamp_max(n_src - 1)
    l1 = (s - i0)[:, None]
    return (1 - l1) * t[i0] + l1 * t[i1]


def torch_resize(t, n_dst):
    """What the reference's get_rel_pos runs (util/vitdet_utils.py:79-85), on the CPU in float32."""
    return F.interpolate(t.reshape(1, t.shape[0], -1).permute(0, 2, 1), size=n_dst, mode="linear").reshape(-1, n_dst).permute(1, 0)


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("sh,sw,dh,dw", [(15, 7, 19, 9), (15, 7, 11, 5), (111, 55, 139, 69)])
def test_relpos_resize_vs_float64(sh, sw, dh, dw, hd):
    nb = 3
    hs = [gen((sh, hd), 30 + k, 0.2) for k in range(nb)]
    ws = [gen((sw, hd), 40 + k, 0.2) for k in range(nb)]
    tabs = torch.tensor([t.data_ptr() for t in hs] + [t.data_ptr() for t in ws], dtype=torch.int64).cuda()
    out = ops_anysize.relpos_resize(tabs, nb, sh, sw, dh, dw, hd)
    assert out.shape == (nb, dh + dw, hd)
    worst = yard = 0.0
    for k in range(nb):
        for t, got, n in ((hs[k], out[k, :dh], dh), (ws[k], out[k, dh:], dw)):
            want = resize_statement(t.cpu(), n)
            scale = float(t.abs().max())
            worst = max(worst, float((got.cpu().double() - want).abs().max()) / scale)
            yard = max(yard, float((torch_resize(t.cpu(), n).double() - want).abs().max()) / scale)
    print("relpos_resize %d->%d, %d->%d hd %d: deviation %.2e of max|t|, CPU F.interpolate's own %.2e" % (sh, dh, sw, dw, hd, worst, yard))
    # both round a float32 coordinate: they may differ from the statement, and from each other, by the sum of two such errors
    assert worst <= 2 * yard, (worst, yard)
    # the address table pa_relpos_pack_batch takes, and the pack for the run-time grid
    Hp, Wp = (dh + 1) // 2, (dw + 1) // 2
    rcat, _ = ops.relpos_pack_batch(ops_anysize.table_addresses(out, dh), nb, Hp, Wp, hd, F32)
    for k in range(nb):
        assert torch.equal(rcat[k, :dh + dw], out[k]) and not rcat[k, dh + dw:].any()


DYADIC_PAIRS = [(8, 16), (16, 8), (8, 32), (32, 8), (12, 48), (45, 15), (27, 9), (3, 6), (6, 3), (4, 1), (1, 4)]


def dyadic_tables(n, hd, nb, seed):
    """nb tables [n, hd] whose entries are integer multiples of 8 in [-248, 248]."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(-31, 32, (n, hd), generator=g) * 8).float() for _ in range(nb)]


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("role", ["h", "w"])
@pytest.mark.parametrize("src,dst", DYADIC_PAIRS, ids=["%dto%d" % p for p in DYADIC_PAIRS])
def test_relpos_resize_dyadic_cases_are_exact(src, dst, role, hd):
    """Length pairs whose ratio is a power of two, or 3 with an odd source: the source coordinate n_src / n_dst * (j + 0.5) - 0.5 and both
    weights are dyadic rationals of a few bits, and the entries are multiples of 8 up to 248, so float32 computes every output without a
    rounding -- CPU F.interpolate in float32 equals the float64 statement bit for bit (asserted here), and the kernel must too: no
    `2 x torch's own deviation`.  Each pair resizes rel_pos_h while rel_pos_w keeps another pair, and the other way round; even lengths,
    which no model asks for, are lengths like any other to the kernel.  Covered: the gather index, both clamps (s < 0 at j = 0, i1 at the
    end), 1 -> n and n -> 1, and the block and table addressing (three blocks, h rows in front of w rows)."""
    nb = 3
    other = (15, 5)                                            # the other table: ratio 3, odd source, exact as well
    (sh, dh), (sw, dw) = ((src, dst), other) if role == "h" else (other, (src, dst))
    hs, ws = dyadic_tables(sh, hd, nb, 100 * src + dst), dyadic_tables(sw, hd, nb, 100 * src + dst + 7)
    for t in hs + ws:
        assert float(t.abs().max()) <= 248 and bool((t % 8 == 0).all())
    dev_h, dev_w = [t.cuda() for t in hs], [t.cuda() for t in ws]
    tabs = torch.tensor([t.data_ptr() for t in dev_h] + [t.data_ptr() for t in dev_w], dtype=torch.int64).cuda()
    out = ops_anysize.relpos_resize(tabs, nb, sh, sw, dh, dw, hd)
    assert out.shape == (nb, dh + dw, hd) and out.dtype == torch.float32
    out = out.cpu()
    for k in range(nb):
        for name, t, got, n in (("rel_pos_h", hs[k], out[k, :dh], dh), ("rel_pos_w", ws[k], out[k, dh:], dw)):
            want = resize_statement(t, n)
            assert torch.equal(want.float().double(), want) and torch.equal(torch_resize(t, n).double(), want)      # (the case is exact)
            bad = (got.double() != want).nonzero()
            assert not len(bad), ("block %d %s %d -> %d: %d of %d entries differ from the float64 statement; first: row %d channel %d, got %r, expected %r"
                                  % (k, name, t.shape[0], n, len(bad), got.numel(), int(bad[0][0]), int(bad[0][1]),
                                     float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))


def test_relpos_resize_to_the_same_lengths_launches_nothing(monkeypatch):
    counting = CountingLib(ops_anysize.lib)
    monkeypatch.setattr(ops_anysize, "lib", counting)
    t = [gen((15, 64), 1, 0.2), gen((7, 64), 2, 0.2)]
    tabs = torch.tensor([x.data_ptr() for x in t], dtype=torch.int64).cuda()
    assert ops_anysize.relpos_resize(tabs, 1, 15, 7, 15, 7, 64) is None and counting.calls == {}
    out = ops_anysize.relpos_resize(tabs, 1, 15, 7, 15, 9, 64)            # one length stays: copied bit for bit
    assert counting.calls == {"pa_relpos_resize": 1} and torch.equal(out[0, :15], t[0])


# ------------------------------------------------------------------------------------------------ the model
def _routes():
    return ops_anysize.attn_any_launches(), sum(ops.attn_launch_counts()["fwd"])


def _run_fixture(name, dtype):
    _, seed_p, _, size, fname = C.CASES[name]
    cfg = C.config(name)
    m, _ = build(cfg, seed_p, dtype)
    imgs, tgts, mask, valid = C.inputs(name)
    r0 = _routes()
    with torch.no_grad():
        loss, pred, mo = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(C.BATCH, *C.run_config(name).grid).cuda(), valid=valid.cuda())
    r1 = _routes()
    Hp, Wp = C.run_config(name).grid
    any_grid = not ops_anysize.attn_fwd_takes(Hp * Wp, Hp, Wp)
    assert any_grid == (name != "D")
    # every block's attention on the any-grid kernel, or (16 x 8) every block on the existing ones with only the tables resized
    assert (r1[0] - r0[0], r1[1] - r0[1]) == ((cfg.depth, 0) if any_grid else (0, cfg.depth))
    assert mo.shape == (C.BATCH, Hp * Wp) and mo.dtype == torch.bool
    return G.load(fname), float(loss), pred.cpu()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fp32_build_at_another_size_vs_reference_golden(name):
    fx, loss, pred = _run_fixture(name, "fp32")
    ref = float(fx[name + "/loss"])
    e_l, e_p = abs(loss - ref) / abs(ref), G.rel_err(pred, fx[name + "/pred"])
    print("case %s fp32 build vs the reference at %s: loss %.2e, pred %.2e (gate %.0e)" % (name, C.CASES[name][3], e_l, e_p, C.FP32_GATE))
    assert e_l < C.FP32_GATE and e_p < C.FP32_GATE, (e_l, e_p)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_bf16_build_at_another_size_vs_reference_golden(name):
    """Measured on the MI355X (relative Frobenius error of pred; the reference's own bf16 autocast in brackets): see DESIGN.md 4.21."""
    fx, loss, pred = _run_fixture(name, "bf16")
    ref, yard = float(fx[name + "/loss"]), float(fx[name + "/bf16_dev"])
    e_l, e_p = abs(loss - ref) / abs(ref), G.rel_fro(pred, fx[name + "/pred"])
    print("case %s bf16 build vs the reference at %s: loss %.2e, pred %.3e (the reference's own bf16 autocast: %.3e, ratio %.2f)"
          % (name, C.CASES[name][3], e_l, e_p, yard, e_p / yard))
    assert e_l < 2e-3, e_l
    assert e_p <= 1.25 * yard, (e_p, yard)


def _oracle_fp64(cfg, P, imgs, tgts, mask, valid, seg_type=None, merge=-1, dtype=torch.float64, autocast=False):
    Pd = {k: v.to(DEV, dtype) for k, v in P.items()}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        lo, po, _ = O.forward(Pd, cfg, imgs.to(DEV, dtype), tgts.to(DEV, dtype), mask.to(DEV), valid.to(DEV, dtype),
                              None if seg_type is None else seg_type.to(DEV, dtype), merge)
    return float(lo), po.double()


def _against_oracle(tag, dtype, loss, pred, cfg, P, imgs, tgts, mask, valid, seg_type=None, merge=-1):
    """The gates of tests/test_model_gpu.py::test_vit_huge_full_width_vs_oracle_in_fp64, forward half."""
    rf = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    lo, po = _oracle_fp64(cfg, P, imgs, tgts, mask, valid, seg_type, merge)
    e_loss, e_pred = abs(loss - lo) / abs(lo), rf(pred, po)
    if dtype == "fp32":
        print("%s fp32 build vs fp64 oracle: loss %.2e, pred %.2e" % (tag, e_loss, e_pred))
        assert e_loss < 1e-4 and e_pred < 2e-4, (e_loss, e_pred)
        return
    la, pa = _oracle_fp64(cfg, P, imgs, tgts, mask, valid, seg_type, merge, dtype=torch.float32, autocast=True)
    y_loss, y_pred = abs(la - lo) / abs(lo), rf(pa, po)
    print("%s bf16 build vs fp64 oracle (oracle's own bf16 autocast): loss %.2e (%.2e), pred %.2e (%.2e)" % (tag, e_loss, y_loss, e_pred, y_pred))
    assert e_loss <= 1.25 * y_loss and e_pred <= 1.25 * y_pred, (e_loss, y_loss, e_pred, y_pred)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_seggpt_feature_ensemble_at_10x5_vs_oracle_in_fp64(dtype):
    cfg = O.small_config(seggpt=True)
    run = dataclasses.replace(cfg, img_size=(160, 80))
    n, merge = 3, 0
    m, P = build(cfg, 71, dtype)
    imgs, tgts, _, valid = O.synthetic_batch(run, n, 72, "half")
    L = run.grid[0] * run.grid[1]
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.tensor([[1.0], [0.0], [1.0]])             # both type tokens
    r0 = _routes()
    with torch.no_grad():
        loss, pred, mo = m(imgs.cuda(), tgts.cuda(), mask.cuda(), valid.cuda(), seg_type.cuda(), merge)
        loss_none = m(imgs.cuda(), tgts.cuda(), None, valid.cuda(), seg_type.cuda(), merge)[0]      # no mask: zeros of the RUN-TIME length
    assert _routes()[0] - r0[0] == 2 * cfg.depth and mo.shape == (1, L)
    assert torch.isnan(loss_none) or float(loss_none) == 0.0   # (SegGPT's loss has no +1e-2: nothing masked is 0 / 0)
    _against_oracle("SegGPT 10x5 ensemble", dtype, float(loss), pred.double(), cfg, P, imgs, tgts, mask.bool().expand(n, L), valid, seg_type, merge)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_vit_large_factory_at_1120x560_vs_oracle_in_fp64(dtype):
    """The COCO panoptic recipe's size (Painter/eval/coco_panoptic/eval.sh: SIZE=560) on the 896 x 448 ViT-L: 70 x 35 tokens, L = 2450."""
    cfg = O.vit_large_config()
    run = dataclasses.replace(cfg, img_size=(1120, 560))
    m, P = build(cfg, 91, dtype)
    imgs, tgts, mask, valid = O.synthetic_batch(run, 1, 92, "half")
    r0 = _routes()
    with torch.no_grad():
        loss, pred, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(1, 70, 35).cuda(), valid=valid.cuda())
    assert _routes()[0] - r0[0] == cfg.depth and pred.shape == (1, 2450, 768)
    loss, pred = float(loss), pred.double()
    del m
    torch.cuda.empty_cache()
    _against_oracle("ViT-L at 1120x560", dtype, loss, pred, cfg, P, imgs, tgts, mask, valid)


def test_refusals_launch_nothing(monkeypatch):
    cfg = O.small_config()
    m, _ = build(cfg, 51, "fp32")
    counting = {mod: CountingLib(mod.lib) for mod in (ops, ops_anysize)}
    for mod, c in counting.items():
        monkeypatch.setattr(mod, "lib", c)
    x = lambda H, W: torch.zeros(1, 3, H, W, device=DEV)
    with pytest.raises(NotImplementedError, match="forward only"):              # gradients enabled at another size
        m(x(160, 80), x(160, 80))
    with pytest.raises(NotImplementedError, match="whole numbers of 16-pixel patches"):
        with torch.no_grad():
            m(x(168, 84), x(168, 84))
    with pytest.raises(NotImplementedError, match=r"\(2W, W\)"):
        with torch.no_grad():
            m(x(160, 96), x(160, 96))
    launched = {k: v for c in counting.values() for k, v in c.calls.items()}
    assert launched == {}, launched
    with torch.no_grad():                                                           # ... and the same call under no_grad runs
        loss = m(x(160, 80), x(160, 80))[0]
    assert torch.isfinite(loss) and counting[ops_anysize].calls["pa_attn_any_fwd"] == cfg.depth
    for p in m.parameters():                                                        # a frozen model needs no no_grad
        p.requires_grad_(False)
    assert torch.isfinite(m(x(96, 48), x(96, 48))[0])


def test_two_sizes_used_alternately_keep_their_tables(monkeypatch):
    cfg = O.small_config()
    m, _ = build(cfg, 52, "bf16")
    counting = CountingLib(ops_anysize.lib)
    monkeypatch.setattr(ops_anysize, "lib", counting)
    g = torch.Generator().manual_seed(5)
    xs = {s: (torch.randn(1, 3, 2 * s, s, generator=g).cuda(), torch.randn(1, 3, 2 * s, s, generator=g).cuda()) for s in (80, 48, 64)}
    first = {}
    with torch.no_grad():
        for rnd in range(3):
            for s, (a, b) in xs.items():
                pred = m(a, b)[1]
                assert torch.equal(first.setdefault(s, pred), pred)
    assert counting.calls.get("pa_relpos_resize") == 2                              # once per other size, never at the constructed one
    with torch.no_grad():                                                           # a table update re-resizes, like HotPath.relpos re-packs
        m.blocks[3].attn.rel_pos_h.mul_(1.5)
        assert not torch.equal(m(*xs[80])[1], first[80])
    assert counting.calls.get("pa_relpos_resize") == 3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_painter_engine_with_a_real_model_at_input_size_80(dtype):
    from painter_amd import painter_engine as E
    from tests import painter_eval_cases as PC
    cfg = O.small_config()
    m, _ = build(cfg, 53, dtype)
    pictures = [PC.picture(80 + i, h, w) for i, (h, w) in enumerate([(120, 160), (97, 61), (200, 150)])]
    n0 = ops_anysize.attn_any_launches()
    outs = {bs: E.PainterEngine(m, "cuda", "ade20k_semseg", *PC.prompt_pair(), input_size=80, batch_size=bs).run(pictures) for bs in (1, 3)}
    assert ops_anysize.attn_any_launches() - n0 == 4 * cfg.depth                    # 3 forwards of one picture, 1 forward of three
    for a, b, p in zip(outs[1], outs[3], pictures):
        assert a.shape == p.shape and a.dtype == np.uint8 and np.array_equal(a, b)
        assert len(np.unique(a.reshape(-1, 3), axis=0)) > 1                          # (a picture, not one colour)
