"""GPU parity of Painter task inference on the device (csrc/painter_io.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_eval_host.py -- itself pinned to CPU torch and to the unmodified scripts (tests/test_painter_eval_cpu.py) -- and
against the digests the unmodified scripts produced (tests/golden/painter_eval_io.npz).

The bars: stitch, uint8 and int32 outputs, class maps: np.array_equal, no tolerance.  Bicubic float64 output: max |delta| <=
1e-11 * max(1, max |ref|) -- 16 products and 15 additions in float64 plus a source coordinate p <= 448 whose fused and unfused forms
differ by <= 448 * 2^-53 ~ 5e-14, times a weight slope <= 1.5 per axis -- and the saved uint8 picture equal except where the
reference value lies within 1e-9 of a multiple of 1/255, at most one such pixel per million.  F.interpolate is never called here."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import painter_eval_cases as C
from tests import painter_eval_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E

BICUBIC_GATE = 1e-11
assert {(1, 1), (449, 447), (96, 1000), (480, 640)} <= set(C.SIZES) and len(C.SIZES) >= 12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_eval_io.npz"))


def _engine(task, batch_size=8, model=None):
    return E.PainterEngine(model or C.StandInModel(), "cuda", task, *C.prompt_pair(), input_size=C.RES, batch_size=batch_size)


def _decode(task, toks, sizes, saved=False):
    """toks: float32 numpy [N][L][768]; sizes [(h, w)] -> list of numpy outputs through ONE launch of the C entry point."""
    plan = E.decode(task, torch.from_numpy(toks).cuda(), [(w, h) for h, w in sizes], C.RES, C.RES, C.PATCH, saved=saved)
    if saved:
        return plan.pictures(), plan.saved_pictures()
    return plan.pictures()


# ---- 1. stitch
def test_stitch_is_bit_exact():
    rng = np.random.default_rng(41)
    prompt = rng.integers(0, 256, (C.RES, C.RES, 3), dtype=np.uint8)
    target = rng.integers(0, 256, (C.RES, C.RES, 3), dtype=np.uint8)
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8).repeat(2)[:C.RES, None], (C.RES, C.RES, 3)).copy()
    ramp = np.ascontiguousarray(np.roll(ramp, 7, axis=0))               # every byte value through the normalisation, every channel
    queries = np.stack([rng.integers(0, 256, (C.RES, C.RES, 3), dtype=np.uint8), ramp, ramp.transpose(1, 0, 2).copy()])
    for p, t in ((prompt, target), (ramp, ramp[::-1].copy())):
        eng = E.PainterEngine(C.StandInModel(), "cuda", "ade20k_semseg", p, t)
        assert np.array_equal(eng.prompt.cpu().numpy(), p) and np.array_equal(eng.prompt_tgt.cpu().numpy(), t)
        imgs, tgts = eng.stitch(torch.from_numpy(queries).cuda())
        assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (3, 3, 2 * C.RES, C.RES) and tuple(tgts.shape) == tuple(imgs.shape)
        imgs, tgts = imgs.cpu().numpy(), tgts.cpu().numpy()
        for n in range(3):
            x, tt = H.model_inputs(*H.canvases(p, t, queries[n], C.RES, query_is_resized=True))
            assert np.array_equal(imgs[n:n + 1], x) and np.array_equal(tgts[n:n + 1], tt)


# ---- 2. uint8 / int32 decodes: no tolerance
@pytest.mark.parametrize("h,w", C.SIZES)
def test_decode_u8_and_depth_are_bit_exact(h, w):
    toks = C.tokens(1000 + h)
    for task in ("ade20k_semseg", "coco_pano_inst", "nyuv2_depth"):          # bilinear u8, nearest u8, bilinear depth
        got = _decode(task, toks, [(h, w)])[0]
        ref = H.decode(task, toks[0], (w, h), C.RES, C.RES, C.PATCH)
        assert got.dtype == ref.dtype and got.shape == ref.shape
        bad = int((got != ref).sum())
        print("%s %dx%d: %d of %d values differ" % (task, h, w, bad, ref.size))
        assert np.array_equal(got, ref)
    src = H.lower_half(toks[0], C.RES, C.RES, C.PATCH).astype(np.float64) * H.STD + H.MEAN
    assert (src <= 0).mean() > 0.2 and (src >= 1).mean() > 0.2               # the source saturates at both ends (gain 6: ~35 % each)


def test_decode_all_sizes_in_one_launch():
    toks = C.tokens(77, n=len(C.SIZES))
    for task in ("coco_pano_semseg", "coco_pose", "nyuv2_depth"):
        got = _decode(task, toks, C.SIZES)
        for i, (h, w) in enumerate(C.SIZES):
            assert np.array_equal(got[i], H.decode(task, toks[i], (w, h), C.RES, C.RES, C.PATCH)), (task, h, w)


# ---- 3. bicubic float64: the derived gate
@pytest.mark.parametrize("h,w", C.SIZES)
def test_decode_f64_within_gate(h, w):
    toks = C.tokens(2000 + h, gain=1.5)
    (got,), (got8,) = _decode("derain", toks, [(h, w)], saved=True)
    ref = H.decode("derain", toks[0], (w, h), C.RES, C.RES, C.PATCH)
    assert got.dtype == np.float64 and got.shape == ref.shape and got8.dtype == np.uint8
    err = float(np.abs(got - ref).max())
    ref8 = H.saved_picture(ref)
    diff = got8 != ref8
    scaled = ref * 255.0
    exempt = diff & (np.abs(scaled - np.round(scaled)) <= 1e-9 * 255.0)
    print("bicubic %dx%d: max |delta| %.3e (gate %.3e), saved picture: %d differ, %d exempt" %
          (h, w, err, BICUBIC_GATE * max(1.0, float(np.abs(ref).max())), int(diff.sum()), int(exempt.sum())))
    assert err <= BICUBIC_GATE * max(1.0, float(np.abs(ref).max()))
    assert not (diff & ~exempt).any()
    assert int(exempt.any(-1).sum()) <= ref8.shape[0] * ref8.shape[1] // 1000000          # at most one pixel per million
    assert np.array_equal(_decode("derain", toks, [(h, w)])[0], got)          # without the second output: the same values


def test_run_restoration_returns_the_saved_pictures():
    net = C.StandInModel()
    pictures = C.query_pictures("derain")
    restored, saved = _engine("derain", model=net).run_restoration(pictures)
    plain = _engine("derain").run(pictures)
    assert len(restored) == len(saved) == len(pictures)
    for r, s8, p, pic in zip(restored, saved, plain, pictures):
        assert np.array_equal(r, p) and s8.dtype == np.uint8 and s8.shape == pic.shape
        assert np.array_equal(s8, H.saved_picture(r))                        # the device's clip * 255 of its own float64 values
    with pytest.raises(ValueError):
        _engine("ade20k_semseg").run_restoration(pictures)


def test_a_job_outside_the_batch_writes_nothing():
    """include/painter_hip.h: a job whose sample is outside [0, n_samples) writes nothing."""
    toks = torch.from_numpy(C.tokens(5, n=2)).cuda()
    for task in ("ade20k_semseg", "coco_pose", "nyuv2_depth", "derain"):
        plan = E.DecodePlan(task, [(40, 30), (40, 30), (40, 30), (40, 30)], "cuda", saved=True, samples=[1, -1, 2, 0])
        plan.out.fill_(7)
        if plan.out8 is not None:
            plan.out8.fill_(7)
        outs = plan.launch(toks, C.RES, C.RES, C.PATCH).pictures()
        assert np.array_equal(outs[0], H.decode(task, toks[1].cpu().numpy(), (40, 30), C.RES, C.RES, C.PATCH))
        assert np.array_equal(outs[3], H.decode(task, toks[0].cpu().numpy(), (40, 30), C.RES, C.RES, C.PATCH))
        assert (outs[1] == 7).all() and (outs[2] == 7).all()
        if plan.out8 is not None:
            s8 = plan.saved_pictures()
            assert (s8[1] == 7).all() and (s8[2] == 7).all() and np.array_equal(s8[0], H.saved_picture(outs[0]))


def test_entry_points_refuse_bad_arguments():
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched."""
    from painter_amd._lib import lib
    ok = dict(n_jobs=1, n_samples=1, max_h=8, max_w=8, res_h=448, res_w=448, patch=16)
    bad = [dict(n_jobs=0), dict(n_jobs=65536), dict(n_samples=0), dict(max_h=0), dict(max_h=65536), dict(max_w=0), dict(patch=0),
           dict(res_h=440), dict(res_w=450), dict(res_h=0)]
    for change in bad:
        a = dict(ok, **change)
        args = (0, 0, a["n_jobs"], a["n_samples"], a["max_h"], a["max_w"], a["res_h"], a["res_w"], a["patch"])
        assert lib.pa_painter_decode_u8(*args, 0, 0) == 1 and lib.pa_painter_decode_u8(*args, 1, 0) == 1, change
        assert lib.pa_painter_decode_depth(*args, 0) == 1 and lib.pa_painter_decode_f64(*args, 0) == 1, change
    for n, rh, rw in ((0, 448, 448), (65536, 448, 448), (1, 0, 448), (1, 448, 0), (1, 32768, 448)):
        assert lib.pa_painter_stitch(0, 0, 0, 0, 0, n, rh, rw, 0) == 1, (n, rh, rw)
    for h, w, k, d in ((0, 4, 3, 0), (4, 0, 3, 0), (4, 4, 0, 0), (4, 4, 4097, 0), (4, 4, 3, 3), (4, 4, 3, -1)):
        assert lib.pa_palette_argmin(0, 0, 0, h, w, k, d, 0) == 1, (h, w, k, d)
    with pytest.raises(RuntimeError, match="pa_palette_argmin"):
        E.class_map(np.zeros((2, 2, 3), np.uint8), np.zeros((5000, 3), np.float32))


# ---- 4. palette argmin
@pytest.mark.parametrize("dist_type", ["abs", "square", "mean"])
def test_palette_argmin_matches_the_evaluator(golden, dist_type):
    rng = np.random.default_rng(9)
    pal150 = golden["palette"]
    pal37 = rng.integers(0, 256, (37, 3))
    pal37[20] = pal37[3]                                                     # a duplicate colour: the first index wins
    pic = C.picture(91, 200, 301)
    pic[:40, :150] = pal150[rng.integers(0, 150, (40, 150))]                 # palette colours only: distance 0
    pic[40:60, :37] = pal37[None, :, :]
    pic[60:80] = 128                                                          # equidistant from many colours
    ties_pal = np.array([[10, 0, 0], [0, 10, 0], [0, 0, 10], [10, 0, 0]])
    for pal in (pal150, pal37, ties_pal):
        ref = H.class_map(pic, pal, dist_type)
        got = E.class_map(pic, pal, dist_type)
        assert got.dtype == np.int32 and np.array_equal(got, ref), (len(pal), dist_type)
    zero = np.zeros((3, 5, 3), np.uint8)
    assert (E.class_map(zero, ties_pal, dist_type) == 0).all()                # exact three-way tie
    only = np.ascontiguousarray(pal150[rng.integers(0, 150, (64, 70))].astype(np.uint8))
    assert np.array_equal(E.class_map(only, pal150, dist_type), H.class_map(only, pal150, dist_type))


# ---- 5. the engine against what the unmodified scripts produced
@pytest.mark.parametrize("task", list(H.SCRIPTS))
def test_engine_reproduces_the_scripts(golden, task):
    net = C.StandInModel()
    eng = _engine(task, model=C.Wrapped(net))                                # the scripts hand over a DDP-wrapped model
    pictures = C.query_pictures(task)
    sizes = [C.out_size(task, h, w) for (_, h, w) in C.QUERIES[task]]
    outs = eng.run(pictures, sizes=sizes if task == "sidd" else None)
    assert len(net.calls) == len(pictures) and all(c["batch"] == len(pictures) for c in net.calls)         # ONE forward
    for i, out in enumerate(outs):
        key = "%s.%d." % (task, i)
        call = net.calls[i]
        assert call["x"] == str(golden[key + "x_digest"]) and call["tgt"] == str(golden[key + "tgt_digest"])
        assert call["masked"] == int(golden[key + "masked"]) and call["second_half"] and call["valid_ok"]
        assert tuple(golden[key + "out_shape"]) == out.shape and str(golden[key + "out_dtype"]) == str(out.dtype)
        if out.dtype == np.float64:
            ref = golden[key + "out_sample"]
            assert np.abs(out[::C.SAMPLE_STRIDE, ::C.SAMPLE_STRIDE] - ref).max() <= BICUBIC_GATE * max(1.0, np.abs(ref).max())
        else:
            assert C.digest(out) == str(golden[key + "out_digest"])


def test_run_one_image_writes_the_scripts_file(golden, tmp_path):
    prompt, prompt_tgt = C.prompt_pair()
    for task in ("ade20k_semseg", "nyuv2_depth", "lol"):
        s, h, w = C.QUERIES[task][0]
        img, tgt = H.canvases(prompt, prompt_tgt, C.picture(s, h, w), C.RES)
        path = str(tmp_path / (task + ".png"))
        ret = E.run_one_image(img, tgt, (w, h), C.Wrapped(C.StandInModel()), path, "cuda", task)
        key = task + ".0."
        if task == "lol":
            ref = golden[key + "out_sample"]
            assert ret.dtype == np.float64 and np.abs(ret[::C.SAMPLE_STRIDE, ::C.SAMPLE_STRIDE] - ref).max() <= BICUBIC_GATE * max(1.0, np.abs(ref).max())
        else:
            from PIL import Image
            assert ret is None
            out = np.array(Image.open(path))
            assert C.digest(out.astype(np.int32) if task == "nyuv2_depth" else out) == str(golden[key + "out_digest"])


# ---- 6. batching
@pytest.mark.parametrize("task", ["ade20k_semseg", "nyuv2_depth", "derain"])
def test_a_batch_equals_its_pictures_one_by_one(task):
    shapes = [(480, 640), (200, 300), (333, 517), (600, 450), (97, 1000)]
    pictures = [C.picture(300 + i, h, w) for i, (h, w) in enumerate(shapes)]
    single = [_engine(task, batch_size=1).run([p])[0] for p in pictures]
    for bs in (8, 2):                                                        # one batch of 5; 2 + 2 + 1
        net = C.StandInModel()
        outs = _engine(task, batch_size=bs, model=net).run(pictures)
        assert [c["batch"] for c in net.calls] == ([5] * 5 if bs == 8 else [2, 2, 2, 2, 1])
        for a, b, (h, w) in zip(outs, single, shapes):
            assert a.shape[:2] == (h, w) and a.dtype == b.dtype and np.array_equal(a, b)


# ---- 7. a real (small) Painter module
class _Recorder:
    def __init__(self, model):
        self.model, self.patch_size, self.patch_embed, self.preds = model, model.patch_size, model.patch_embed, []

    @property
    def training(self):
        return self.model.training

    def eval(self):
        self.model.eval()
        return self

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def __call__(self, *a, **k):
        out = self.model(*a, **k)
        self.preds.append(out[1].detach().float().cpu().numpy())
        return out


@pytest.mark.parametrize("task", ["coco_pano_semseg", "coco_pose", "nyuv2_depth", "sidd"])
def test_end_to_end_on_a_small_painter(task):
    import torch.nn as nn

    from oracle import painter_oracle as O
    from painter_amd import models_painter
    cfg = O.small_config()
    m = models_painter.Painter(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               drop_path_rate=0.1, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), use_rel_pos=True,
                               decoder_embed_dim=cfg.decoder_embed_dim, compute_dtype="fp32")
    m.load_state_dict(O.random_params(cfg, 7), strict=True)
    m = m.to("cuda").train()                                                # run() switches to eval and back
    rec = _Recorder(m)
    res = cfg.img_size[1]
    eng = E.PainterEngine(rec, "cuda", task, *C.prompt_pair(), input_size=res, batch_size=4)
    shapes = [(120, 160), (50, 40), (64, 64)]
    pictures = [C.picture(500 + i, h, w) for i, (h, w) in enumerate(shapes)]
    outs = eng.run(pictures)
    assert m.training and len(rec.preds) == 1 and rec.preds[0].shape == (3, 2 * (res // 16) * (res // 16), 768)
    for i, (h, w) in enumerate(shapes):
        ref = H.decode(task, rec.preds[0][i], (w, h), res, res, 16)
        if ref.dtype == np.float64:
            assert np.abs(outs[i] - ref).max() <= BICUBIC_GATE * max(1.0, np.abs(ref).max())
        else:
            assert outs[i].dtype == ref.dtype and np.array_equal(outs[i], ref)
    assert len({o.tobytes() for o in outs}) == 3 and all(np.isfinite(o).all() for o in outs)


# ---- 8. no fallback
def test_cpu_device_raises():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.PainterEngine(C.StandInModel(), "cpu", "ade20k_semseg", *C.prompt_pair())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.run_one_image(np.zeros((896, 448, 3)), np.zeros((896, 448, 3)), (4, 4), C.StandInModel(), None, "cpu", "lol")
