"""Guard-band tests of the C ABI entry points that never go through painter_amd/ops.py: the ones painter_engine, seggpt_engine,
pair_pipeline, optim and engine drive.  tests/test_guard_bands_gpu.py covers the ops.py half.

Each case runs its calls twice on the same inputs:
  (a) the ordinary way, through the public wrapper, buffers from torch's caching allocator;
  (b) under tests/guard_bands.guarded_ops + CountingLib: every device tensor the wrapper accepts is first copied into, and every output,
      packed output buffer and workspace the module allocates (torch.empty / zeros / full) comes from, a byte buffer
      [4 MiB guard | payload | 4 MiB guard] pre-filled with 0xFF -- a workspace at EXACTLY the bytes its pa_*_workspace_bytes helper returns.
and asserts that no guard byte changed, that every entry point the case names was reached, that (b) equals (a) byte for byte in every
section the wrapper exposes, and that the results equal the family's host definition as the family's own GPU test compares them (the
case does that comparison itself, in both runs).  A guard cannot see one section of a packed buffer running into the next; the byte
equality with (a) and with the host definition covers that.

What the harness does not reach: tables a wrapper uploads itself (`torch.from_numpy(..).to(device)`, pinned job tables) come from torch's
allocator in both runs.  They are inputs of a few dozen bytes, read only."""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests.guard_bands import Arena, CountingLib, abi_symbols, guarded_ops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Ctx:
    """What a case builds its device inputs and reaches the library with: run (a) has arena = None and the real library."""

    def __init__(self, arena=None, counting=None):
        self.arena = arena
        self.lib = counting if counting is not None else lib
        self.ws_calls = []                 # (bytes asked, tensor) of the ops.workspace calls of the guarded run

    @property
    def guarded(self):
        return self.arena is not None

    def dev(self, x, name=None):
        """numpy array or tensor -> CUDA tensor; in (b) an exact-size arena tensor surrounded by 0xFF"""
        t = x if torch.is_tensor(x) else torch.from_numpy(np.array(x, order="C"))          # (a copy: the cached palettes are read-only)
        t = t.to(DEV).contiguous()
        return t if not self.guarded else self.arena.place(t, name=name)

    def devs(self, xs):
        return [self.dev(x) for x in xs]

    def buf(self, shape, dtype, fill=None):
        """an output a direct call has to bring: torch.empty in (a), an arena tensor in (b)"""
        t = torch.empty(shape, dtype=dtype, device=DEV) if not self.guarded else self.arena.empty(shape, dtype)
        return t if fill is None else t.fill_(fill)

    def holds(self, what, tensor, nbytes):
        """The case's claim that `tensor` is the workspace of exactly `nbytes` its helper returned; in (b) it must also be the arena's."""
        assert nbytes >= 0 and tensor.numel() * tensor.element_size() == nbytes, "%s: %d bytes allocated, the helper returned %d" % (
            what, tensor.numel() * tensor.element_size(), nbytes)
        if self.guarded:
            assert any(a.tensor.data_ptr() == tensor.data_ptr() and a.payload_bytes == nbytes for a in self.arena.allocs), "%s is not an arena tensor" % what


def host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else t


def same_bytes(name, a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), name
        for k in a:
            same_bytes("%s/%s" % (name, k), a[k], b[k])
        return
    if isinstance(a, (list, tuple)) and any(isinstance(x, (np.ndarray, torch.Tensor, dict, list, tuple)) for x in a):
        assert len(a) == len(b), name
        for i, (x, y) in enumerate(zip(a, b)):
            same_bytes("%s[%d]" % (name, i), x, y)
        return
    if isinstance(a, (np.ndarray, torch.Tensor)):
        assert type(a) is type(b) and a.shape == b.shape and a.dtype == b.dtype, (name, type(a), type(b), a.shape, b.shape, a.dtype, b.dtype)
        if torch.is_tensor(a):                                             # (as bytes: numpy has no bfloat16)
            a, b = (t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy() for t in (a, b))
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        diff = int((a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)).sum())
        assert diff == 0, "%s: the guarded run differs from the ordinary one in %d byte(s) of %d" % (name, diff, a.nbytes)
        return
    assert a == b or (a != a and b != b), "%s: (a) %r, (b) %r" % (name, a, b)


CASES = []


def case(id_, modules, symbols):
    """modules: names of the painter_amd modules whose `torch` and `lib` the guarded run replaces; symbols: the C entry points the case
    claims (kernel-enqueuing ones and the size helpers it holds them to)."""
    def deco(fn):
        CASES.append(pytest.param(fn, tuple(modules), tuple(symbols), id=id_))
        return fn
    return deco


def run_case(fn, modules, symbols, monkeypatch):
    import importlib
    res_a = fn(Ctx())
    torch.cuda.synchronize()
    arena, counting = Arena(DEV), CountingLib(lib)
    ctx = Ctx(arena, counting)
    with contextlib.ExitStack() as stack, monkeypatch.context() as m:
        for name in modules:
            mod = importlib.import_module("painter_amd." + name)
            calls = stack.enter_context(guarded_ops(monkeypatch, arena, ops=mod, exact_workspace=True))
            if hasattr(mod, "workspace"):
                ctx.ws_calls = calls
            m.setattr(mod, "lib", counting)
        res_b = fn(ctx)
    arena.check()
    missing = [s for s in symbols if not counting.calls.get(s)]
    assert not missing, "the case says it covers %s but never called them (called: %s)" % (missing, sorted(counting.calls))
    same_bytes("result", res_a, res_b)


@pytest.mark.parametrize("fn,modules,symbols", CASES)
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, modules, symbols, monkeypatch)


def offsets_inside(what, total, offsets_and_sizes):
    """The *_workspace_offset helpers: every section starts at or after the previous one's end and ends inside the helper's total."""
    end = 0
    for i, (off, size) in enumerate(offsets_and_sizes):
        assert off >= end and off + size <= total, "%s: section %d [%d, %d) against the previous end %d and the total %d" % (what, i, off, off + size, end, total)
        end = off + size


# ------------------------------------------------------------------------------------------------ instance decode
_memo = {}


def memo(key, make):
    """A host definition's result, computed once per session and never modified."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _inst_picture(seed, h, w):
    from tests.painter_inst_cases import painted_picture
    return memo(("inst picture", seed, h, w), lambda: painted_picture(seed, h, w, n_obj=14 if h > 30 else 4))


def _inst_decode(h, w, thr, nms_pre, max_num, tail, seed=13, black=False):
    def fn(c):
        from tests import painter_inst_host as H
        from tests.test_painter_inst_gpu import _compare_result
        pal = E.location_palette()
        pic = np.zeros((h, w, 3), np.uint8) if black else _inst_picture(seed, h, w)
        ref = memo(("inst", h, w, tuple(thr), nms_pre, max_num, seed, black), lambda: H.decode(pic, pal, thr, nms_pre, max_num))
        k, m = len(pal), len(thr) * len(pal)
        dec = E.InstanceDecode(c.dev(pic, "picture"), None, thr, nms_pre, max_num, "gaussian", 2.0, tail=tail)
        shape = (h, w, k, len(thr), nms_pre)
        total = lib.pa_inst_workspace_bytes(*shape)
        c.holds("pa_inst_decode's workspace", dec.workspace, total)
        assert dec.workspace.data_ptr() % 256 == 0
        stride, words = int(lib.pa_inst_workspace_offset(*shape, 9)), (h * w + 31) // 32
        assert stride % 4 == 0 and words <= stride < words + 4
        sizes = [4 * m, 8 * m, 8, 4 * nms_pre, 4 * nms_pre, 8 * nms_pre, 4 * nms_pre * stride, 4 * nms_pre * nms_pre, 8 * nms_pre]
        offsets_inside("pa_inst_workspace_offset%s" % (shape,), total, sorted((int(lib.pa_inst_workspace_offset(*shape, s)), sizes[s]) for s in range(9)))
        end = dec.obytes + max_num * h * w                                    # an empty tail takes no room, not even its padding
        assert dec.out.numel() == (dec.tail + tail if tail else end) and end <= dec.tail < end + 16 and dec.tail % 16 == 0
        if tail:
            dec.out[dec.tail:].fill_(0x5A)                                    # what a caller chains behind the decode; the decode ran before
        res = dec.result(with_f64=True, with_bits=True)
        live, n_surv = dec.section(2, np.int32, 2)
        assert live == ref["live"] and n_surv == len(ref["survivors"]) == min(live, nms_pre)
        r = dict(res, out=dec.out, n=dec.section(0, np.uint32, m), s=dec.section(1, np.uint64, m), counts=dec.section(2, np.int32, 2),
                 survivors=dec.section(3, np.int32, nms_pre)[:n_surv], areas=dec.section(4, np.int32, nms_pre)[:n_surv],
                 pre=dec.section(5, np.float64, nms_pre)[:n_surv])
        assert np.array_equal(r["n"], ref["n"]) and np.array_equal(r["s"], ref["s"]) and np.array_equal(r["survivors"], ref["survivors"])
        if ref.get("empty"):
            assert black and res["scores"].tolist() == [0.0] and res["candidates"].tolist() == [-1] and not res["masks"].any()
            assert not dec.out[:dec.tail].any()                               # count 0, every entry past it 0
            return r
        assert np.array_equal(r["areas"], ref["areas"]) and np.abs(r["pre"] - ref["survivor_scores"]).max() <= 4 * np.finfo(np.float64).eps
        bits = dec.section(6, np.uint32, nms_pre * stride).reshape(nms_pre, stride)[:n_surv]
        assert np.array_equal(bits[:, :words], H.pack_bits(ref["survivor_masks"])) and not bits[:, words:].any()
        inter = dec.section(7, np.int32, nms_pre * nms_pre).reshape(nms_pre, nms_pre)[:n_surv, :n_surv]
        upper = np.triu(np.ones((n_surv, n_surv), bool), 1)
        assert np.array_equal(inter[upper], ref["inter"][upper])
        r["bits_ws"], r["inter_upper"] = bits, inter[upper]
        _compare_result(res, ref, max_num)
        n = len(res["scores"])
        a = dec.out.cpu().numpy()
        for name in ("scores_f64", "scores", "candidates"):                    # "Entries past n are 0"
            assert not E._section(a, dec.at, name)[n:].any(), name
        assert not E._section(a, dec.at, "bits")[n * words:].any() and not E._section(a, dec.at, "masks")[n * h * w:].any()
        assert not tail or bool((dec.out[dec.tail:] == 0x5A).all())
        return r
    return fn


INST = ("pa_inst_decode", "pa_inst_workspace_bytes", "pa_inst_workspace_offset")
for h_, w_, thr_, pre_, top_, tail_ in [(61, 83, [19.0], 65, 65, 0), (61, 83, [19.0], 65, 1, 48), (61, 83, [19.0], 257, 257, 0), (61, 83, [19.0], 257, 1, 0),
                                        (61, 83, [19.0], 1, 1, 0), (7, 5, [30.0], 65, 65, 16),
                                        (23, 19, [3.0, 6.0, 9.0, 12.0, 15.0, 19.0, 25.0, 40.0], 257, 257, 0)]:
    case("inst_decode-%dx%d-thr%d-pre%d-top%d-tail%d" % (h_, w_, len(thr_), pre_, top_, tail_), ["painter_engine"], INST)(
        _inst_decode(h_, w_, thr_, pre_, top_, tail_))
case("inst_decode-no-candidate-37x53", ["painter_engine"], INST)(_inst_decode(37, 53, [5.0], 65, 65, 32, black=True))


@case("inst_stats-and-intersections-direct", [], ("pa_inst_stats", "pa_inst_intersections"))
def _inst_direct(c):
    from tests import painter_inst_host as H
    r = {}
    pal = E.location_palette()
    for (h, w), thr in (((61, 83), [19.0]), ((7, 5), [3.0, 6.0, 9.0, 12.0, 15.0, 19.0, 25.0, 40.0])):
        pic = _inst_picture(5, h, w)
        m = len(thr) * len(pal)
        n, s = c.buf((m,), torch.int32, 7), c.buf((m,), torch.int64, 7)
        assert c.lib.pa_inst_stats(c.dev(pic).data_ptr(), c.dev(pal).data_ptr(), c.dev(np.array(thr, np.float32)).data_ptr(), n.data_ptr(), s.data_ptr(),
                                   h, w, len(pal), len(thr), E._stream()) == 0
        hn, hs = H.stats(pic, pal, thr)
        assert np.array_equal(host(n), hn) and np.array_equal(host(s), hs)
        r["n%d" % h], r["s%d" % h] = n, s
    for rows, words, ld in ((65, 4, 65 + 3), (130, 36, 130 + 5), (1, 4, 2)):
        rng = np.random.default_rng(rows)
        masks = rng.random((rows, words * 32)) < 0.4
        out = c.buf((rows, ld), torch.int32, -1)
        assert c.lib.pa_inst_intersections(c.dev(H.pack_bits(masks).view(np.int32)).data_ptr(), rows, words, out.data_ptr(), ld, E._stream()) == 0
        got, ref = host(out), H.intersections(masks)
        upper = np.triu(np.ones((rows, rows), bool), 1)
        assert np.array_equal(got[:, :rows][upper], ref[upper]) and not got[:, rows:].any()                # cleared up to ld, nothing behind the last row
        r["inter%d" % rows] = out
    return r


# ------------------------------------------------------------------------------------------------ Painter stitch, decodes, palette argmin
def _painter_decode(sizes, seed):
    """sizes: (height, width) per sample.  Every task kind in one case: bilinear and nearest uint8, depth, bicubic float64 with and
    without the second (saved) output buffer."""
    def fn(c):
        from tests import painter_eval_cases as C
        from tests import painter_eval_host as H
        from tests.test_painter_eval_gpu import BICUBIC_GATE
        n = len(sizes)
        toks, toks64 = C.tokens(seed, n=n), C.tokens(seed + 1, n=n, gain=1.5)
        wh = [(w, h) for h, w in sizes]
        r = {}
        for task in ("ade20k_semseg", "coco_pose", "nyuv2_depth"):
            plan = E.decode(task, c.dev(toks), wh, C.RES, C.RES, C.PATCH)
            assert plan.out.numel() == sum(h * w * (1 if task == "nyuv2_depth" else 3) for h, w in sizes)
            r[task] = plan.out
            for i, got in enumerate(plan.pictures()):
                ref = memo(("decode", task, seed, n, i, sizes[i]), lambda: H.decode(task, toks[i], wh[i], C.RES, C.RES, C.PATCH))
                assert got.dtype == ref.dtype and np.array_equal(got, ref), (task, sizes[i])
        pred = c.dev(toks64)
        plan = E.decode("derain", pred, wh, C.RES, C.RES, C.PATCH, saved=True)
        assert plan.out8.numel() == plan.out.numel() == sum(3 * h * w for h, w in sizes)
        r["f64"], r["saved"], r["f64_alone"] = plan.out, plan.out8, E.decode("derain", pred, wh, C.RES, C.RES, C.PATCH).out
        assert torch.equal(r["f64"], r["f64_alone"])
        for i, (got, got8) in enumerate(zip(plan.pictures(), plan.saved_pictures())):
            ref = memo(("decode", "derain", seed, n, i, sizes[i]), lambda: H.decode("derain", toks64[i], wh[i], C.RES, C.RES, C.PATCH))
            assert got.dtype == np.float64 and np.abs(got - ref).max() <= BICUBIC_GATE * max(1.0, float(np.abs(ref).max())), sizes[i]
            diff = got8 != H.saved_picture(ref)
            assert not (diff & ~(np.abs(ref * 255.0 - np.round(ref * 255.0)) <= 1e-9 * 255.0)).any(), sizes[i]
            assert np.array_equal(got8, H.saved_picture(got))                      # the device's clip * 255 of its own float64 values
        return r
    return fn


DECODES = ("pa_painter_decode_u8", "pa_painter_decode_depth", "pa_painter_decode_f64")
case("painter_decode-batch3-1x7-9x1-5x3", ["painter_engine"], DECODES)(_painter_decode([(1, 7), (9, 1), (5, 3)], 31))
case("painter_decode-batch1-1x1", ["painter_engine"], DECODES)(_painter_decode([(1, 1)], 33))
case("painter_decode-batch1-37x1", ["painter_engine"], DECODES)(_painter_decode([(37, 1)], 35))


def _painter_stitch(n, res):
    def fn(c):
        from tests import painter_eval_cases as C
        from tests import painter_eval_host as H
        rng = np.random.default_rng(41 + n)
        prompt, target = (rng.integers(0, 256, (res, res, 3), dtype=np.uint8) for _ in range(2))
        queries = rng.integers(0, 256, (n, res, res, 3), dtype=np.uint8)
        eng = E.PainterEngine(C.StandInModel(), "cuda", "ade20k_semseg", prompt, target, input_size=res)
        eng.prompt, eng.prompt_tgt = c.dev(eng.prompt), c.dev(eng.prompt_tgt)
        imgs, tgts = eng.stitch(c.dev(queries))
        assert tuple(imgs.shape) == (n, 3, 2 * res, res) == tuple(tgts.shape)
        for i in range(n):
            x, tt = H.model_inputs(*H.canvases(prompt, target, queries[i], res, query_is_resized=True))
            assert np.array_equal(host(imgs[i:i + 1]), x) and np.array_equal(host(tgts[i:i + 1]), tt)
        return dict(imgs=imgs, tgts=tgts)
    return fn


case("painter_stitch-batch1-res16", ["painter_engine", "seggpt_engine"], ("pa_painter_stitch",))(_painter_stitch(1, 16))
case("painter_stitch-batch3-res48", ["painter_engine", "seggpt_engine"], ("pa_painter_stitch",))(_painter_stitch(3, 48))


@case("palette_argmin-1x7-9x1-61x83", ["painter_engine"], ("pa_palette_argmin",))
def _palette_argmin(c):
    from tests import painter_eval_cases as C
    from tests import painter_eval_host as H
    rng = np.random.default_rng(9)
    pal = rng.integers(0, 256, (37, 3))
    pal[20] = pal[3]                                                           # a duplicate colour: the first index wins
    r = {}
    for h, w in ((1, 7), (9, 1), (61, 83)):
        pic = C.picture(91 + h, h, w)
        pic[:, : w // 2] = pal[rng.integers(0, 37, (h, w // 2))]
        for dist in ("abs", "square", "mean"):
            got = E.class_map(c.dev(pic), pal, dist)
            assert got.dtype == np.int32 and np.array_equal(got, H.class_map(pic, pal, dist)), (h, w, dist)
            r["%dx%d-%s" % (h, w, dist)] = got
    return r


# ------------------------------------------------------------------------------------------------ SegGPT pre- and post-processing
@case("seggpt_resize-odd-row-bytes-and-a-49155-byte-row", ["seggpt_engine"], ("pa_resample_u8", "pa_gather_u8"))
def _seggpt_resize(c):
    """Source rows of w * 3 bytes with w * 3 % 4 = 1, 2, 3 (w = 3, 2, 1: the rows are staged through aligned dword loads), upscaling
    from a source one pixel wide, and a 2-row source whose rows of 16385 * 3 = 49155 bytes exceed 48 KiB (the route without LDS)."""
    from PIL import Image
    from painter_amd import seggpt_engine as S
    from tests import seggpt_io_cases as C
    io = S.DeviceIO("cuda")
    r = {}
    for h, w, oh, ow in ((5, 3, 7, 6), (4, 2, 3, 5), (6, 1, 4, 9), (1, 9, 4, 4), (2, 16385, 3, 40), (7, 5, 7, 2), (7, 5, 3, 5)):
        assert (h, w) != (2, 16385) or w * 3 > 48 << 10
        a = C.picture(h * 1000 + w, h, w)
        d = c.dev(a)
        got = io.resize(d, (ow, oh))
        assert np.array_equal(host(got), np.array(Image.fromarray(a).resize((ow, oh)))), (h, w, oh, ow)
        near = io.resize(d, (ow, oh), nearest=True)
        assert np.array_equal(host(near), np.array(Image.fromarray(a).resize((ow, oh), Image.NEAREST))), (h, w, oh, ow)
        r["%dx%d->%dx%d" % (h, w, oh, ow)], r["%dx%d->%dx%d nearest" % (h, w, oh, ow)] = got, near
    return r


def _seggpt_post(n_prompts):
    def fn(c):
        from oracle import seggpt_io_oracle as O
        from painter_amd import seggpt_engine as S
        from tests import seggpt_io_cases as C
        hres, res, patch = 32, 48, 16
        io = S.DeviceIO("cuda", res=res, hres=hres, patch=patch)
        rng = np.random.default_rng(31 + n_prompts)
        prompts = rng.integers(0, 256, (n_prompts, hres, res, 3), dtype=np.uint8)
        targets = rng.integers(0, 256, (n_prompts, hres, res, 3), dtype=np.uint8)
        targets[1:] = targets[1:] & 1                                          # cached video masks: {0,1}, used undivided
        query = rng.integers(0, 256, (hres, res, 3), dtype=np.uint8)
        div = [255.0] + [1.0] * (n_prompts - 1)
        imgs, tgts = io.stitch(c.dev(prompts), c.dev(targets), c.dev(query), div)
        ri, rt = O.stitch(prompts, targets, query, div)
        assert np.array_equal(host(imgs), ri) and np.array_equal(host(tgts), rt)
        y = torch.randn((2 * hres // patch) * (res // patch), patch * patch * 3, generator=torch.Generator().manual_seed(n_prompts)) * 1.5
        near = (128.0 / 255 - torch.tensor(O.IMAGENET_MEAN).repeat(256)) / torch.tensor(O.IMAGENET_STD).repeat(256)
        y[-3] = near.float()                                                  # de-normalises to ~128 per channel: the mask threshold
        y[-2], y[-1] = -40.0, 40.0                                            # saturate at 0 and at 255
        yd = c.dev(y)
        r = dict(imgs=imgs, tgts=tgts, decode=io.decode(yd), mask=io.mask(yd))
        assert np.array_equal(host(r["decode"]), O.decode(y.numpy(), hres, res, patch)) and np.array_equal(host(r["mask"]), O.mask(y.numpy(), hres, res, patch))
        for h0, w0 in ((5, 7), (1, 9), (61, 1)):
            frame = C.picture(h0 + w0, h0, w0)
            frame[: max(h0 // 4, 1), : max(w0 // 2, 1)] = 255
            r["blend %dx%d" % (h0, w0)] = io.blend(yd, c.dev(frame))
            assert np.array_equal(host(r["blend %dx%d" % (h0, w0)]), O.blend(y.numpy(), frame, hres, res, patch)), (h0, w0)
        return r
    return fn


SEGGPT_POST = ("pa_seggpt_stitch", "pa_seggpt_decode", "pa_seggpt_mask", "pa_seggpt_blend")
case("seggpt_stitch-decode-mask-blend-1-prompt", ["seggpt_engine"], SEGGPT_POST)(_seggpt_post(1))
case("seggpt_stitch-decode-mask-blend-3-prompts", ["seggpt_engine"], SEGGPT_POST)(_seggpt_post(3))


# ------------------------------------------------------------------------------------------------ pose keypoints
def _pose(name):
    """name -> (pictures, flipped or None, palette or None, flip_pairs): n = 1 with K = 1; K = 17 with flipped pictures at h * w < 256
    (8 x 6), at h * w = 2049 = 3 x 683 (one pixel into a second chunk of 2048) and on the hand-built 9 x 11 boxes, whose `edges` box
    has a peak in every border row and column."""
    def fn(c):
        from tests import painter_pose_cases as C
        from tests import painter_pose_host as H
        if name == "n1-K1-5x4":
            pal, pairs = C.custom_palette(1)
            p, q = C.painted_pair(3, 1, 5, 4, palette=pal, pair=H.pair_table(pairs, 1), noise=8)
            q = None
        else:
            pal, pairs = None, C.FLIP_PAIRS
            p, q = C.hand_boxes()[:2] if name == "hand-9x11" else C.painted_pair(16, 3, 3, 683) if name == "3x683" else C.shape_pair("8x6")
        hp, hpair = (C.PALETTE, C.PAIR) if pal is None else (pal, H.pair_table(pairs, len(pal) - 1))
        dp, dq = c.dev(p), None if q is None else c.dev(q)
        r = {}
        for shift in (True, False):
            dec = E.PoseDecode(dp, dq, pal, pairs, shift)
            c.holds("pa_pose_keypoints's workspace", dec.workspace, lib.pa_pose_workspace_bytes(dec.n, dec.k))
            assert dec.out.numel() == 3 * dec.n * dec.k
            got = dec.result()
            ref = memo(("pose", name, shift), lambda: H.keypoints(p, q, hp, hpair, shift=shift))
            assert got["preds"].dtype == np.float32 and np.array_equal(got["preds"], ref["preds"]) and np.array_equal(got["maxvals"], ref["maxvals"])
            heat = E.PoseDecode(dp, dq, pal, pairs, shift, heatmaps=True).out
            assert tuple(heat.shape) == (dec.n, dec.k) + tuple(p.shape[1:3])
            assert np.array_equal(host(heat), memo(("heat", name, shift), lambda: H.heatmaps(p, q, hp, hpair, shift=shift)))
            r["out%d" % shift], r["heat%d" % shift] = dec.out, heat
        if name == "hand-9x11":
            preds, maxvals = C.hand_expected()
            got = E.PoseDecode(dp, dq, pal, pairs, True).result()
            assert np.array_equal(got["preds"], preds) and np.array_equal(got["maxvals"], maxvals)
        return r
    return fn


for name_ in ("n1-K1-5x4", "8x6", "3x683", "hand-9x11"):
    case("pose-" + name_, ["painter_engine"], ("pa_pose_keypoints", "pa_pose_heatmaps", "pa_pose_workspace_bytes"))(_pose(name_))


# ------------------------------------------------------------------------------------------------ semantic confusion, depth errors
def _semseg(k, every_ignored=False):
    def fn(c):
        from tests import painter_score_cases as C
        from tests import painter_score_host as H
        pal = C.synthetic_palette(k)
        shapes = [(1, 1), (7, 5), (61, 83)]                                    # three jobs of different sizes in one table; 5063 pixels: no multiple of 64
        pairs = [C.noisy_case(k + i, h, w, pal, ignore=k < 255) for i, (h, w) in enumerate(shapes)]
        pics, gts = [p for p, _ in pairs], [np.full_like(g, C.IGNORE) if every_ignored else g for _, g in pairs]
        ref = memo(("semseg", k, every_ignored), lambda: H.confusion(pics, gts, pal)[0])
        r = {"lds": lib.pa_semseg_lds_bins(k)}
        for bins in (0, 1):
            score = E.SemsegScore(pal)
            score.bins = bins
            assert score.out.numel() == 8 * ((k + 1) ** 2 + 1)
            got = score.add(c.devs(pics), c.devs(gts)).matrix()
            assert np.array_equal(got, ref) and got.sum() == sum(h * w for h, w in shapes)
            assert not every_ignored or got[:, :-1].sum() == 0
            score.add(c.devs(pics[:1]), c.devs(gts[:1]))                        # accumulated in place
            r["out%d" % bins] = score.out
            assert score.matrix().sum() == got.sum() + 1
        return r
    return fn


SEMSEG = ("pa_semseg_confusion",)
case("semseg-k1", ["painter_engine"], SEMSEG)(_semseg(1))
case("semseg-k199-lds", ["painter_engine"], SEMSEG)(_semseg(199))
case("semseg-k200-global", ["painter_engine"], SEMSEG)(_semseg(200))
case("semseg-k37-every-pixel-ignored", ["painter_engine"], SEMSEG)(_semseg(37, every_ignored=True))


@case("depth_errors-1-job-3-jobs-flush-box-no-valid-pixel", ["painter_engine"], ("pa_depth_errors", "pa_depth_workspace_bytes"))
def _depth(c):
    """Two runs of pa_depth_errors give the same bits (include/painter_hip.h): (b) is held to the bits of (a), both to the statement at the
    gate of tests/test_painter_score_gpu.py."""
    from tests import painter_score_cases as C
    from tests.test_painter_score_gpu import _check_depth
    cases = [C.depth_case(31 + i, h, w) for i, (h, w) in enumerate([(37, 53), (1, 1), (64, 80)])]
    cases[1][1][0, 0] = 2000                                                  # the one pixel of the 1 x 1 picture is measured
    dev = lambda pairs: (c.devs([p for p, _ in pairs]), c.devs([g.view(np.int16) for _, g in pairs]))
    r = {}

    def run(tag, pairs, **kw):
        job = E.DepthErrors(*dev(pairs), **dict(E.DEPTH_DEFAULTS, **kw))
        c.holds("pa_depth_errors's workspace", job.workspace, max(lib.pa_depth_workspace_bytes(len(pairs)), 8))
        assert tuple(job.out.shape) == (len(pairs), 10)
        r[tag] = job.out
        metrics, n = job.result()
        for i, (p, g) in enumerate(pairs):
            _check_depth(p, g, kw, metrics[i], n[i], job.sums()[i])
        return n
    assert (run("three jobs", cases, max_depth=10.0) > 0).all()
    assert run("one job", cases[:1], max_depth=10.0)[0] > 0
    h, w = cases[0][0].shape
    assert run("box flush with the last row and column", cases[:1], crop=(h - 9, h, w - 11, w))[0] > 0
    assert run("one-pixel box in the last corner", cases[:1], crop=(h - 1, h, w - 1, w))[0] <= 1
    assert run("no valid pixel", [(cases[0][0], np.zeros_like(cases[0][1]))])[0] == 0
    return r


# ------------------------------------------------------------------------------------------------ restoration scores
def _restore(metric):
    """One window exactly (7 x 7 for skimage's window, 11 x 11 for the Gaussian), 23 x 37 (partial tiles both ways), 25 x 25 (one window
    past a 24-window tile for the 7 x 7 window: 19 windows; 11 x 11: 15), and tile + win (one window past the tile for either window);
    alone and as jobs of different sizes in one table.  Two runs give the same bits (include/painter_hip.h)."""
    def fn(c):
        from tests import painter_restore_cases as C
        from tests import painter_restore_host as H
        from tests.test_painter_restore_gpu import check_record
        win, tile = len(H.weights(metric)), lib.pa_restore_tile()
        assert tile == 24
        shapes = [(win, win), (23, 37), (25, 25), (tile + win, tile + win), (win, tile + win)]
        pairs = [C.inputs(*C.case("natural", 60 + i, h, w), metric) for i, (h, w) in enumerate(shapes)]
        ref = memo(("restore", metric), lambda: [H.sums(p, g, metric) for p, g in pairs])
        ch = 3 if metric == "skimage" else 1
        r = {}

        def run(tag, idx):
            job = E.RestorationScores(c.devs([pairs[i][0] for i in idx]), c.devs([pairs[i][1] for i in idx]), metric)
            tiles = sum(ch * -(-(shapes[i][0] - win + 1) // tile) * -(-(shapes[i][1] - win + 1) // tile) for i in idx)
            c.holds("pa_restore_scores's workspace", job.workspace, lib.pa_restore_workspace_bytes(len(idx), tiles))
            assert tuple(job.out.shape) == (len(idx), 8)
            for row, i in zip(job.sums(), idx):
                check_record(row, ref[i], metric, shapes[i])
            r[tag] = job.out
            return job.sums()
        mixed = run("all", range(len(shapes)))
        assert mixed[0, 3] == 1 and mixed[3, 3] == (tile + 1) ** 2
        for i in range(len(shapes)):
            assert run("alone %dx%d" % shapes[i], [i])[0].tobytes() == mixed[i].tobytes()
        run("two jobs", [1, 0])
        return r
    return fn


for metric_ in ("skimage", "matlab_y"):
    case("restore-" + metric_, ["painter_engine"], ("pa_restore_scores", "pa_restore_tile", "pa_restore_workspace_bytes"))(_restore(metric_))


# ------------------------------------------------------------------------------------------------ training input pipeline
def _allocated(c, what, nbytes):
    """A scratch buffer a wrapper keeps to itself: in (b) the arena must have handed out exactly the bytes the helper returned."""
    assert nbytes > 0, (what, nbytes)
    assert not c.guarded or any(a.payload_bytes == nbytes and a.tensor.dtype == torch.uint8 for a in c.arena.allocs), \
        "%s: no arena allocation of the %d bytes its helper returned" % (what, nbytes)


@case("pair_crops-boxes-at-byte-offsets-1-2-3-mod-4", ["pair_pipeline"], ("pa_resample_u8_box", "pa_gather_u8_box", "pa_resized_crop_u8_batch"))
def _pair_crops(c):
    """A 9 x 7 picture (rows of 21 bytes): boxes that start 21, 42 and 27 bytes in (1, 2, 3 mod 4) and end on the picture's last row and
    column, and the 1 x 1 box of its last pixel; both passes, the horizontal pass alone, the vertical pass alone, no pass; picture by
    picture and as one job table."""
    from PIL import Image
    from painter_amd import pair_pipeline as PP
    from tests.seggpt_io_cases import picture
    pipe = PP.DevicePairPipeline("cuda")
    img = picture(97, 9, 7)
    boxes = [(1, 0, 8, 7), (2, 0, 7, 7), (1, 2, 8, 5), (8, 6, 1, 1)]
    assert [(i * 7 + j) * 3 % 4 for i, j, _, _ in boxes] == [1, 2, 3, 2] and all(i + h == 9 and j + w == 7 for i, j, h, w in boxes)
    sizes = [(5, 6), (8, 6), (5, 7), (8, 7), (7, 5), (1, 1)]               # (8, 6): box 0 keeps its rows; (5, 7): its columns; (8, 7): both
    pil = lambda box, size, near: np.array(Image.fromarray(img).crop((box[1], box[0], box[1] + box[3], box[0] + box[2])).resize(
        (size[1], size[0]), Image.NEAREST if near else Image.BICUBIC))
    dev = c.dev(img)
    r = {}
    for box in boxes:
        for size in sizes:
            for near in (False, True):
                out = c.buf(size + (3,), torch.uint8, 0)
                pipe.resized_crop(dev, box, out, near)
                assert np.array_equal(host(out), pil(box, size, near)), (box, size, near)
                r["%s->%s %d" % (box, size, near)] = out
    for size in sizes:                                                       # the job table: every box, both interpolations, one output size
        jobs = [(box, near) for box in boxes for near in (False, True)]
        out = c.buf((len(jobs),) + size + (3,), torch.uint8, 0)
        pipe.resized_crop_batch([img] * len(jobs), [b for b, _ in jobs], [n for _, n in jobs], out)
        for k, (box, near) in enumerate(jobs):
            assert np.array_equal(host(out[k]), pil(box, size, near)), (box, size, near)
        r["batch->%s" % (size,)] = out
    return r


@case("pair_jitter-normalize-float-crops-valid", ["pair_pipeline"],
      ("pa_color_jitter", "pa_color_jitter_workspace_bytes", "pa_to_tensor_normalize", "pa_resized_crop_f32", "pa_resized_crop_f32_modes", "pa_pair_valid",
       "pa_pair_valid_workspace_bytes"))
def _pair_rest(c):
    from oracle import pair_pipeline_oracle as O
    from painter_amd import pair_pipeline as PP
    from tests.seggpt_io_cases import picture
    from tests.test_pair_pipeline_gpu import _jitter_batch
    pipe = PP.DevicePairPipeline("cuda")
    r = {}
    # ColorJitter in place: B = 1 with an odd h * w (5 x 7 = 35 pixels, 105 bytes), then six samples with every slot pattern
    ops, fac = _jitter_batch()
    for tag, (B, h, w) in (("one", (1, 5, 7)), ("six", (6, 9, 11))):
        imgs = np.stack([picture(90 + b, h, w) for b in range(B)])
        d = c.dev(imgs)
        assert pipe.color_jitter(d, ops[:B], fac[:B]) is d
        _allocated(c, "pa_color_jitter's workspace", lib.pa_color_jitter_workspace_bytes(B))
        for b in range(B):
            ref = O.color_jitter(imgs[b], ops[b], [O.hue_shift_byte(f) if o == PP.HUE else f for o, f in zip(ops[b], fac[b])])
            assert np.array_equal(host(d[b]), ref), (tag, b)
        r["jitter " + tag] = d
    # ToTensor + Normalize into rows [row0, row0 + h) of the canvas: row0 = 0 of an h-row canvas and the last h rows of a 2 h-row one --
    # the canvas ends exactly at the last written row
    for B, h, w in ((1, 5, 7), (3, 4, 6)):
        imgs = np.stack([picture(30 + b, h, w) for b in range(B)])
        flips = [False, True, True][:B]
        for canvas_h, row0 in ((h, 0), (2 * h, h)):
            canvas = c.buf((B, 3, canvas_h, w), torch.float32, 7.0)
            pipe.to_tensor_normalize(c.dev(imgs), flips, canvas, row0)
            got = canvas.cpu()
            assert float((got[:, :, :row0] - 7.0).abs().sum()) == 0.0
            for b in range(B):
                assert torch.equal(got[b, :, row0:], O.to_tensor_normalize(imgs[b], flips[b])), (B, b, row0)
            r["normalize %d %d" % (B, row0)] = canvas
    # the second crop on float canvases: boxes that end on the last row and column, the 1 x 1 box of the last pixel, the whole canvas
    H, W = 10, 6
    x = torch.randn(4, 3, H, W, generator=torch.Generator().manual_seed(5)) * 1.2
    boxes = [(3, 1, 7, 5), (H - 1, W - 1, 1, 1), (0, 0, H, W), (2, 3, 8, 3)]
    xd = c.dev(x)
    for near in (False, True):
        got = pipe.resized_crop_tensor(xd, boxes, near)
        for b, box in enumerate(boxes):
            ref = O.resized_crop_tensor(x[b], box, (H, W), near)
            if near:
                assert torch.equal(got[b].cpu(), ref), b
            else:                                                            # the gate of tests/test_pair_pipeline_gpu.py
                assert float((got[b].cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), b
        r["float crop %d" % near] = got
    modes = [0, 2, 1, 0]
    r["float crop modes"] = got = pipe.resized_crop_tensor_modes(xd, boxes, modes)
    for b, m in enumerate(modes):
        assert torch.equal(got[b], xd[b] if m == 2 else r["float crop %d" % (m == 1)][b]), b
    one = pipe.resized_crop_tensor_modes(xd[1:2], boxes[1:2], [0])
    assert torch.equal(one[0], r["float crop 0"][1])
    r["float crop modes B1"] = one
    # `valid`: B = 1 with a plane of 35 elements (every counted rule sees fewer than 300), then every rule in one call
    types = ["coco_image2pose", "ade20k_image2semantic", "nyuv2_image2depth", "coco_image2panoptic_inst", "ssid_2image_denoise",
             "coco_image2panoptic_sem_seg"]
    black = (torch.zeros(3) - torch.tensor(O.MEAN)) / torch.tensor(O.STD)
    for tag, (B, h, w) in (("B1 5x7", (1, 5, 7)), ("B6 19x17", (6, 19, 17))):
        tg = torch.randn(B, 3, h, w, generator=torch.Generator().manual_seed(6))
        tg[:, :, : h // 2] = black[:, None, None]
        got = pipe.valid_map(c.dev(tg), types[:B])
        _allocated(c, "pa_pair_valid's workspace", lib.pa_pair_valid_workspace_bytes(B))
        for b in range(B):
            assert torch.equal(got[b].cpu(), O.valid_map(tg[b], types[b])), (tag, b)
        r["valid " + tag] = got
    return r


# ------------------------------------------------------------------------------------------------ panoptic merge
PANO_KW = dict(overlap_threshold=0.3, stuff_area_thresh=20, instances_score_thresh=0.3)


def _pano_inputs(h, w, n, seed=6):
    """A semantic picture in the 133 COCO colours and n random boxes with many overlaps, equal scores among them."""
    from tests import painter_pano_cases as C
    from tests.test_painter_pano_gpu import _random_instances
    sem = C.picture_pair(seed, h, w, n_obj=5)[0]
    semmap, masks, scores, classes = _random_instances(seed, h, w, n, side=0.6)
    return sem, semmap, masks, scores + np.float32(0.25), classes


def _garbage_bits(masks, h, w):
    """bool [n][h][w] -> int32 [max(n, 1)][words] in the decode's bit layout with every padding bit of the last word SET."""
    from tests import painter_inst_host as IH
    bits = np.zeros((max(len(masks), 1), (h * w + 31) // 32), np.uint32)
    if len(masks):
        bits[:len(masks)] = IH.pack_bits(masks.reshape(len(masks), -1))
    if h * w % 32:
        bits[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(h * w % 32)
    return bits.view(np.int32)


def _pano(h, w, n, as_bits):
    """as_bits: the masks arrive as bit words with their padding bits set (pa_pano_vote / pa_pano_decode must ignore them); otherwise as
    bytes with any non-zero value, packed by pa_pack_mask_bits."""
    def fn(c):
        from tests import painter_pano_host as H
        from tests.test_painter_pano_gpu import _check_result, _same_segments
        sem, _, masks, scores, _ = _pano_inputs(h, w, n)
        pal = E.semantic_palette()
        assert as_bits or n > 0
        if as_bits:
            assert h * w % 32 != 0
            dmasks = c.dev(_garbage_bits(masks, h, w)[:n] if n else np.zeros((0, (h * w + 31) // 32), np.int32))
        else:
            dmasks = c.dev(masks.view(np.uint8) * np.random.default_rng(1).integers(1, 256, masks.shape).astype(np.uint8))
        r = {}
        for dist in ("abs", "mean"):
            got = E.classify_instances(c.dev(sem), dmasks, dist_type=dist)
            ref = memo(("vote", h, w, n, dist), lambda: H.vote(sem, pal, masks, 80, dist)[1] if n else np.zeros(0, np.int32))
            assert got.dtype == np.int32 and np.array_equal(got, ref[:n]), dist
            r["classes " + dist] = got
        given = (np.arange(max(n, 1)) * 7 % 80).astype(np.int32)[:n]
        for tag, classes in (("voted", None), ("given", given)):
            dec = E.PanopticDecode(c.dev(sem), supplied=dict(masks=dmasks, scores=scores, classes=classes), **PANO_KW)
            m = max(n, 1)
            c.holds("pa_pano_decode's workspace", dec.workspace, lib.pa_pano_workspace_bytes(h, w, 133, 80, m))
            assert dec.workspace.data_ptr() % 256 == 0 and dec.max_inst == m and dec.out.numel() == E.PanopticDecode.out_bytes(h, w, 133, 80, m)
            res = dec.result()
            if n:
                ref = memo(("pano", h, w, n, tag), lambda: H.panoptic(sem, pal, masks, scores, classes, **PANO_KW))
            else:                                                            # stuff only: the statement's single empty mask with score 0 adds nothing
                ref = memo(("pano", h, w, n), lambda: H.panoptic(sem, pal, np.zeros((1, h, w), bool), [0.0], None, **PANO_KW))
                assert len(res["classes"]) == 0 and not any(s["isthing"] for s in ref["segments"]) and ref["segments"]
            _check_result(dict(res, masks=masks), h, w)
            assert np.array_equal(res["panoptic"], ref["panoptic"]) and np.array_equal(res["areas"], ref["areas"])
            assert not n or np.array_equal(res["classes"], ref["classes"])
            _same_segments(res["segments"], ref["segments"])
            a = host(dec.out)
            cnt = int(E._section(a, dec.at, "count")[0])
            assert cnt == len(ref["segments"]) and not E._section(a, dec.at, "segments")[cnt:].view(np.uint8).any()      # entries past the count are 0
            r["out " + tag] = dec.out
        return r
    return fn


PANO = ("pa_pano_vote", "pa_pano_decode", "pa_pano_workspace_bytes")
case("pano-61x83-12-instances-padding-bits-set", ["painter_engine"], PANO)(_pano(61, 83, 12, True))
case("pano-61x83-12-instances-bytes", ["painter_engine"], PANO + ("pa_pack_mask_bits",))(_pano(61, 83, 12, False))
case("pano-3x683-2049-pixels-5-instances", ["painter_engine"], PANO)(_pano(3, 683, 5, True))
case("pano-3x683-2049-pixels-bytes", ["painter_engine"], PANO + ("pa_pack_mask_bits",))(_pano(3, 683, 5, False))
case("pano-7x5-max_inst-1", ["painter_engine"], PANO)(_pano(7, 5, 1, True))
case("pano-7x5-max_inst-1-bytes", ["painter_engine"], PANO + ("pa_pack_mask_bits",))(_pano(7, 5, 1, False))
case("pano-61x83-0-instances", ["painter_engine"], ("pa_pano_decode", "pa_pano_workspace_bytes"))(_pano(61, 83, 0, True))


@case("pano-behind-an-instance-decode-tail", ["painter_engine"], ("pa_inst_decode", "pa_pano_decode"))
def _pano_chained(c):
    """PanopticDecode writes into the tail of the InstanceDecode's output buffer and reads count, scores and bit masks where the decode
    left them: one packed buffer, every section compared."""
    from tests import painter_pano_cases as C
    from tests import painter_pano_host as H
    from tests.test_painter_pano_gpu import _same_segments
    h, w, max_num = 61, 83, 7
    sem, inst_pic = C.picture_pair(13, h, w)
    tail = E.PanopticDecode.out_bytes(h, w, 133, 80, max_num)
    dec = E.InstanceDecode(c.dev(inst_pic), None, [19.0], 65, max_num, "gaussian", 2.0, tail=tail)
    pano = E.PanopticDecode(c.dev(sem), decode=dec, **PANO_KW)
    assert pano.out is dec.out and dec.out.numel() == dec.tail + tail
    c.holds("pa_pano_decode's workspace", pano.workspace, lib.pa_pano_workspace_bytes(h, w, 133, 80, max_num))
    res = pano.result()
    inst = dec.result(with_bits=True)
    assert len(inst["scores"]) == max_num and np.array_equal(res["masks"], inst["masks"])
    ref = H.panoptic(sem, E.semantic_palette(), inst["masks"], inst["scores"], None, **PANO_KW)
    assert np.array_equal(res["panoptic"], ref["panoptic"]) and np.array_equal(res["classes"], ref["classes"]) and np.array_equal(res["areas"], ref["areas"])
    _same_segments(res["segments"], ref["segments"])
    return dict(out=dec.out, bits=inst["bits"])


@case("pano_merge-direct", [], ("pa_pano_merge",))
def _pano_merge(c):
    from tests.test_painter_pano_gpu import _compare_merge
    r = {}
    for h, w, n in ((61, 83, 12), (3, 683, 5), (7, 5, 1), (61, 83, 0)):
        _, semmap, masks, scores, classes = _pano_inputs(h, w, n)
        m, merge = max(n, 1), (0.3, 20, 0.3)
        sc, cl = np.zeros(m, np.float32), np.zeros(m, np.int32)
        sc[:n], cl[:n] = scores, classes
        ws = c.buf((lib.pa_pano_workspace_bytes(h, w, 133, 80, m),), torch.uint8)
        cap = m + 133 - 80
        pan, pic, out_n = c.buf((h, w), torch.int32, -1), c.buf((h, w, 3), torch.uint8, 77), c.buf((1,), torch.int32, -1)
        seg = c.buf((cap * E.SEGMENT.itemsize,), torch.uint8, 255)
        assert c.lib.pa_pano_merge(c.dev(semmap.astype(np.int32)).data_ptr(), c.dev(_garbage_bits(masks, h, w)).data_ptr(), c.dev(sc).data_ptr(),
                                   c.dev(cl).data_ptr(), c.dev(np.array([n], np.int32)).data_ptr(), h, w, 133, 80, m, *[float(v) for v in merge],
                                   ws.data_ptr(), pan.data_ptr(), pic.data_ptr(), out_n.data_ptr(), seg.data_ptr(), E._stream()) == 0
        table, cnt = host(seg).view(E.SEGMENT), int(host(out_n)[0])
        assert not table[cnt:].view(np.uint8).any()
        got = dict(panoptic=host(pan), rgb=host(pic), table=table[:cnt], count=cnt)
        _compare_merge(got, semmap, masks, scores, classes, merge=merge)
        assert np.array_equal(got["rgb"], E.id2rgb(got["panoptic"]))
        r["%dx%d-%d" % (h, w, n)] = dict(pan=pan, pic=pic, n=out_n, seg=seg)
    return r


# ------------------------------------------------------------------------------------------------ panoptic quality
def _pq(caps):
    """61 x 83 with 7 ground-truth and 9 predicted segments (the call's g_cap / p_cap are exactly this picture's table sizes when caps =
    (1, 1)), a picture with no predicted segment, one with no ground-truth segment, a 1 x 1 picture with neither; int32 and RGB ground
    truth.  caps = (254, 255): pa_pq_lds_bins says no and the bins are in memory."""
    def fn(c):
        from tests import painter_pq_cases as C
        from tests import painter_pq_host as H
        from tests.test_painter_pq_gpu import same, statement
        cases = [C.case(3, 61, 83, 7, 9, noise=0.05), C.case(24, 9, 7, 3, 0), C.case(25, 7, 5, 0, 2), C.case(20, 1, 1, 0, 0)]
        assert not cases[1]["pred_segments"] and not cases[2]["gt_segments"] and cases[2]["pred_segments"]
        ref, flags = memo("pq", lambda: statement(cases))
        assert flags == [0] * 4 and ref[0].sum() >= 2
        g_cap, p_cap = max(caps[0], max(len(x["gt_segments"]) for x in cases)), max(caps[1], max(len(x["pred_segments"]) for x in cases))
        r = {"lds": lib.pa_pq_lds_bins(g_cap, p_cap)}
        assert r["lds"] == int(caps == (1, 1))
        for gt in ("gt", "gt_rgb"):
            for bins in (0, 1):
                score = E.PanopticQuality(C.K, C.THINGS)
                score.bins, score.min_caps = bins, caps
                score.add(c.devs([x["pred"] for x in cases]), [x["pred_segments"] for x in cases], c.devs([x[gt] for x in cases]),
                          [x["gt_segments"] for x in cases])
                c.holds("pa_pq_add's workspace", score._last[4], lib.pa_pq_workspace_bytes(len(cases), g_cap, p_cap, C.K))
                assert score.out.numel() == 32 * C.K and score._flags[0].numel() == len(cases)
                same(score.counts(), ref)
                score.add(c.devs([cases[0]["pred"]]), [cases[0]["pred_segments"]], c.devs([cases[0][gt]]), [cases[0]["gt_segments"]])      # accumulated in place
                r["%s bins %d" % (gt, bins)], r["%s flags %d" % (gt, bins)] = score.out, score._flags
        return r
    return fn


case("pq-caps-exactly-met-lds", ["painter_engine"], ("pa_pq_add", "pa_pq_workspace_bytes"))(_pq((1, 1)))
case("pq-caps-254-255-global", ["painter_engine"], ("pa_pq_add", "pa_pq_workspace_bytes"))(_pq((254, 255)))


# ------------------------------------------------------------------------------------------------ instance mask AP
def _ap(as_bits):
    """61 x 83 (159 words, the last holds 7 pixels) with 12 detections and 7 ground truths -- the call's d_cap / g_cap exactly; 9 x 7 with
    0 detections; 9 x 7 with 0 ground truths; 1 x 1 with neither.  as_bits: both sides arrive as bit words with the padding bits of the
    last word set; otherwise as bytes, packed by pa_pack_mask_bits."""
    def fn(c):
        from tests import painter_ap_cases as C
        from tests import painter_ap_host as H
        from tests.test_painter_ap_gpu import RANGES, nothing, same, statement
        pictures = [C.case(1, 61, 83, 7, 12), C.case(33, 9, 7, 3, 0), C.case(34, 9, 7, 0, 5), nothing(1, 1)]
        ref, flags = memo("ap", lambda: statement(pictures))
        assert flags == [0] * 4 and [len(x) for x in ref] == [12, 0, 5, 0]

        def conv(m):
            h, w = m.shape[1:]
            return c.dev(_garbage_bits(m, h, w)[:len(m)]) if as_bits else c.dev(m.view(np.uint8) * np.uint8(201))
        ap = E.InstanceAP(C.K, H.MODES, area_ranges=RANGES)
        ap.add([conv(d["masks"]) for d, _ in pictures], [d["scores"] for d, _ in pictures], [d["classes"] for d, _ in pictures],
               [conv(g["masks"]) for _, g in pictures], [g["annotations"] for _, g in pictures], sizes=[d["masks"].shape[1:] for d, _ in pictures])
        n, d_cap, g_cap = shape = ap._outs[-1][2]
        assert shape == (4, 12, 7)
        total = lib.pa_ap_workspace_bytes(*shape)
        ws = ap._last[4]
        c.holds("pa_ap_add's workspace", ws, total)
        sizes = [4 * n * d_cap * g_cap, 4 * n * d_cap, 4 * n * g_cap, 4 * n * d_cap, 8 * n * 4 * d_cap]
        at = [int(lib.pa_ap_workspace_offset(*shape, which)) for which in range(5)]
        offsets_inside("pa_ap_workspace_offset%s" % (shape,), total, sorted(zip(at, sizes)))
        same(ap.records(), ref)
        a = host(ws)
        inter = a[at[0]:at[0] + sizes[0]].view(np.uint32).reshape(n, d_cap, g_cap)
        r = dict(out=ap._outs[-1][0], gpix=a[at[2]:at[2] + sizes[2]].copy())
        for i, pic in enumerate(pictures):
            want, darea, gpix = H.intersections(*pic)
            d, g = want.shape
            assert np.array_equal(inter[i, :d, :g], want), i
            assert np.array_equal(a[at[1]:at[1] + sizes[1]].view(np.uint32).reshape(n, d_cap)[i, :d], darea), i
            assert np.array_equal(r["gpix"].view(np.uint32).reshape(n, g_cap)[i, :g], gpix), i
            r["inter%d" % i] = inter[i, :d, :g].copy()
        res = ap.result()
        want = H.instance_ap(pictures, C.K, "agnostic", area_ranges=RANGES)
        assert all(res["agnostic"][key] == want[key] for key in ("AP", "AP50", "APs", "AR1", "AR100", "ARl"))
        return r
    return fn


case("instance_ap-caps-exactly-met-padding-bits-set", ["painter_engine"], ("pa_ap_add", "pa_ap_workspace_bytes", "pa_ap_workspace_offset"))(_ap(True))
case("instance_ap-caps-exactly-met-bytes", ["painter_engine"], ("pa_ap_add", "pa_ap_workspace_bytes", "pa_ap_workspace_offset", "pa_pack_mask_bits"))(_ap(False))


# ------------------------------------------------------------------------------------------------ keypoint AP
def _kpt(name):
    def fn(c):
        from tests import painter_kpt_cases as C
        from tests import painter_kpt_host as H
        from tests.test_painter_kpt_gpu import OKS_BAR, same
        if name == "one-box-no-ground-truth":
            data = memo("kpt " + name, lambda: C.dataset(19, [(1, 0), (3, 2)]))
        else:
            data = C.case(name)
        ref = data["statement"]
        ap = E.KeypointAP(data["ground_truth"], **data["settings"])
        ap.add(c.dev(data["preds"]), c.dev(data["maxvals"]), data["centers"], data["scales"], data["box_scores"], data["image_ids"], data["bbox_ids"])
        want = H.poses(data["preds"], data["maxvals"], data["centers"], data["scales"], data["box_scores"], data["settings"].get("heatmap_size", C.HEAT))
        for g, w in zip(ap.poses(), want):
            assert g.dtype == np.float32 and g.tobytes() == w.tobytes()
        assert ap._chunks[0][0].numel() == len(data["preds"]) * (3 * ap.k + 2)
        got = ap.records()
        same(got, ref)
        _, _, ws, shape, images = ap._last_eval
        n, d_cap, g_cap, max_det = shape
        total = lib.pa_kpt_workspace_bytes(*shape)
        c.holds("pa_kpt_evaluate's workspace", ws, total)
        sizes = [4 * n * d_cap, 4 * n * d_cap, 8 * n * max_det * g_cap]
        at = [int(c.lib.pa_kpt_workspace_offset(*shape, which)) for which in range(3)]
        offsets_inside("pa_kpt_workspace_offset%s" % (shape,), total, sorted(zip(at, sizes)))
        a = host(ws)
        r = dict(chunk=ap._chunks[0][0], out=ap._outs[0][0])
        for j, image in enumerate(images):                                    # only the entries of a job's own boxes and ground truths are written
            w_ = ref[image]
            d = len(w_["order"])
            order = a[at[0]:at[0] + sizes[0]].view(np.int32).reshape(n, d_cap)[j, :d]
            alive = a[at[1]:at[1] + sizes[1]].view(np.int32).reshape(n, d_cap)[j, :d]
            e, g = w_["oks"].shape
            oks = a[at[2]:at[2] + sizes[2]].view(np.float64).reshape(n, max_det, g_cap)[j, :e, :g]
            assert order.tolist() == w_["order"].tolist() and alive.tolist() == w_["alive"].astype(int).tolist(), image
            assert (np.abs(oks - w_["oks"]) <= OKS_BAR * np.abs(w_["oks"])).all(), image
            r["ws %s" % image] = dict(order=order.copy(), alive=alive.copy(), oks=oks.copy())
        if name == "second_word":
            evaluated, high, unmatched, ignored = C.second_word_facts(data, ref)
            assert evaluated == max_det == 64 == len(got[100]) and high >= 1 and d_cap == 93 and g_cap == 70       # max_det exactly met, the 33rd and later detections
        if name == "one-box-no-ground-truth":
            assert len(got[100]) == 1 and not data["ground_truth"][100] and ap.survivors[100] == 1
        return r
    return fn


for name_ in ("second_word", "one-box-no-ground-truth", "hand_made"):
    case("keypoint_ap-" + name_, ["painter_engine"], ("pa_kpt_poses", "pa_kpt_evaluate", "pa_kpt_workspace_bytes", "pa_kpt_workspace_offset"))(_kpt(name_))


@case("keypoint_ap-behind-pose-decodes", ["painter_engine"], ("pa_pose_keypoints", "pa_kpt_poses", "pa_kpt_evaluate"))
def _kpt_chain(c):
    """pa_kpt_poses reads preds and maxvals where two PoseDecodes left them (one packed buffer each) and writes one chunk in two parts."""
    from tests import painter_kpt_cases as C
    from tests.test_painter_kpt_gpu import same
    data = C.case("chain")
    decs = [E.PoseDecode(c.dev(data["pictures"][lo:hi]), c.dev(data["flipped"][lo:hi])) for lo, hi in ((0, 4), (4, 6))]
    ap = E.KeypointAP(data["ground_truth"], **data["settings"])
    ap.add_decodes(decs, data["centers"], data["scales"], data["box_scores"], data["image_ids"], data["bbox_ids"])
    same(ap.records(), data["statement"])
    return dict(chunk=ap._chunks[0][0], out=ap._outs[0][0], decodes=[d.out for d in decs])


# ------------------------------------------------------------------------------------------------ optimizer
@case("optim-1-chunk-and-one-element-past-a-chunk", ["ops", "optim"], ("pa_grad_sumsq", "pa_grad_sumsq_workspace_bytes", "pa_adamw_step"))
def _optim(c):
    """painter_amd.optim.AdamW over p / g / m / v that are views of guarded flat buffers (tests/optim_cases.guarded_views, element
    offsets 1 .. 3 mod 4), the scratch of pa_grad_sumsq at exactly pa_grad_sumsq_workspace_bytes(nchunks): one chunk (8 bytes), a count
    one past a chunk boundary, three tensors.  Held to float64 AdamW at the gates of tests/test_optim_kernels_gpu.py; no float atomics,
    so (b) is also held to the bits of (a)."""
    from painter_amd import optim as PO
    from tests import optim_cases as OC
    chunk = int(lib.pa_opt_chunk_elems())
    scale, max_norm, betas, eps = 128.0, 0.05, (0.9, 0.95), 1e-8
    r = {}
    for tag, lengths in (("1 chunk", [5]), ("chunk + 1", [chunk + 1]), ("3 tensors", [3, chunk + 1, chunk])):
        nchunks = sum(-(-n // chunk) for n in lengths)
        gen = torch.Generator().manual_seed(len(lengths) + lengths[0])
        params = [torch.randn(n, generator=gen) for n in lengths]
        grads = [[torch.randn(n, generator=gen) * 0.2 * scale for n in lengths] for _ in range(2)]
        bufs, views, guards = {}, {}, {}
        for q in "pgmv":
            bufs[q], views[q], guards[q] = OC.guarded_views(lengths, OC.ALIGN_CLASSES["all"][q], device=DEV)
        ps = []
        for i, p in enumerate(params):
            views["p"][i].copy_(p)
            views["m"][i].zero_()
            views["v"][i].zero_()
            ps.append(torch.nn.Parameter(views["p"][i]))
            assert ps[i].data_ptr() == views["p"][i].data_ptr()
        opt = PO.AdamW([{"params": ps, "lr": 1e-3, "weight_decay": 0.05}], lr=1e-3, betas=betas, eps=eps)
        for i, p in enumerate(ps):
            opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = views["m"][i], views["v"][i]
        first = len(c.ws_calls)
        for k, gk in enumerate(grads):
            for i, p in enumerate(ps):
                views["g"][i].copy_(gk[i])
                p.grad = views["g"][i]
            info = opt.grad_sumsq()
            r["%s info %d" % (tag, k)] = info.clone()
            assert float(info[1]) == 0.0
            opt.step(grad_scale=torch.tensor(scale), max_norm=max_norm)
        if c.guarded:                                                      # the scratch: exactly what the helper returned, nothing rounded
            asked = c.ws_calls[first:]
            assert len(asked) == 2 and all(n == lib.pa_grad_sumsq_workspace_bytes(nchunks) == t.numel() == 8 * nchunks for n, t in asked), asked
        got = {"p": [v.cpu() for v in views["p"]], "exp_avg": [v.cpu() for v in views["m"]], "exp_avg_sq": [v.cpu() for v in views["v"]],
               "step": [float(opt.state[p]["step"]) for p in ps]}
        ref, gates, yard = memo(("optim", tag), lambda: OC.reference_and_gates(params, [0] * len(lengths), [(1e-3, 0.05)], [dict(grads=gk) for gk in grads],
                                                                              betas=betas, eps=eps, scale=scale, max_norm=max_norm))
        OC.check_against("optim[%s]" % tag, got, ref, gates, yard)
        for q in "pgmv":                                                   # the elements between the views of a flat buffer
            assert bool((bufs[q][guards[q]] == OC.GUARD).all()), "guard elements of the %s buffer of %s were written" % (q, tag)
            r["%s %s" % (tag, q)] = bufs[q]
    return r


# ------------------------------------------------------------------------------------------------ slab reduce, dead rows, the diagnostic kernel
@case("slab_reduce-n-68-260-nz-1-3-accumulate-0-1", [], ("pa_slab_reduce",))
def _slab_reduce(c):
    """pa_slab_reduce refuses an n that is no multiple of 4 (one float4 per thread); the nearest shapes it accepts that are no multiple of
    a workgroup's 64 columns: n = 4, 68 and 260.  engine._add_ is the call with nz = 1, accumulate = 1.  The sums run in a fixed order
    (out, then slab 0, 1, 2), which fp32 on the host repeats exactly."""
    from painter_amd import engine
    from painter_amd import ops
    r = {}
    gen = torch.Generator().manual_seed(3)
    assert lib.pa_slab_reduce(256, 256, 6, 1, 8, 0, 0) == 1                  # hipErrorInvalidValue before anything is launched
    for n in (4, 68, 260):
        for nz in (1, 3):
            slabs, start = torch.randn(nz, n, generator=gen), torch.randn(n, generator=gen)
            for acc in (0, 1):
                out = c.dev(start)
                assert c.lib.pa_slab_reduce(c.dev(slabs).data_ptr(), out.data_ptr(), n, nz, n, acc, ops.stream()) == 0
                want = start.clone() if acc else torch.zeros(n)
                for z in range(nz):
                    want = want + slabs[z]
                assert torch.equal(out.cpu(), want), (n, nz, acc)
                r["%d %d %d" % (n, nz, acc)] = out
        a, b = c.dev(start), c.dev(slabs[0])
        assert engine._add_(a, b) is a and torch.equal(a.cpu(), start + slabs[0])
        r["_add_ %d" % n] = a
    return r


@case("fill_dead_rows-direct", [], ("pa_fill_dead_rows",))
def _fill_dead_rows(c):
    """No Python caller (pa_linear_dgrad_live calls it inside the library): rows of 32 of 48 bytes, the last row dead -- its 16 bytes
    of pitch behind the row do not exist."""
    from painter_amd import ops
    r = {}
    for M, rowmap in ((1, [-1]), (5, [0, -1, 1, 2, -1]), (3, [0, 1, 2])):
        pitch, row = 48, 32
        x = torch.arange(1, (M - 1) * pitch + row + 1, dtype=torch.int32).to(torch.uint8)
        d = c.dev(x)
        assert c.lib.pa_fill_dead_rows(d.data_ptr(), pitch, row, c.dev(np.array(rowmap, np.int32)).data_ptr(), M, ops.stream()) == 0
        want = x.clone()
        for i, m in enumerate(rowmap):
            if m < 0:
                want[i * pitch:i * pitch + row] = 0
        assert torch.equal(d.cpu(), want), rowmap
        r["M%d" % M] = d
    return r


@case("debug_rmw-direct", [], ("pa_debug_rmw",))
def _debug_rmw(c):
    """No Python caller in the package (tools/gradsync_overlap.py drives it): scratch = 0.5 * (scratch + src), `passes` times; one fp32
    add and an exact halving per pass, which the host repeats exactly."""
    from painter_amd import ops
    r = {}
    gen = torch.Generator().manual_seed(4)
    for n, passes, nblocks in ((4, 1, 1), (1028, 2, 3), (260, 3, 7)):
        src, scratch = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        d = c.dev(scratch)
        assert c.lib.pa_debug_rmw(c.dev(src).data_ptr(), d.data_ptr(), n, passes, nblocks, ops.stream()) == 0
        want = scratch.clone()
        for _ in range(passes):
            want = 0.5 * (src + want)
        assert torch.equal(d.cpu(), want), (n, passes, nblocks)
        r["%d %d %d" % (n, passes, nblocks)] = d
    return r


# ------------------------------------------------------------------------------------------------ the plain forms of four _skip entry points
class _PlainForms:
    """`lib` for painter_amd.ops in which pa_linear_fwd_skip, pa_linear_dgrad_skip, pa_attn_fwd_skip and pa_attn_bwd_skip are reached through
    pa_linear_fwd, pa_linear_dgrad, pa_attn_fwd and pa_attn_bwd: the same arguments without `rowskip` (which must be NULL) and, for the two
    GEMMs, without `skip_rows_per_sample`.  No Python module calls the plain forms; this is how their case reaches them with the buffers
    ops.py allocates."""
    DROP = {"pa_linear_fwd_skip": 2, "pa_linear_dgrad_skip": 2, "pa_attn_fwd_skip": 1, "pa_attn_bwd_skip": 1}      # arguments in front of `stream`

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name not in self.DROP:
            return getattr(self._real, name)
        plain, drop = getattr(self._real, name[:-len("_skip")]), self.DROP[name]

        def call(*a):
            assert a[-1 - drop] == 0, "%s was asked to skip rows" % name
            return plain(*a[:-1 - drop], a[-1])
        return call


@case("plain-forms-of-linear_fwd-linear_dgrad-attn_fwd-attn_bwd", ["ops"], ("pa_linear_fwd", "pa_linear_dgrad", "pa_attn_fwd", "pa_attn_bwd"))
def _plain_forms(c):
    """Each result through the plain entry point equals, bit for bit, what painter_amd.ops computes through the _skip form (held to fp64
    by tests/test_kernels_gpu.py and guarded by tests/test_guard_bands_gpu.py)."""
    from painter_amd import ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_GELU
    BF, F32 = torch.bfloat16, torch.float32

    def gen(shape, seed, scale=1.0, dtype=F32):
        return c.dev((torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype))

    def both(fn):
        """fn() through the _skip forms, then through the plain ones -> the plain results, asserted equal"""
        want = fn()
        base = ops.lib
        ops.lib = _PlainForms(base)
        try:
            got = fn()
        finally:
            ops.lib = base
        same_bytes("plain form against the _skip form", want, got)
        return got
    r = {}
    for T in (BF, F32):
        tag = "bf16" if T == BF else "fp32"
        for M, N, K in ((96, 64, 72), (328, 264, 256)):                      # the generic engine; bf16: the 256 x 256 kernel with ragged tiles
            x, w, b = gen((M, K), 1, 1.0, T), gen((N, K), 2, 0.05, T), gen((N,), 3)
            dy = gen((M, N), 6, 1.0, T)

            def linear():
                act, aux = ops.linear_gelu(x, w, b)
                cs = c.buf((K,), F32)
                return dict(bias=ops.linear_fwd(x, w, b, EPI_BIAS), f32=ops.linear_fwd(x, w, b, EPI_BIAS_F32), act=act, aux=aux,
                            dx=ops.linear_dgrad(dy, w), dx_gelu=ops.linear_dgrad(gen((M, K), 7, 1.0, T), gen((K, N), 8, 0.05, T), gelu_aux=aux),
                            dx_cs=ops.linear_dgrad(dy, w, colsum_out=cs), cs=cs)
            r["linear %s %dx%dx%d" % (tag, M, N, K)] = both(linear)
        for B, H, Hp, Wp, hd in ((1, 2, 8, 4, 64),) + (((1, 1, 8, 28, 64),) if T == BF else ()):      # generic; bf16: generation 3 with tables
            L, scale = Hp * Wp, hd ** -0.5
            qkv, dout = gen((B * L, 3 * H * hd), 1, 1.0, T), gen((B * L, H * hd), 4, 1.0, T)
            rel_h, rel_w = gen((2 * Hp - 1, hd), 2, 0.2), gen((2 * Wp - 1, hd), 3, 0.2)
            rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T)

            def attn():
                out, lse, tables = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale, need_tables=True)
                dqkv, dG = ops.attn_bwd_core(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale, tables=tables)
                return dict(out=out, lse=lse, dqkv=dqkv, drcat=ops.attn_bwd_relpos(dG, qkv, rcat.shape[0], B, L, H, Hp, Wp))
            r["attn %s %dx%dx%dx%d" % (tag, B, H, Hp, Wp)] = both(attn)
    return r


# ------------------------------------------------------------------------------------------------ completeness
# C entry points that enqueue nothing, or that another test already holds between guards
_SIZE = "host only: a size / offset helper; the case of its kernel allocates exactly what it returns"
EXCLUDED = {
    "pa_abi_version": "host only: the ABI version number",
    "pa_debug_set": "host only: sets a knob of the library (pa_debug_*)",
    "pa_debug_get": "host only: reads a knob of the library (pa_debug_*)",
    "pa_attn_set_generation": "host only: selects the attention kernel family",
    "pa_attn_trace": "host only: reads the attention launch counters",
    "pa_opt_chunk_elems": "host only: the chunk size of the optimizer tables (the optim case sizes its tensors by it)",
    "pa_semseg_lds_bins": "host only: which bin route pa_semseg_confusion takes (the semseg cases assert both answers)",
    "pa_pq_lds_bins": "host only: which bin route pa_pq_add takes (the pq cases assert both answers)",
    "pa_decoder_live_ok": "host only: whether the live-row kernels take a decoder shape",
    "pa_live_rows_max": "host only: the largest B * L pa_live_rows takes",
    "pa_semseg_boundary_workspace_bytes": _SIZE + " (tests/test_painter_boundary_gpu.py::test_guard_bands_of_both_entry_points)",
    "pa_semseg_boundary_confusion": "guarded by tests/test_painter_boundary_gpu.py::test_guard_bands_of_both_entry_points",
    "pa_label_boundary": "guarded by tests/test_painter_boundary_gpu.py::test_guard_bands_of_both_entry_points",
}


def _ops_symbols():
    """(i): the symbols painter_amd/ops.py references; tests/test_guard_bands_gpu.py holds every function of that module to a case."""
    import re
    return set(re.findall(r"\blib\.(pa_\w+)", open(os.path.join(ROOT, "painter_amd", "ops.py")).read()))


def _claimed():
    out = set()
    for p in CASES:
        out |= set(p.values[2])
    return out


def test_every_abi_symbol_is_guarded_or_excluded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_hip.h")).read())
    from_ops, claimed = _ops_symbols(), _claimed()
    assert len(abi) >= 134 and from_ops <= abi and claimed <= abi and set(EXCLUDED) <= abi, (from_ops - abi, claimed - abi, set(EXCLUDED) - abi)
    assert not (claimed & set(EXCLUDED)), claimed & set(EXCLUDED)
    for name, why in EXCLUDED.items():                                     # an exclusion is a helper, a knob, or names the test that guards it
        assert why.startswith("host only") or "::" in why, (name, why)
    unplaced = abi - from_ops - claimed - set(EXCLUDED)
    assert not unplaced, "entry points of include/painter_hip.h without a guard-band case or a stated exclusion: %s" % sorted(unplaced)
    helpers = {s for s in abi if s.endswith(("_workspace_bytes", "_workspace_offset"))}
    assert helpers <= from_ops | claimed | set(EXCLUDED)
