"""Host restatement of the pixel work of Painter's eight task-inference scripts (Painter/eval/*/painter_inference_*.py) and of the
colour -> class decode of ADE20kSemSegEvaluatorCustom.py: what tests/test_painter_eval_gpu.py compares the device path with.
TEST INFRASTRUCTURE -- pure numpy (+ CPU torch for the evaluator's float32 expression), deterministic on any machine.

What pins it (tests/test_painter_eval_cpu.py):
  * `bilinear` / `nearest` / `channel_mean` against live CPU torch `F.interpolate` / `.mean(-1)`, bit for bit; `bicubic` within the
    documented gate (torch's own operation order for bicubic is not reproduced);
  * every digest of tests/golden/painter_eval_io.npz, which the UNMODIFIED scripts' `run_one_image` functions and
    `util/ddp_utils.DatasetTest` produced (tests/golden/make_golden_painter_eval_io.py);
  * the scripts' MAIN BODIES need CUDA, DDP and the datasets and cannot run in a test: their prompt / canvas lines (`resize`,
    `/ 255.`, `np.concatenate`, `- mean`, `/ std`) are restated in `canvases` and pinned against Pillow and numpy themselves.

`F.interpolate` is NOT called here: the bilinear resize is restated with an exactly emulated fused multiply-add, because the values
the scripts write are trunc() of float64 numbers that sit exactly on 0 / 255 / 10000 over saturated regions, where one ulp flips a byte.
"""
import numpy as np
import torch
from PIL import Image

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])

# The eight scripts' settings as the scripts state them: (script path under Painter/eval, resize mode, scale, clip, output kind).
SCRIPTS = {
    "ade20k_semseg": ("ade20k_semantic/painter_inference_segm.py", "bilinear", 255.0, True, "u8"),
    "coco_pano_semseg": ("coco_panoptic/painter_inference_pano_semseg.py", "bilinear", 255.0, True, "u8"),
    "coco_pano_inst": ("coco_panoptic/painter_inference_pano_inst.py", "nearest", 255.0, True, "u8"),
    "coco_pose": ("mmpose_custom/painter_inference_pose.py", "nearest", 255.0, True, "u8"),
    "nyuv2_depth": ("nyuv2_depth/painter_inference_depth.py", "bilinear", 10000.0, True, "depth"),
    "derain": ("derain/painter_inference_derain.py", "bicubic", 1.0, False, "f64"),
    "lol": ("lol/painter_inference_lol.py", "bicubic", 1.0, False, "f64"),
    "sidd": ("sidd/painter_inference_sidd.py", "bicubic", 1.0, False, "f64"),
}


# ---- exact fused multiply-add in float64 (numpy has none): error-free product and sum, the two error terms added with rounding to
# odd so that the final addition rounds the exact a * b + c once (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums").
def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _add_round_to_odd(a, b):
    u, v = _two_sum(a, b)
    u = np.ascontiguousarray(u, dtype=np.float64)
    bits = u.view(np.int64).copy()
    fix = (v != 0.0) & ((bits & 1) == 0)
    away = (v > 0.0) == (u > 0.0)                     # the discarded part points away from zero: magnitude + 1 ulp, else - 1 ulp
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p, e = _two_prod(a, b)
    s, t = _two_sum(p, c)
    return s + _add_round_to_odd(t, e)


# ---- F.interpolate on the float64 [H][W][3] picture the scripts pass (channels-last view of NCHW, size = [h, w])
def _linear_axis(n_in, n_out):
    scale = n_in / n_out
    d = np.arange(n_out, dtype=np.float64)
    p = np.maximum(fma(np.full(n_out, scale), d + 0.5, np.full(n_out, -0.5)), 0.0)
    i0 = np.minimum(np.floor(p).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = p - i0
    return i0, i1, 1.0 - lam, lam


def bilinear(pic, out_h, out_w):
    """mode='bilinear', align_corners=False: width first for the two source rows, then height; one fma per combination."""
    y0, y1, wy0, wy1 = _linear_axis(pic.shape[0], out_h)
    x0, x1, wx0, wx1 = _linear_axis(pic.shape[1], out_w)
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    top, bot = pic[y0], pic[y1]
    r0 = fma(wx0, top[:, x0], wx1 * top[:, x1])
    r1 = fma(wx0, bot[:, x0], wx1 * bot[:, x1])
    return fma(wy0[:, None, None], r0, wy1[:, None, None] * r1)


def nearest_index(n_in, n_out):
    """mode='nearest': scale * dst in double, narrowed to float32, floored, clamped."""
    scale = float(n_in) / float(n_out)
    src = np.floor((scale * np.arange(n_out, dtype=np.float64)).astype(np.float32))
    return np.minimum(src.astype(np.int64), n_in - 1)


def nearest(pic, out_h, out_w):
    return pic[nearest_index(pic.shape[0], out_h)][:, nearest_index(pic.shape[1], out_w)]


def _cubic_axis(n_in, n_out):
    a = -0.75
    scale = n_in / n_out
    p = scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    f = np.floor(p)
    t = p - f

    def c1(x):
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0

    def c2(x):
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a

    u = 1.0 - t
    w = np.stack([c2(t + 1.0), c1(t), c1(u), c2(u + 1.0)])
    idx = np.clip(f.astype(np.int64)[None, :] + np.arange(-1, 3)[:, None], 0, n_in - 1)
    return idx, w


def bicubic(pic, out_h, out_w):
    """mode='bicubic' (A = -0.75, align_corners=False, border indices clamped): weights, then sum over x inside sum over y."""
    iy, wy = _cubic_axis(pic.shape[0], out_h)
    ix, wx = _cubic_axis(pic.shape[1], out_w)
    acc = np.zeros((out_h, out_w, pic.shape[2]), np.float64)
    for j in range(4):
        rows = pic[iy[j]]
        rowv = np.zeros_like(acc)
        for k in range(4):
            rowv = rowv + rows[:, ix[k]] * wx[k][None, :, None]
        acc = acc + rowv * wy[j][:, None, None]
    return acc


def channel_mean(pic):
    """torch `.mean(-1)` over three float64 channels."""
    return ((pic[..., 0] + pic[..., 1]) + pic[..., 2]) / 3.0


# ---- the scripts' lines
def pil_resize(pic, res):
    """`Image.resize((res, res))` of an RGB picture: Pillow itself (BICUBIC is its default for RGB)."""
    return np.array(Image.fromarray(pic).resize((res, res)))


def canvases(prompt, prompt_tgt, query, res=448, query_is_resized=False):
    """painter_inference_segm.py:133-162 (the same lines in every script): uint8 RGB pictures of any size -> the two normalised float64
    canvases [2*res][res][3] the script hands to run_one_image."""
    prompt01, target01 = pil_resize(prompt, res) / 255., pil_resize(prompt_tgt, res) / 255.
    query01 = (query if query_is_resized else pil_resize(query, res)) / 255.

    def normalised(top, bottom):                      # one rounding per operation: subtract, then divide
        canvas = np.concatenate((top, bottom), axis=0)
        canvas = canvas - MEAN
        return canvas / STD

    return normalised(prompt01, query01), normalised(target01, target01)      # "tgt is not available": the prompt's target twice


def model_inputs(img, tgt):
    """run_one_image's tensors: float32 NCHW [1][3][2*res][res]."""
    x = np.ascontiguousarray(img.astype(np.float32).transpose(2, 0, 1)[None])
    t = np.ascontiguousarray(tgt.astype(np.float32).transpose(2, 0, 1)[None])
    return x, t


def lower_half(tokens, res_h, res_w, patch):
    """unpatchify + einsum('nchw->nhwc') + `y[0, y.shape[1]//2:]` for ONE sample's float32 tokens [L][p*p*3] -> float32 [res_h][res_w][3]."""
    hp, wp = 2 * res_h // patch, res_w // patch
    y = np.asarray(tokens, np.float32).reshape(hp, wp, patch, patch, 3).transpose(0, 2, 1, 3, 4).reshape(hp * patch, wp * patch, 3)
    return y[res_h:]


def decode(task, tokens, size, res_h=448, res_w=448, patch=16):
    """The lines after the model call (e.g. painter_inference_segm.py:88-92) for one sample's tokens; size = (width, height) as the
    scripts pass it.  -> uint8 [H][W][3] / int32 [H][W] / float64 [H][W][3]."""
    _, mode, scale, clip, kind = SCRIPTS[task]
    out = lower_half(tokens, res_h, res_w, patch).astype(np.float64) * STD + MEAN
    if clip:
        out = np.clip(out * scale, 0, scale)
    resize = {"bilinear": bilinear, "nearest": nearest, "bicubic": bicubic}[mode]
    out = resize(out, size[1], size[0])
    if kind == "u8":
        return out.astype(np.int32).astype(np.uint8)
    if kind == "depth":
        return channel_mean(out).astype(np.int32)
    return out


def saved_picture(restored):
    """painter_inference_derain.py:157-162: what the restoration scripts save."""
    return (np.clip(restored, 0, 1) * 255).astype(np.uint8)


def class_map(picture, palette, dist_type="abs"):
    """The colour -> class decode of ADE20kSemSegEvaluatorCustom.post_process_segm_output (:114-141) with CPU torch in float32: per
    pixel and palette colour the per-channel distance (abs, square, or their mean), summed over the channels; argmin over colours."""
    pix = torch.from_numpy(np.ascontiguousarray(picture)).to(torch.float32)
    pal = torch.as_tensor(np.asarray(palette), dtype=torch.float32)
    per_channel = {"abs": lambda d: d.abs(), "square": lambda d: d.pow(2), "mean": lambda d: (d.abs() + d.pow(2)) / 2.}
    if dist_type not in per_channel:
        raise NotImplementedError(dist_type)
    rows = max(1, (1 << 22) // (pix.shape[1] * pal.shape[0]))         # chunked: the [H][W][K][3] tensor of a whole picture is GBs
    out = np.empty(pix.shape[:2], np.int32)
    for r in range(0, pix.shape[0], rows):
        diff = pix[r:r + rows, :, None, :] - pal[None, None, :, :]
        out[r:r + rows] = per_channel[dist_type](diff).sum(-1).argmin(-1).numpy()
    return out
