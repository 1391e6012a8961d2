"""Host statement of restoration scoring (csrc/painter_restore.hip): the definition the device path is held to.  TEST INFRASTRUCTURE.

Plain numpy / scipy.  skimage and MATLAB are not available where this project is tested, so both metrics are restated from published
sources and are unverified against skimage / MATLAB; the one piece of the reference that runs here, `myPSNR` of
Painter/eval/lol/painter_inference_lol.py:73-77, pins the PSNR of the first metric (tests/golden/painter_restore.npz).

  metric "skimage"    what painter_inference_lol.py:166-169 computes per picture: prediction float64 [H][W][3] clipped to [0, 1], ground
                      truth uint8 [H][W][3] taken as gt / 255. in float64.  PSNR = 10 log10(1 / mean((p - g)^2)) over all 3 H W elements
                      (`peak_signal_noise_ratio` with data range 1: the clipped prediction is >= 0, so skimage takes the range (0, 1)).
                      SSIM = `structural_similarity(multichannel=True)` with its defaults: per channel a 7 x 7 uniform window, K1 = 0.01,
                      K2 = 0.03, sample covariance (cov_norm = 49 / 48), S averaged over the map cropped by 3 pixels (full windows only),
                      then the mean of the three channel means.  `data_range` defaults to 2.0: skimage takes it from the float dtype's
                      range (-1, 1) when none is passed, and that is the release whose call signature (`multichannel=`) the reference
                      uses -- so C1 = 0.02^2 and C2 = 0.06^2, not the 0.01^2 / 0.03^2 of a [0, 1] picture.  Pass data_range=1.0 for those.
  metric "matlab_y"   Painter/eval/derain/evaluate_PSNR_SSIM.m on two uint8 [H][W][3] pictures (the prediction is the `saved` picture
                      uint8(clip * 255) of run_restoration).  Y = 16 + floor((65481 R + 128553 G + 24966 B + 127500) / 255000): the
                      65.481 / 128.553 / 24.966 row of rgb2ycbcr scaled by 1000, rounded half up, in exact integers.  194 of the 2^24
                      colours tie exactly at one half (tests/test_painter_restore_cpu.py counts them) and naive double evaluations of the
                      row round a few dozen colours the other way; what MATLAB's rgb2ycbcr does on those colours is NOT KNOWN here.
                      PSNR = 20 log10(255 / sqrt(mean(dY^2))), the squared sum an exact integer.  SSIM = SSIM_index (:81-202) on the two
                      Y planes in float64: 11 x 11 Gaussian, sigma 1.5, normalised; 'valid' windows; C1 = 2.55^2, C2 = 7.65^2; plain
                      covariance; mean of the map.

Every window moment is computed two ways (`route`): "scipy" -- `uniform_filter` / `correlate` with the 2-D window, cropped to the valid
part -- and "direct" -- a separable weighted sum over the valid windows, the order the device uses.  Their disagreement is the summation
noise of the definition itself (<= 5e-14 for the uniform window at L = 2, <= 2.7e-13 for the Gaussian at L = 255 on 7 x 7 .. 97 x 131
pictures, near-constant ones included).

A picture with H or W below the window is a ValueError (not MATLAB's -Inf).  A perfect prediction gives psnr = inf and ssim = 1.0 exactly:
with x == y the numerator and the denominator of S are the same operations on the same numbers.

`eval_sidd.m` uses MATLAB's built-in ssim / psnr on single 256 x 256 x 3 blocks; their source is not published, so it is not restated."""
import math

import numpy as np
from scipy import ndimage

METRICS = ("skimage", "matlab_y")
OUT = 8                                    # count, squared sum, then (sum of S, windows) per channel -- the device's record


def y_channel(rgb):
    """uint8 [..][3] -> int64 [..]: the Y of rgb2ycbcr, rounded half up, in exact integers."""
    c = np.asarray(rgb).astype(np.int64)
    return 16 + (65481 * c[..., 0] + 128553 * c[..., 1] + 24966 * c[..., 2] + 127500) // 255000


def weights(metric):
    """The 1-D window (both windows are separable) -> float64 [win]."""
    if metric == "skimage":
        return np.full(7, 1.0 / 7.0)
    k = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def constants(metric, data_range=None):
    """-> (cov_norm, C1, C2)."""
    if metric == "skimage":
        r = 2.0 if data_range is None else float(data_range)
        return 49.0 / 48.0, (0.01 * r) ** 2, (0.03 * r) ** 2
    r = 255.0 if data_range is None else float(data_range)
    return 1.0, (0.01 * r) ** 2, (0.03 * r) ** 2


def planes(pred, gt, metric):
    """-> list of (x, y) float64 plane pairs, one per channel, and the squared sum of x - y over all of them (an exact int for matlab_y,
    else the exactly rounded float64 sum)."""
    assert metric in METRICS, metric
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape or pred.ndim != 3 or pred.shape[2] != 3:
        raise ValueError("restoration scores: prediction %s, ground truth %s" % (pred.shape, gt.shape))
    assert gt.dtype == np.uint8, gt.dtype
    if metric == "skimage":
        assert pred.dtype == np.float64, pred.dtype
        p, g = np.clip(pred, 0, 1), gt / 255.
        d = p - g
        return [(p[..., c], g[..., c]) for c in range(3)], math.fsum((d * d).ravel().tolist())
    assert pred.dtype == np.uint8, pred.dtype
    yp, yg = y_channel(pred), y_channel(gt)
    d = yp - yg
    return [(yp.astype(np.float64), yg.astype(np.float64))], int((d * d).sum())


def moments(x, y, w, route):
    """The five window moments (x, y, x^2, y^2, x y) over the valid windows -> five float64 [H - win + 1][W - win + 1]."""
    win = len(w)
    h, wd = x.shape
    if h < win or wd < win:
        raise ValueError("restoration scores: a %d x %d picture is smaller than the %d x %d window" % (h, wd, win, win))
    pad = win // 2
    fields = (x, y, x * x, y * y, x * y)
    if route == "scipy":
        if np.all(w == w[0]):
            return [ndimage.uniform_filter(f, size=win)[pad:h - pad, pad:wd - pad] for f in fields]
        w2 = np.outer(w, w)
        w2 = w2 / w2.sum()
        return [ndimage.correlate(f, w2)[pad:h - pad, pad:wd - pad] for f in fields]
    assert route == "direct", route
    nh, nw = h - win + 1, wd - win + 1
    out = []
    for f in fields:
        rows = sum(w[k] * f[:, k:k + nw] for k in range(win))
        out.append(sum(w[k] * rows[k:k + nh] for k in range(win)))
    return out


def ssim_map(x, y, w, cov_norm, c1, c2, route="direct"):
    """S of every valid window of one plane pair."""
    ux, uy, uxx, uyy, uxy = moments(x, y, w, route)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    return ((2 * (ux * uy) + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def sums(pred, gt, metric, data_range=None, route="direct"):
    """-> float64 [8], the device's record: element count, squared sum, then per channel the exactly rounded sum of S (math.fsum) and the
    window count; channels a metric does not have hold zeros."""
    pairs, ssd = planes(pred, gt, metric)
    w = weights(metric)
    cov_norm, c1, c2 = constants(metric, data_range)
    out = np.zeros(OUT)
    out[0], out[1] = len(pairs) * pairs[0][0].size, float(ssd)
    for c, (x, y) in enumerate(pairs):
        s = ssim_map(x, y, w, cov_norm, c1, c2, route)
        out[2 + 2 * c], out[3 + 2 * c] = math.fsum(s.ravel().tolist()), s.size
    return out


def metrics(record, metric):
    """float64 [..][8] -> (psnr, ssim) float64 [..]."""
    s = np.asarray(record, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = s[..., 1] / s[..., 0]
        psnr = 10 * np.log10(1 / mse) if metric == "skimage" else 20 * np.log10(255 / np.sqrt(mse))
        ch = 3 if metric == "skimage" else 1
        ssim = sum(s[..., 2 + 2 * c] / s[..., 3 + 2 * c] for c in range(ch)) / ch
    return psnr, ssim


def scores(pred, gt, metric, data_range=None, route="direct"):
    """One picture -> (psnr, ssim) as Python floats."""
    p, s = metrics(sums(pred, gt, metric, data_range, route), metric)
    return float(p), float(s)


def saved_picture(pred):
    """What the restoration scripts save: uint8(clip(pred, 0, 1) * 255)."""
    return (np.clip(pred, 0, 1) * 255).astype(np.uint8)


def torch_route(preds, gts, metric, data_range=None):
    """The same op sequence with torch float64 convolutions on the device of `preds` (lists of tensors: float64 / uint8 [H][W][3]
    predictions, uint8 ground truths) -> list of (psnr, ssim) 0-d tensors on that device.  For tools/painter_restore_bench.py."""
    import torch
    import torch.nn.functional as F
    w = torch.from_numpy(weights(metric))
    cov_norm, c1, c2 = constants(metric, data_range)
    out = []
    for p, g in zip(preds, gts):
        w = w.to(p.device)
        if metric == "skimage":
            x, y = p.clamp(0, 1).permute(2, 0, 1), g.to(torch.float64).permute(2, 0, 1) / 255.
            d = x - y
            psnr = 10 * torch.log10(1 / (d * d).mean())
        else:
            def luma(t):
                t = t.to(torch.int64)
                return (16 + torch.div(65481 * t[..., 0] + 128553 * t[..., 1] + 24966 * t[..., 2] + 127500, 255000,
                                       rounding_mode="floor")).to(torch.float64)[None]
            x, y = luma(p), luma(g)
            d = x - y
            psnr = 20 * torch.log10(255 / torch.sqrt((d * d).mean()))
        f = torch.stack([x, y, x * x, y * y, x * y], 1)                          # [C][5][H][W]
        f = F.conv2d(f.reshape(-1, 1, *f.shape[2:]), w.view(1, 1, 1, -1))
        f = F.conv2d(f, w.view(1, 1, -1, 1))
        f = f.reshape(x.shape[0], 5, *f.shape[2:])
        ux, uy, uxx, uyy, uxy = f.unbind(1)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * (ux * uy) + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        out.append((psnr, s.mean((1, 2)).mean()))
    return out
