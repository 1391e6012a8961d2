"""Shared inputs for the Painter task-inference tests: seeded synthetic pictures, the output-size list, test tokens and a stand-in for
the network.  TEST INFRASTRUCTURE."""
import hashlib
import types

import numpy as np
import torch

from tests.seggpt_io_cases import patchify, picture          # noqa: F401  (the same seeded pictures as the SegGPT I/O tests)

RES, PATCH = 448, 16                       # --input_size default of every script; the model's patch size
L = (2 * RES // PATCH) * (RES // PATCH)
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])

# output sizes (height, width): the picture sizes of the evaluation sets (480 x 640 NYUv2 / COCO, 512 x 683 ADE20K, 256 x 256 SIDD, ...),
# up- and down-scaling on either axis, odd sizes, one pixel
SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (512, 683), (256, 256), (1080, 1920), (333, 517), (96, 1000), (768, 1024),
         (449, 447), (224, 224), (1, 1)]


def special_regions(c):
    """Overwrite three bands of the LOWER half of a canvas [..., 3, 2*RES, RES] (float32, normalised scale) with the values that
    decide a byte: a band that de-normalises to (almost) exactly k / 255 for every k -- float32 rounding leaves it a hair above or
    below the integer, so trunc() depends on every float64 operation -- a band far above 1 (saturates at 255 / 10000) and a band
    far below 0."""
    k = (torch.arange(RES) % 256).double()
    for ch in range(3):
        c[..., ch, RES + 32:RES + 64, :] = ((k / 255.0 - MEAN[ch]) / STD[ch]).float()
    c[..., RES + 64:RES + 96, :RES // 2] = 40.0
    c[..., RES + 64:RES + 96, RES // 2:] = -40.0
    return c


def tokens(seed, n=1, gain=6.0):
    """Random float32 tokens [n][L][768] (~70 % of the de-normalised values saturate at gain 6) with the special bands."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, 3, 2 * RES, RES, generator=g) * gain
    return patchify(special_regions(c)).numpy()


def standin_tokens(imgs, tgts):
    """What the stand-in network returns for (imgs, tgts) float32 [N][3][2*RES][RES] CPU tensors: a fixed float32 function of BOTH
    canvases, sample by sample (a batch equals its samples run one by one), with enough gain that the de-normalised picture
    saturates on both sides, plus the special bands.  CPU torch only (the GPU tests move tensors to the host for this call)."""
    assert imgs.device.type == "cpu" and imgs.dtype == torch.float32
    c = imgs * 0.6
    c = c + tgts * 0.4
    c = c + imgs.flip(2) * 0.5
    c = c + tgts.flip(3) * 0.25
    g = torch.Generator().manual_seed(4321)
    c = c + 0.05 * torch.randn(c.shape[1:], generator=g)
    return patchify(special_regions(c))


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


class StandInModel:
    """Duck-types what the scripts' run_one_image touches on the model (painter_inference_segm.py:76-85): patch_size,
    patch_embed.num_patches, __call__, unpatchify -- and records, per sample, what it was handed."""
    patch_size = PATCH
    training = False

    def __init__(self):
        self.patch_embed = types.SimpleNamespace(num_patches=L)
        self.calls = []

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __call__(self, x, tgt, bool_masked_pos, valid):
        xc, tc = x.detach().float().cpu(), tgt.detach().float().cpu()
        for i in range(xc.shape[0]):
            self.calls.append(dict(batch=xc.shape[0], x=digest(xc[i:i + 1].numpy()), tgt=digest(tc[i:i + 1].numpy()),
                                   masked=int(bool_masked_pos.sum()), mask_shape=tuple(bool_masked_pos.shape),
                                   second_half=bool((bool_masked_pos[0, L // 2:] == 1).all()),
                                   valid_ok=bool((valid == 1).all()) and tuple(valid.shape) == tuple(tgt.shape)))
        return None, standin_tokens(xc, tc).to(x.device), bool_masked_pos

    def unpatchify(self, x):
        """Tokens [N][L][p*p*3] -> canvas [N][3][2*RES][RES]: the inverse of seggpt_io_cases.patchify."""
        n = x.shape[0]
        grid = x.reshape(n, 2 * RES // PATCH, RES // PATCH, PATCH, PATCH, 3)
        return grid.permute(0, 5, 1, 3, 2, 4).reshape(n, 3, 2 * RES, RES)


class Wrapped:
    """What DistributedDataParallel looks like to the scripts that call `model.module.*`."""

    def __init__(self, module):
        self.module = module

    def __call__(self, *a, **k):
        return self.module(*a, **k)


# ---- the fixture's cases: per task the prompt pair and the queries as (seed, height, width); every task sees 480 x 640 and one
# picture larger than the 448 x 448 canvas on at least one axis (a down-scale for the prompt side) / smaller (a down-scale after it)
PROMPT = (51, 300, 400)
QUERIES = {
    "ade20k_semseg": [(61, 480, 640), (62, 200, 300)],
    "coco_pano_semseg": [(63, 480, 640), (64, 333, 517)],
    "coco_pano_inst": [(65, 480, 640), (66, 200, 300)],
    "coco_pose": [(67, 480, 640), (68, 256, 192)],
    "nyuv2_depth": [(69, 480, 640), (70, 200, 300)],
    "derain": [(71, 480, 640), (72, 321, 481)],
    "lol": [(73, 480, 640), (74, 400, 600)],
    "sidd": [(75, 448, 448)],              # SIDD hands over an already resized 448 x 448 query and asks for 256 x 256 back
}
SAMPLE_STRIDE = 11                         # float64 outputs are stored as [::11, ::11] samples


def out_size(task, h, w):
    """(width, height) the script passes as `size`."""
    return (256, 256) if task == "sidd" else (w, h)


def prompt_pair():
    s, h, w = PROMPT
    return picture(s, h, w), picture(s + 100, h, w, flat=True)


def query_pictures(task):
    return [picture(s, h, w) for (s, h, w) in QUERIES[task]]
