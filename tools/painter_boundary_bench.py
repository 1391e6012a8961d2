"""Measure the boundary-IoU branch of the semantic scorers on two batches of eight pictures: 512 x 683 ADE20K pictures (K = 150, d = 17)
and 480 x 640 COCO pictures (K = 133, d = 16), in one process, legs alternated.

    python tools/painter_boundary_bench.py [--rounds 5 --iters 3 --batch 8] -> lines per round, then ONE JSON line

Before anything is timed both device matrices are compared with the host statement (tests/painter_boundary_host.py, equal), the plain
matrix with `SemsegScore`'s (equal bytes), and the two baseline routes' boundary matrices with the device's.  Legs, milliseconds per
BATCH from HIP events around `iters` back-to-back runs, median and range over the rounds; pictures and label maps are device-resident, as
they are behind the decode, except where a route says otherwise:
    boundary_add   `SemsegBoundaryScore.add` of the batch: three launches, nothing copied back
    score_add      `SemsegScore.add` of the same batch: boundary_add - score_add is what the branch costs
    torch_route    the evaluator's op sequence per picture with torch on the same GPU: upload, the float32 [H][W][K][3] tensor and its
                   arg-min, the zero ring, d times `-max_pool2d(-x, 3, 1, 1)` (its padding never wins, as cv2.erode's border) on both maps,
                   two bincounts on the device, both matrices copied back -- the class map stays on the device, which the evaluator's does not
    host_route     `class_map` per picture (the int32 map's copy back), then on the host scipy's minimum filter of (2d + 1)^2 with
                   everything outside read as 0 on both maps -- ONE separable filter instead of cv2's d iterations, cv2 not being
                   available: a floor for the host route -- and two np.bincount
and per leg the bytes copied back per batch and the peak of torch's allocator."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E       # noqa: E402
from tests import painter_boundary_host as B      # noqa: E402
from tests import painter_score_cases as C        # noqa: E402
from tools.painter_inst_bench import peak_mb          # noqa: E402
from tools.painter_score_bench import run_legs        # noqa: E402


def torch_route(picture, gt, palette, d, ignore_label=255):
    """-> (conf, bconf) int64 numpy [K + 1][K + 1] of one picture; picture uint8 numpy, gt uint8 CUDA tensor, palette float32 CUDA [K][3]."""
    import torch.nn.functional as F
    segm = torch.from_numpy(picture).float().to(palette.device)
    h, w, k = segm.shape[0], segm.shape[1], palette.shape[0]
    pred = torch.sum(torch.abs(segm.view(h, w, 1, 3) - palette.view(1, 1, k, 3)), dim=-1).argmin(dim=-1)
    gtk = gt.long()
    gtk[gtk == ignore_label] = k

    def boundary(m):
        x = F.pad(m.float().view(1, 1, h, w), (1, 1, 1, 1))
        for _ in range(d):
            x = -F.max_pool2d(-x, 3, 1, 1)
        return m - x[0, 0, 1:-1, 1:-1].long()

    conf = torch.bincount(((k + 1) * pred + gtk).view(-1), minlength=(k + 1) ** 2)
    bconf = torch.bincount(((k + 1) * boundary(pred) + boundary(gtk)).view(-1), minlength=(k + 1) ** 2)
    return conf.cpu().numpy().reshape(k + 1, k + 1), bconf.cpu().numpy().reshape(k + 1, k + 1)


def host_route(picture, gt, palette, d, ignore_label=255):
    """-> (conf, bconf); picture uint8 CUDA tensor, gt uint8 numpy."""
    from scipy import ndimage
    k = len(palette)
    pred = E.class_map(picture, palette).astype(np.uint8)
    gtk = np.where(gt == ignore_label, k, gt).astype(np.uint8)
    bp, bg = (m - ndimage.minimum_filter(m, size=2 * d + 1, mode="constant", cval=0) for m in (pred, gtk))
    count = lambda a, b: np.bincount((k + 1) * a.reshape(-1).astype(np.int64) + b.reshape(-1).astype(np.int64), minlength=(k + 1) ** 2)
    return count(pred, gtk).reshape(k + 1, k + 1), count(bp, bg).reshape(k + 1, k + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_boundary_bench: needs the MI355X (nothing here is measured on a CPU)")
    summary = {"what": "semantic confusion matrix with the boundary-IoU branch, batch %d" % a.batch, "device": torch.cuda.get_device_name(0),
               "rounds": a.rounds, "iters": a.iters, "unit": "ms per batch", "check": {}, "legs": {}, "copied_back_bytes_per_batch": {},
               "memory": {}}
    settings = {"ade_512x683": ("ade", 512, 683), "coco_480x640": ("coco", 480, 640)}
    for tag, (which, h, w) in settings.items():
        # two distinct pictures per setting, repeated through the batch (the host statement runs on CPU torch: seconds per picture)
        pairs = [C.semseg_case(which, 40 + i, h, w)[:2] for i in range(2)]
        pal = np.array(C.ade_palette() if which == "ade" else C.coco_palette(), np.float32)
        k, d, dpal = len(pal), E.boundary_dilation(h, w), torch.from_numpy(pal).cuda()
        pics, gts = [pairs[i % 2][0] for i in range(a.batch)], [pairs[i % 2][1] for i in range(a.batch)]
        dpics, dgts = [torch.from_numpy(p).cuda() for p in pics], [torch.from_numpy(g).cuda() for g in gts]
        score, plain = E.SemsegBoundaryScore(pal), E.SemsegScore(pal)
        host = [B.boundary_confusion([p], [g], pal) for p, g in pairs]
        mult = [len(range(i, a.batch, 2)) for i in range(2)]
        conf, bconf = (sum(host[i][j] * mult[i] for i in range(2)) for j in range(2))
        score.add(dpics, dgts)
        got, bgot, pgot = score.matrix(), score.boundary_matrix(), plain.add(dpics, dgts).matrix()

        def torch_leg():
            return [torch_route(p, g, dpal, d) for p, g in zip(pics, dgts)]

        def host_leg():
            return [host_route(p, g, pal, d) for p, g in zip(dpics, gts)]

        check = dict(d=d, matrix_equals_statement=bool(np.array_equal(got, conf)), boundary_matrix_equals_statement=bool(np.array_equal(bgot, bconf)),
                     matrix_equals_plain_scorer=bool(got.tobytes() == pgot.tobytes()),
                     torch_route_equals_device=bool(np.array_equal(sum(m[1] for m in torch_leg()), bgot)),
                     host_route_equals_device=bool(np.array_equal(sum(m[1] for m in host_leg()), bgot)),
                     pixels=int(bgot.sum()), nonzero_boundary_bins=int((bgot != 0).sum()), off_boundary_pixels=int(bgot[0, 0]))
        print("%s: %s" % (tag, check), flush=True)
        assert check["matrix_equals_statement"] and check["boundary_matrix_equals_statement"] and check["matrix_equals_plain_scorer"], check
        summary["check"][tag] = check
        legs = {"boundary_add_ms": lambda: score.add(dpics, dgts), "score_add_ms": lambda: plain.add(dpics, dgts), "torch_route_ms": torch_leg,
                "host_route_ms": host_leg}
        t = summary["legs"][tag] = run_legs(tag, legs, a.rounds, a.iters)
        t["branch_cost_ms_median"] = round(t["boundary_add_ms"]["median"] - t["score_add_ms"]["median"], 3)
        for other in ("torch_route_ms", "host_route_ms"):
            t["boundary_add_vs_" + other[:-3]] = {"speedup_median": round(t[other]["median"] / t["boundary_add_ms"]["median"], 1),
                                                  "faster_beyond_the_spread": bool(t["boundary_add_ms"]["max"] < t[other]["min"])}
        # per batch, while it is scored; the scorers' matrices come back once per data set (2 (K + 1)^2 + 1 int64)
        summary["copied_back_bytes_per_batch"][tag] = {"boundary_add": 0, "score_add": 0, "torch_route": a.batch * 2 * (k + 1) ** 2 * 8,
                                                       "host_route": a.batch * h * w * 4,
                                                       "boundary_matrices_once_per_data_set": (2 * (k + 1) ** 2 + 1) * 8}
        summary["memory"][tag] = {name[:-3] + "_peak_MiB": round(peak_mb(fn), 1) for name, fn in legs.items()}
        summary["memory"][tag]["boundary_workspace_MiB"] = round(score.workspace.numel() / 2 ** 20, 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
