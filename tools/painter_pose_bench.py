"""Measure the pose keypoint decode on one synthetic batch of painted person boxes (32 boxes of 256 x 192 with their flipped twins, the
flip test with the one-column shift): painter_amd.painter_engine.keypoints from device-resident pictures against the reference's own op
sequence restated with torch on the same GPU (TopDownCustom.forward_pseudo_test, mmpose_custom/model/top_down.py:163-258: the float32
[n][18][H][W] distance tensor, `min`, 18 masks, 17 masked copies of R, `cat`, `.cpu().numpy()` of [n][17][H][W], the same again for the
flipped pictures, numpy flip_back / shift / average; then mmpose's argmax and the Python refinement loop over n x 17 heat maps as
tests/painter_pose_host.peaks states them), in one process, legs alternated.

    python tools/painter_pose_bench.py [--rounds 5 --iters 5 --boxes 32 --height 256 --width 192] -> lines per round, then one JSON line

Before anything is timed the device result is compared with the torch leg's (preds and maxvals equal).  Legs, milliseconds per batch
from HIP events around `iters` back-to-back runs (every leg ends with its copy back, so the events see the host work too), median and
range over the rounds:
  torch_route        the reference's op sequence from device-resident uint8 pictures to preds / maxvals on the host
  torch_heatmaps     its first part alone: up to the averaged float32 heat maps in numpy (no argmax, no refinement loop)
  keypoints          `keypoints(pictures, flipped)` from the same device-resident pictures: one memset, two launches, ONE copy back
  keypoints_launches the same launches without the copy back
and the peak of torch's allocator and the bytes copied back for both routes."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E       # noqa: E402
from tests import painter_pose_cases as C         # noqa: E402
from tests import painter_pose_host as H          # noqa: E402
from tools.painter_inst_bench import events_ms, peak_mb          # noqa: E402


def torch_heat(images, colors):
    """decode_images_to_heatmaps_minmax (top_down.py:219-258), line by line."""
    batch_size, image_height, image_width, _ = images.shape
    images = images.float()
    GB = images[..., 1:].view(batch_size, 1, image_height, image_width, 2)
    num_classes = colors.shape[0]
    dist = torch.abs(GB - colors.view(1, -1, 1, 1, 2)).sum(-1)
    dist, indices = torch.min(dist, dim=1)
    masks = [indices == idx for idx in range(num_classes)]
    R = images[..., 0]
    heatmaps = torch.cat([(masks[idx] * R).unsqueeze(1) for idx in range(num_classes) if idx != num_classes - 1], dim=1)
    return heatmaps.cpu().numpy() / 255.


def torch_heatmaps(dp, dq, colors, pair):
    out = torch_heat(dp, colors)
    flipped = H.flip_back(torch_heat(dq, colors), pair)
    flipped[:, :, :, 1:] = flipped[:, :, :, :-1]
    return (out + flipped) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_pose_bench: needs the MI355X (nothing here is measured on a CPU)")
    n, h, w = a.boxes, a.height, a.width
    p, q = C.painted_pair(9, n, h, w)
    dp, dq = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    colors = torch.tensor(E.pose_palette().tolist(), dtype=torch.float32, device="cuda")

    def torch_route():
        return H.peaks(torch_heatmaps(dp, dq, colors, C.PAIR))

    def heat_only():
        return torch_heatmaps(dp, dq, colors, C.PAIR)

    def ours():
        return E.keypoints(dp, dq)

    def launches():
        E.PoseDecode(dp, dq)

    res, (t_preds, t_maxvals) = ours(), torch_route()
    check = dict(preds_equal=bool(np.array_equal(res["preds"], t_preds)), maxvals_equal=bool(np.array_equal(res["maxvals"], t_maxvals)),
                 channels_with_a_peak=int((res["maxvals"] > 0).sum()), channels=int(res["maxvals"].size))
    print("device against the torch route: %s" % check, flush=True)
    assert check["preds_equal"] and check["maxvals_equal"], check
    legs = {"torch_route_ms": torch_route, "torch_heatmaps_ms": heat_only, "keypoints_ms": ours, "keypoints_launches_ms": launches}
    for fn in legs.values():                                  # warm-up of every shape the timed passes use
        fn()
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(events_ms(fn, a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
    mem = {"keypoints_peak_MiB": round(peak_mb(ours), 3), "torch_route_peak_MiB": round(peak_mb(torch_route), 1),
           "keypoints_copied_back_bytes": int(res["preds"].nbytes + res["maxvals"].nbytes),
           "torch_route_copied_back_bytes": int(2 * n * C.K * h * w * 4), "pictures_bytes": int(p.nbytes + q.nbytes)}
    summary = {"what": "pose keypoints, %d boxes of %dx%d, 17 keypoints, flip test with shift" % (n, h, w),
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "check": check, "memory": mem, "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    hi, lo = summary["legs"]["torch_route_ms"], summary["legs"]["keypoints_ms"]
    summary["keypoints_speedup_median"] = round(hi["median"] / lo["median"], 1)
    summary["keypoints_faster_beyond_the_spread"] = bool(lo["max"] < hi["min"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
