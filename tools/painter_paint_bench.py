"""Measure the target encoders (painter_amd.painter_engine.paint_semantic / paint_instances / paint_pose, csrc/painter_paint.hip) against
the host route the reference's offline generators imply -- their op sequence in numpy, then the upload of the painted picture -- in one
process, legs alternated.

    python tools/painter_paint_bench.py [--rounds 5 --iters 10 --host-iters 1] -> lines per round, then ONE JSON line

The BASELINE of every case is the host route, never the code under test.  Before anything is timed the device pictures are compared
with the host route's, byte for byte.  Legs, wall-clock milliseconds per call between two device synchronisations around back-to-back
runs (`iters`; `host-iters` for the host legs), median and range over the rounds; every window is preceded by one untimed run of its leg:
  semantic   8 label maps of 512 x 683 (uint8)
    sem_host_upload      colorEncode's loop over the labels present (a compare, a tile and a multiply-add per label) + upload of 8 pictures
    sem_device_from_host paint_semantic on host maps: 8 uploads of 350 KB, ONE launch, the 4-byte counts back
    sem_device_resident  paint_semantic on maps already on the device
  instances  100 masks of 480 x 640
    inst_host_upload     SaveDataPairCustom's loop (center_of_mass on the dense mask, boolean-index paint) + upload of the picture
    inst_torch_same_gpu  the same loop in torch on the device-resident bool masks (one `.item()` per centre, as `int()` needs)
    inst_device_bits     paint_instances on device-resident bit masks (what `rle_decode` and the instance decode leave)
    inst_device_bool     paint_instances on host bool masks: the 30.7 MB upload and the packing included
    inst_device_rle      paint_instances on the masks' COCO RLE dicts: `rle_decode` on the device included
  pose       32 boxes of 256 x 192, 17 joints
    pose_host_upload     the MSRA heat maps for both sigmas + encode_rgb_target_to_image's array operations + upload of 32 pictures
    pose_device          paint_pose: rectangles and table on the host, one upload of a few KB, one launch
bytes_up / bytes_back: what each route moves to / from the device per call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E       # noqa: E402
from tests import painter_paint_cases as C        # noqa: E402
from tests import painter_paint_host as H         # noqa: E402


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def host_color_encode(labelmap, colors):
    """colorEncode's op sequence (gen_color_ade20k_sem.py:66-82), restated."""
    labelmap = labelmap.astype("int")
    rgb = np.zeros((labelmap.shape[0], labelmap.shape[1], 3), dtype=np.uint8)
    for label in np.unique(labelmap):
        if label <= 0:
            continue
        rgb += (labelmap == label)[:, :, np.newaxis] * np.tile(np.array(colors[label - 1], dtype=np.uint8), (labelmap.shape[0], labelmap.shape[1], 1))
    return rgb


def host_instances(masks):
    """SaveDataPairCustom.__call__'s loop with center_of_mass (transforms.py:109-128, :153-172), restated."""
    n, h, w = masks.shape
    seg = np.zeros((h, w, 3), dtype="uint8")
    grid_h, grid_w = np.arange(h)[:, None], np.arange(w)
    for idx in range(n):
        mask = masks[idx]
        norm = mask.sum().astype("float").clip(min=1e-6)
        cy, cx = (mask * grid_h).sum() / norm, (mask * grid_w).sum() / norm
        seg[mask.astype("bool")] = H.location_colour(int(cx / w * 79), int(cy / h * 79))
    return seg


def torch_instances(masks, pal):
    """The same loop in torch on device-resident bool masks."""
    n, h, w = masks.shape
    seg = torch.zeros((h, w, 3), dtype=torch.uint8, device=masks.device)
    grid_h, grid_w = torch.arange(h, device=masks.device)[:, None], torch.arange(w, device=masks.device)
    for idx in range(n):
        mask = masks[idx]
        norm = mask.sum().to(torch.float64).clamp(min=1e-6)
        cy, cx = (mask * grid_h).sum() / norm, (mask * grid_w).sum() / norm
        seg[mask] = pal[H.cell_row(int(cx / w * 79), int(cy / h * 79))]
    return seg


def host_pose(joints, visible, size):
    out = []
    for j, v in zip(joints, visible):
        tc, _, _ = H.msra_target(j, v, size, 1.5)
        tk, _, _ = H.msra_target(j, v, size, 3)
        out.append(H.pose_dense(tc, tk, H.pose_colours()))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # ---- inputs
    labels = [C._labels(512, 683, 20 + k, np.uint8) for k in range(8)]
    labels_d = [up(m) for m in labels]
    pal = H.ade_palette()
    masks = {n: m for n, m, _ in C.instance_cases()}["n100_480x640"]
    masks_d = up(masks)
    bits_d = up(H.pack_bits(masks).view(np.int32))
    rles = E.rle_encode(masks)[0]
    loc_d = up(E.location_palette().astype(np.uint8))
    j5, v5 = C.pose_boxes(192, 256)
    joints, visible = np.concatenate([j5] * 7)[:32], np.concatenate([v5] * 7)[:32]

    # ---- equality first
    sem_host = [host_color_encode(m, pal) for m in labels]
    sem_dev = E.paint_semantic(labels)
    inst_host = host_instances(masks)
    pose_host = host_pose(joints, visible, (192, 256))
    check = dict(
        semantic_equal=all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(sem_host, sem_dev)),
        instances_equal=all(inst_host.tobytes() == E.paint_instances(x, size=(480, 640))[0].cpu().numpy().tobytes() for x in (masks, bits_d, rles)),
        torch_route_equal=inst_host.tobytes() == torch_instances(masks_d, loc_d).cpu().numpy().tobytes(),
        pose_equal=pose_host.tobytes() == E.paint_pose(joints, visible)[0].cpu().numpy().tobytes())
    print("device against the host route:", check, flush=True)
    assert all(check.values()), check

    legs = {
        "sem_host_upload": (lambda: [up(host_color_encode(m, pal)) for m in labels], args.host_iters),
        "sem_device_from_host": (lambda: E.paint_semantic(labels), args.iters),
        "sem_device_resident": (lambda: E.paint_semantic(labels_d), args.iters),
        "inst_host_upload": (lambda: up(host_instances(masks)), args.host_iters),
        "inst_torch_same_gpu": (lambda: torch_instances(masks_d, loc_d), args.host_iters),
        "inst_device_bits": (lambda: E.paint_instances(bits_d, size=(480, 640)), args.iters),
        "inst_device_bool": (lambda: E.paint_instances(masks), args.host_iters),
        "inst_device_rle": (lambda: E.paint_instances(rles), args.iters),
        "pose_host_upload": (lambda: up(host_pose(joints, visible, (192, 256))), args.host_iters),
        "pose_device": (lambda: E.paint_pose(joints, visible), args.iters),
    }
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for k, (fn, iters) in legs.items():
            times[k].append(wall_ms(fn, iters))
        print("round %d  " % r + "  ".join("%s_ms %.3f" % (k, times[k][-1]) for k in legs), flush=True)
    pic = 512 * 683 * 3
    rle_chars = sum(len(r["counts"]) for r in rles)
    summary = {
        "what": "painted targets from annotations: 8 label maps of 512x683; 100 masks of 480x640; 32 pose boxes of 256x192, 17 joints",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "host_iters": args.host_iters, "check": check,
        "baseline": "the host route (the reference's op sequence in numpy + upload of the picture), never the code under test",
        "bytes_up": {"sem_host_upload": 8 * pic, "sem_device_from_host": 8 * 512 * 683 + 450 + 8 * 40, "sem_device_resident": 450 + 8 * 40,
                     "inst_host_upload": 480 * 640 * 3, "inst_torch_same_gpu": 0, "inst_device_bits": 19200, "inst_device_bool": masks.size + 19200,
                     "inst_device_rle": rle_chars + 16 * len(rles) + 19200, "pose_host_upload": 32 * 256 * 192 * 3,
                     "pose_device": 32 * 2 * 17 * 16 + 34 + 163},
        "bytes_back": {"sem_device_from_host": 32, "sem_device_resident": 32, "inst_device_bits": 804, "inst_device_bool": 804, "inst_device_rle": 804 + 400,
                       "inst_torch_same_gpu": 16 * 100, "pose_device": 0},
        "latency_bound": "pose_device and sem_device_* move 4.7 MB and 11 MB of output: at these sizes the legs are launch, upload and "
                         "synchronisation latency, not bandwidth",
        "legs": {k + "_ms": {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()},
    }
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
