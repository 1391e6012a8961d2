"""Measure the nearest-colour (minmax) instance decode on one synthetic painted 480 x 640 picture with the default palette (6400 colours +
black): painter_amd.painter_engine.instances_minmax, instance_results and the nearest-colour kernel alone against the evaluator's own
op sequence run with torch on the same GPU (`torch_evaluator_route` below: four windows of an [H/4 + 1][W][6401][3] float32 difference
tensor, torch.min, one boolean mask and one torch.mean per colour found, a float32 [n][H][W] mask stack), in one process, legs
alternated.

    python tools/painter_minmax_bench.py [--rounds 5 --iters 3 --height 480 --width 640 --skip-host-check] -> lines per round, then one JSON line

Before anything is timed the device result is compared with the host statement (tests/painter_minmax_host.decode) -- label map, distance
map, records, masks: equal -- and the torch leg with the device: maps, instance order, masks and classes equal; its float32 scores may
differ where a sum exceeds 2^24 (reported, not required).  Per leg: milliseconds per picture from HIP events around `iters` back-to-back
runs, median and range over the rounds, and the peak of torch's allocator.  `*_with_copy` legs end with their results on the host (the
evaluator moves its Instances to the CPU, float32 masks included); the `*_device` legs stop at a synchronisation with everything still on
the device."""
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
from painter_amd._lib import lib                  # noqa: E402
from tests import painter_inst_cases as C         # noqa: E402
from tests import painter_minmax_host as H        # noqa: E402

NUM_WINDOWS = 4                                   # COCOEvaluatorCustom.__init__'s default
PAPER_PAIRS_PER_S = 256 * 4 * 16 * 2.4e9 / 2      # 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz, two VALU operations per (pixel, colour)


def torch_evaluator_route(segm_u8, palette):
    """The op sequence of post_process_segm_output_by_minmax (:188-247) on the device the tensors are on.  segm_u8: uint8 [H][W][3];
    palette: float32 [K][3] with the background row.  -> (scores, masks float32 [n][H][W], classes, dist_map, pred_map)"""
    pixels = segm_u8.float()[:, :, None, :]                      # [H][W][1][3]
    colours = palette[None, None]                                # [1][1][K][3]
    k, rows = palette.shape[0], segm_u8.shape[0] // NUM_WINDOWS + 1
    parts = []
    for top in range(0, NUM_WINDOWS * rows, rows):               # a [rows][W][K][3] float32 difference tensor per window
        parts.append((pixels[top:top + rows] - colours).abs().sum(-1).min(-1))
    dist_map, pred_map = torch.cat([p.values for p in parts]), torch.cat([p.indices for p in parts])
    found = torch.unique(pred_map)
    masks = [pred_map == c for c in found]                       # one boolean mask and one mean per colour found
    negs = torch.stack([dist_map[m].mean() for m in masks])
    classes = [int(c != k - 1) for c in found]                   # (one comparison on the host per colour, as the evaluator's loop has)
    scores = 1 - negs / max(negs.max(), 1.)
    return scores, torch.stack(masks).float(), torch.tensor(classes, device=pixels.device), dist_map, pred_map


def events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip-host-check", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_minmax_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w = a.height, a.width
    pic = C.painted_picture(7, h, w, n_obj=24)
    pal = H.with_background(E.location_palette())
    k = len(pal)
    dpic, dpal = torch.from_numpy(pic).cuda(), torch.from_numpy(pal).cuda()

    res = E.instances_minmax(dpic)
    n = len(res["scores"])
    print("picture %dx%d, %d colours: %d instances" % (h, w, k, n), flush=True)
    check = {"instances": n}
    if not a.skip_host_check:
        t0 = time.perf_counter()
        host = H.decode(pic, pal)
        print("host statement: %.1f s" % (time.perf_counter() - t0), flush=True)
        same = dict(label=bool(np.array_equal(res["pred_map"], host["label"])), dist=bool(np.array_equal(res["dist_map"], host["dist"].astype(np.float32))),
                    scores=bool(res["scores"].tobytes() == host["scores"].tobytes()), classes=bool(np.array_equal(res["labels"], host["classes"])),
                    candidates=bool(np.array_equal(res["candidates"], host["candidates"])),
                    masks=bool(np.array_equal(np.argmax(res["masks"], 0), host["slot"][host["label"]]) and (res["masks"].sum(0) == 1).all()),
                    ties=int(host["ties"]), largest_sum=int(host["S"].max()))
        print("device against the host statement:", same, flush=True)
        assert all(same[key] for key in ("label", "dist", "scores", "classes", "candidates", "masks")), same
        check.update(same)
    t_scores, t_masks, t_classes, t_dist, t_pred = torch_evaluator_route(dpic, dpal)
    check["torch_route"] = dict(pred_map=bool(np.array_equal(t_pred.cpu().numpy(), res["pred_map"])), dist_map=bool(np.array_equal(t_dist.cpu().numpy(), res["dist_map"])),
                                classes=bool(np.array_equal(t_classes.cpu().numpy(), res["labels"])),
                                masks=bool(torch.equal(t_masks > 0, torch.from_numpy(res["masks"]).cuda())),
                                scores_bit_equal=bool(t_scores.cpu().numpy().tobytes() == res["scores"].tobytes()),
                                score_err=float(np.abs(t_scores.cpu().numpy() - res["scores"]).max()))
    print("torch route against the device:", check["torch_route"], flush=True)
    assert all(check["torch_route"][key] for key in ("pred_map", "dist_map", "classes", "masks")), check["torch_route"]
    del t_masks
    stream = E._stream()
    label, dist = torch.empty(h * w, dtype=torch.int16, device="cuda"), torch.empty(h * w, dtype=torch.int16, device="cuda")

    def ours_with_copy():
        return E.instances_minmax(dpic)

    def ours_device():                                           # decode, count back, bit masks; nothing else leaves the device
        E.MinmaxDecode(dpic).bits()

    def ours_decode_only():                                      # pa_minmax_decode alone: no count back, no masks
        E.MinmaxDecode(dpic)

    def results():
        return E.instance_results(E.MinmaxDecode(dpic), 1)

    def torch_with_copy():
        scores, masks, classes, _, _ = torch_evaluator_route(dpic, dpal)
        return scores.cpu(), masks.cpu(), classes.cpu()

    def torch_device():
        torch_evaluator_route(dpic, dpal)

    def nearest_kernel():
        E.check(lib.pa_minmax_nearest(dpic.data_ptr(), dpal.data_ptr(), h, w, k, label.data_ptr(), dist.data_ptr(), stream), "pa_minmax_nearest")

    legs = {"instances_minmax_with_copy_ms": ours_with_copy, "torch_route_with_copy_ms": torch_with_copy, "minmax_device_ms": ours_device,
            "torch_route_device_ms": torch_device, "minmax_decode_only_ms": ours_decode_only, "instance_results_ms": results,
            "nearest_kernel_ms": nearest_kernel}
    for fn in legs.values():                                     # warm-up of every shape the timed passes use
        fn()
    times = {name: [] for name in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(events_ms(fn, a.iters * (20 if name == "nearest_kernel_ms" else 1)))
        print("round %d  " % r + "  ".join("%s %.3f" % (name, v[-1]) for name, v in times.items()), flush=True)
    mem = {"minmax_device_peak_MiB": round(peak_mb(ours_device), 1), "instances_minmax_with_copy_peak_MiB": round(peak_mb(ours_with_copy), 1),
           "torch_route_peak_MiB": round(peak_mb(torch_device), 1)}
    summary = {"what": "nearest-colour (minmax) instance decode, %dx%d, %d colours, %d instances" % (h, w, k, n),
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "check": check, "memory": mem, "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    legs = summary["legs"]
    for ours, theirs, key in (("instances_minmax_with_copy_ms", "torch_route_with_copy_ms", "with_copy"), ("minmax_device_ms", "torch_route_device_ms", "device")):
        summary["speedup_median_" + key] = round(legs[theirs]["median"] / legs[ours]["median"], 1)
        summary["faster_beyond_the_spread_" + key] = bool(legs[ours]["max"] < legs[theirs]["min"])
    paper = 1e3 * h * w * k / PAPER_PAIRS_PER_S
    summary["nearest_kernel_paper_ms"] = round(paper, 4)
    summary["nearest_kernel_over_paper"] = round(legs["nearest_kernel_ms"]["median"] / paper, 2)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
