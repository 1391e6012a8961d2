"""Measure the scoring routes on a batch of eight pictures: the confusion matrix of 512 x 683 ADE20K pictures (K = 150) and the depth
errors of 480 x 640 NYUv2 pictures, in one process, legs alternated.

    python tools/painter_score_bench.py [--rounds 5 --iters 3 --batch 8] -> lines per round, then ONE JSON line

Before anything is timed the device results are compared with the host statement (tests/painter_score_host.py: the matrix equal, n and
the counts equal, the sums within 1e-9 of sum |terms|), and the torch leg's matrix with the device's.  Legs, milliseconds per BATCH from
HIP events around `iters` back-to-back runs, median and range over the rounds; the pictures are device-resident, as they are behind
the decode, except for the torch leg, which uploads them as the evaluator does after reading its PNG:
  semseg, on the coherent case pictures (tests/painter_score_cases.painted) and on per-pixel noise (every lane another bin):
    torch_route      the evaluator's op sequence per picture with torch on the same GPU (tests/painter_score_host.torch_evaluator_route:
                     the float32 [H][W][K][3] tensor, the class map's copy to the host, np.bincount)
    class_map_route  `class_map` per picture (the int32 map's copy back) and np.bincount on the host
    score_add        `SemsegScore.add` of the batch: one launch, nothing copied back
    score_add_direct the same with the workgroups' bins forced out of LDS (every run of equal neighbours adds to memory)
  depth:
    numpy_route      the int32 pictures' copy back and the evaluation's numpy steps (eval_with_pngs.py:148-209, :50-71 restated) per picture
    depth_errors     `depth_errors` of the batch: two launches, ten doubles per picture back
and the peak of torch's allocator for the semantic legs."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E       # noqa: E402
from tests import painter_score_cases as C        # noqa: E402
from tests import painter_score_host as H         # noqa: E402
from tools.painter_inst_bench import events_ms, peak_mb          # noqa: E402


def numpy_depth_route(pred, gt, lo=1e-3, hi=10.0, box=H.EIGEN_CROP):
    """eval() and compute_errors of eval_with_pngs.py for one picture, in its float32 numpy."""
    p, g = pred.astype(np.float32) / 1000.0, gt.astype(np.float32) / 1000.0
    p[p < lo] = lo
    p[p > hi] = hi
    valid = np.logical_and(g > lo, g < hi)
    mask = np.zeros(valid.shape)
    mask[box[0]:box[1], box[2]:box[3]] = 1
    valid = np.logical_and(valid, mask)
    g, p = g[valid], p[valid]
    t = np.maximum(g / p, p / g)
    err = np.log(p) - np.log(g)
    return (np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100, np.mean(np.abs(np.log10(p) - np.log10(g))), np.mean(np.abs(g - p) / g),
            np.mean((g - p) ** 2 / g), np.sqrt(((g - p) ** 2).mean()), np.sqrt(((np.log(g) - np.log(p)) ** 2).mean()), (t < 1.25).mean(),
            (t < 1.25 ** 2).mean(), (t < 1.25 ** 3).mean())


def summarise(times):
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}


def run_legs(tag, legs, rounds, iters):
    for fn in legs.values():                                  # warm-up of every shape the timed passes use
        fn()
    times = {k: [] for k in legs}
    for r in range(rounds):
        for name, fn in legs.items():
            times[name].append(events_ms(fn, iters))
        print("%s round %d  " % (tag, r) + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
    return summarise(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_score_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w, pal = 512, 683, C.ade_palette().astype(np.float32)
    k, dpal = len(pal), torch.from_numpy(pal).cuda()
    summary = {"what": "semantic confusion matrix %dx%d K=%d and depth errors 480x640, batch %d" % (h, w, k, a.batch),
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "unit": "ms per batch", "check": {}, "legs": {},
               "memory": {}}
    # two distinct pictures per setting, repeated through the batch (the host statement runs on CPU torch: seconds per picture)
    settings = {"coherent": [C.semseg_case("ade", 40 + i, h, w)[:2] for i in range(2)],
                "noise": [C.noisy_case(50 + i, h, w, pal) for i in range(2)]}
    for tag, pairs in settings.items():
        pics, gts = [pairs[i % 2][0] for i in range(a.batch)], [pairs[i % 2][1] for i in range(a.batch)]
        dpics, dgts = [torch.from_numpy(p).cuda() for p in pics], [torch.from_numpy(g).cuda() for g in gts]
        score, direct = E.SemsegScore(pal), E.SemsegScore(pal)
        direct.bins = 1
        host = sum(H.confusion([pairs[i % 2][0]], [pairs[i % 2][1]], pal)[0] * len(range(i, a.batch, 2)) for i in range(2))
        got, got_direct = score.add(dpics, dgts).matrix(), direct.add(dpics, dgts).matrix()

        def torch_route():
            return sum(H.torch_evaluator_route(p, g, dpal) for p, g in zip(pics, gts))

        def class_map_route():
            return sum(np.bincount((k + 1) * E.class_map(p, pal).reshape(-1).astype(np.int64) + np.where(g == 255, k, g).reshape(-1).astype(np.int64),
                                   minlength=(k + 1) ** 2) for p, g in zip(dpics, gts))

        check = dict(device_equals_statement=bool(np.array_equal(got, host)), direct_equals_statement=bool(np.array_equal(got_direct, host)),
                     torch_route_equals_device=bool(np.array_equal(torch_route(), got)),
                     class_map_route_equals_device=bool(np.array_equal(class_map_route().reshape(k + 1, k + 1), got)),
                     pixels=int(got.sum()), nonzero_bins=int((got != 0).sum()))
        print("%s: %s" % (tag, check), flush=True)
        assert check["device_equals_statement"] and check["direct_equals_statement"], check
        summary["check"][tag] = check
        legs = {"torch_route_ms": torch_route, "class_map_route_ms": class_map_route, "score_add_ms": lambda: score.add(dpics, dgts),
                "score_add_direct_ms": lambda: direct.add(dpics, dgts)}
        summary["legs"][tag] = run_legs(tag, legs, a.rounds, a.iters)
        summary["memory"][tag] = {name[:-3] + "_peak_MiB": round(peak_mb(fn), 1) for name, fn in legs.items()}
        t = summary["legs"][tag]
        for other in ("torch_route_ms", "class_map_route_ms"):
            summary["legs"][tag]["score_add_vs_" + other[:-3]] = {"speedup_median": round(t[other]["median"] / t["score_add_ms"]["median"], 1),
                                                                  "faster_beyond_the_spread": bool(t["score_add_ms"]["max"] < t[other]["min"])}
    # depth
    cases = [C.depth_case(60 + i, 480, 640) for i in range(2)]
    preds, gts = [cases[i % 2][0] for i in range(a.batch)], [cases[i % 2][1] for i in range(a.batch)]
    dpreds, dgts = [torch.from_numpy(p).cuda() for p in preds], [torch.from_numpy(g.view(np.int16)).cuda() for g in gts]
    kw = dict(max_depth=10.0, crop="eigen")
    sums = E.DepthErrors(dpreds, dgts, **kw).sums()
    ok = True
    for i in range(2):
        ref, abs_log, _ = H.depth_sums(*cases[i], **kw)
        scale = np.array([ref[4], ref[5], ref[6], ref[7], abs_log, ref[9]])
        ok = ok and np.array_equal(sums[i, :4], ref[:4]) and bool((np.abs(sums[i, 4:] - ref[4:]) <= 1e-9 * scale).all())
    metrics = E.depth_errors(dpreds, dgts, **kw)[0]
    theirs = np.array([numpy_depth_route(preds[i], gts[i]) for i in range(2)], np.float64)
    summary["check"]["depth"] = dict(device_equals_statement=bool(ok), valid_pixels=int(sums[0, 0]),
                                     worst_relative_distance_to_the_float32_route=float(np.max(np.abs(metrics[:2] - theirs) / np.abs(theirs))))
    print("depth: %s" % summary["check"]["depth"], flush=True)
    assert ok
    legs = {"numpy_route_ms": lambda: [numpy_depth_route(p.cpu().numpy(), g) for p, g in zip(dpreds, gts)],
            "depth_errors_ms": lambda: E.depth_errors(dpreds, dgts, **kw)}
    summary["legs"]["depth"] = run_legs("depth", legs, a.rounds, a.iters)
    t = summary["legs"]["depth"]
    summary["legs"]["depth"]["depth_errors_vs_numpy_route"] = {"speedup_median": round(t["numpy_route_ms"]["median"] / t["depth_errors_ms"]["median"], 1),
                                                               "faster_beyond_the_spread": bool(t["depth_errors_ms"]["max"] < t["numpy_route_ms"]["min"])}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
