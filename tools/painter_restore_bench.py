"""Measure restoration scoring on the workload's shapes, a batch of eight pictures: 400 x 600 (lol, metric "skimage" on the float64
pictures) and 321 x 481 (derain, metric "matlab_y" on the saved uint8 pictures), in one process, legs alternated.

    python tools/painter_restore_bench.py [--rounds 5 --iters 1000 --batch 8] -> lines per round, then ONE JSON line

Before anything is timed the device records are compared with the host statement (tests/painter_restore_host.py: counts equal, the Y
squared sum equal, the float64 squared sum within 1e-12, SSIM within 1e-10), the largest SSIM deviation is printed, and the two baselines'
scores are compared with the device's.  Legs, milliseconds per BATCH, host clock around a window of runs that each END WITH THE SCORES ON THE
HOST (every leg synchronises; `iters` runs of the device leg, iters / 30 of the torch leg, one of the host leg per window), median and range over the rounds; the predictions are device-resident, as they are behind the decode:
    host_route    what the scripts do: the pictures' copy back, then the metric with scipy's filters and numpy means per picture
                  (tests/painter_restore_host.py, route "scipy")
    torch_route   the same op sequence with torch float64 convolutions on the same GPU (tests/painter_restore_host.torch_route), the
                  scores' copy back
    device_route  `RestorationScores(...).sums()`: one table copy, two launches, eight doubles per picture back
and the bytes each leg copies back per batch."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E         # noqa: E402
from tests import painter_restore_cases as C        # noqa: E402
from tests import painter_restore_host as H         # noqa: E402

SETTINGS = {"lol_400x600": ("skimage", 400, 600), "derain_321x481": ("matlab_y", 321, 481)}


def host_scores(pred, gt, metric):
    """The metric as the scripts' libraries compute it on the host: scipy's filters, numpy means."""
    if metric == "skimage":                                   # the script's own steps, without the statement's exactly rounded sum
        p, g = np.clip(pred, 0, 1), gt / 255.
        pairs = [(p[..., c], g[..., c]) for c in range(3)]
    else:
        pairs = [(H.y_channel(pred).astype(np.float64), H.y_channel(gt).astype(np.float64))]
    w = H.weights(metric)
    cov_norm, c1, c2 = H.constants(metric)
    d = np.stack([x - y for x, y in pairs])
    mse = np.mean(d * d)
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(1 / mse) if metric == "skimage" else 20 * np.log10(255 / np.sqrt(mse))
    return psnr, np.mean([H.ssim_map(x, y, w, cov_norm, c1, c2, "scipy").mean() for x, y in pairs])


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def legs_of(iters, host=None, torch_leg=None, device=None):
    return {"host_route_ms": (host, 1), "torch_route_ms": (torch_leg, max(iters // 30, 1)), "device_route_ms": (device, iters)}


def summarise(times):
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_restore_bench: needs the MI355X (nothing here is measured on a CPU)")
    summary = {"what": "restoration scores, batch %d" % a.batch, "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
               "unit": "ms per batch, scores on the host at the end of every run", "check": {}, "legs": {}, "bytes_back_per_batch": {}}
    for tag, (metric, h, w) in SETTINGS.items():
        # two distinct pictures, repeated through the batch
        cases = [C.inputs(*C.case("natural", 70 + i, h, w), metric) for i in range(2)]
        preds, gts = [cases[i % 2][0] for i in range(a.batch)], [cases[i % 2][1] for i in range(a.batch)]
        dpreds, dgts = [torch.from_numpy(p).cuda() for p in preds], [torch.from_numpy(g).cuda() for g in gts]

        def host_route():
            return [host_scores(p.cpu().numpy(), g, metric) for p, g in zip(dpreds, gts)]

        def torch_route():
            return torch.stack([torch.stack(s) for s in H.torch_route(dpreds, dgts, metric)]).cpu().numpy()

        def device_route():
            return E.RestorationScores(dpreds, dgts, metric).sums()

        sums = device_route()
        ok, worst = True, 0.0
        for i in range(2):
            ref = H.sums(*cases[i], metric)
            ok = ok and sums[i, 0] == ref[0] and np.array_equal(sums[i, 3::2], ref[3::2])
            ok = ok and (sums[i, 1] == ref[1] if metric == "matlab_y" else abs(sums[i, 1] - ref[1]) <= 1e-12 * ref[1])
            worst = max(worst, abs(float(H.metrics(sums[i], metric)[1]) - float(H.metrics(ref, metric)[1])))
        got = E.restoration_metrics(sums, metric)
        theirs, torchs = np.array(host_route()), torch_route()
        check = dict(device_equals_statement=bool(ok and worst <= 1e-10), largest_ssim_deviation_from_the_statement=worst,
                     host_route_ssim_minus_device=float(np.abs(theirs[:, 1] - got["ssim"]).max()),
                     torch_route_ssim_minus_device=float(np.abs(torchs[:, 1] - got["ssim"]).max()),
                     torch_route_psnr_minus_device=float(np.abs(torchs[:, 0] - got["psnr"]).max()),
                     psnr=float(got["psnr"][0]), ssim=float(got["ssim"][0]))
        print("%s: %s" % (tag, check), flush=True)
        assert check["device_equals_statement"], check
        summary["check"][tag] = check
        summary["runs_per_window"] = {name: n for name, (_, n) in legs_of(a.iters).items()}
        picture_bytes = sum(p.nbytes for p in preds)
        summary["bytes_back_per_batch"][tag] = dict(host_route=picture_bytes, torch_route=a.batch * 2 * 8, device_route=int(sums.nbytes))
        # runs per timed window, so that every window lasts a fraction of a second or more: the host leg takes that long per run, the
        # torch leg milliseconds, the device leg a fraction of one
        legs = legs_of(a.iters, host_route, torch_route, device_route)
        for fn, _ in legs.values():                               # warm-up of every shape the timed passes use
            fn()
        times = {k: [] for k in legs}
        for r in range(a.rounds):
            for name, (fn, iters) in legs.items():
                times[name].append(wall_ms(fn, iters))
            print("%s round %d  " % (tag, r) + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
        t = summary["legs"][tag] = summarise(times)
        for other in ("host_route_ms", "torch_route_ms"):
            t["device_route_vs_" + other[:-3]] = {"speedup_median": round(t[other]["median"] / t["device_route_ms"]["median"], 1),
                                                  "faster_beyond_the_spread": bool(t["device_route_ms"]["max"] < t[other]["min"])}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
