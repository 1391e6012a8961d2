"""Measure the panoptic merge on one synthetic pair of painted 480 x 640 pictures (133 semantic colours, 80 things, up to 100
instances): painter_amd.painter_engine.panoptic against the evaluators' own op sequence run with torch on the same GPU
(tests/painter_pano_host.torch_evaluator_route: the float32 [H][W][133] distance tensor with its `.cpu().numpy()` round trip, the dense
einsum over float masks, the paste loop with its `.item()` calls), in one process, legs alternated.  Two settings: the evaluator's
defaults (overlap 0.5, stuff area 8192, score threshold 0.55) and score threshold 0.2, at which the paste loop runs long.

    python tools/painter_pano_bench.py [--rounds 5 --iters 5 --height 480 --width 640] -> lines per round, then one JSON line per setting

Before anything is timed the device result is compared with the host statement (tests/painter_pano_host.panoptic on the instances the
device decoded: classes, panoptic map, segments, areas equal), and the torch leg's result with the device's (its float32 vote may break a
tie differently: reported, not required).  Legs, milliseconds per picture pair from HIP events around `iters` back-to-back runs, median
and range over the rounds:
  torch_route       the evaluators' merge from device-resident instances (float masks, scores) -- the instance decode is NOT in it
  panoptic_supplied `panoptic(instances=...)` from the same device-resident masks: pack, vote, merge, copy back -- the like-for-like leg
  panoptic          `panoptic(semantic picture, instance picture)`: instance decode, merge, ONE copy back (the byte masks included)
  device_launches   the same launches without the copy back; pano_launches: pa_pano_decode alone behind a finished instance decode
  vote, merge       pa_pano_vote and pa_pano_merge alone; merge_no_paste: pa_pano_merge with a score threshold no instance passes.  The
                    union is then empty, so the paint pass searches no owner and the histogram counts every pixel: merge - merge_no_paste
                    is an UPPER bound of the single-workgroup paste loop (it also holds paint's owner search), not its kernel time
and the peak of torch's allocator for both routes."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import painter_engine as E       # noqa: E402
from painter_amd._lib import lib                  # noqa: E402
from tests import painter_pano_cases as C         # noqa: E402
from tests import painter_pano_host as H          # noqa: E402
from tools.painter_inst_bench import events_ms, peak_mb          # noqa: E402

SETTINGS = {"defaults": dict(overlap_threshold=0.5, stuff_area_thresh=8192, instances_score_thresh=0.55),
            "long_paste": dict(overlap_threshold=0.5, stuff_area_thresh=8192, instances_score_thresh=0.2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_pano_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w = a.height, a.width
    sem, inst = C.picture_pair(7, h, w, n_obj=24)
    pal = E.semantic_palette()
    dsem, dinst, dpal = torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda(), torch.from_numpy(pal.copy()).cuda()
    stream = E._stream()
    for setting, kw in SETTINGS.items():
        merge = dict(dist_type="abs", **kw)
        res = E.panoptic(dsem, dinst, **kw)
        n = len(res["scores"])
        host = H.panoptic(sem, pal, res["masks"], res["scores"], None, **kw)
        same = dict(classes=bool(np.array_equal(res["classes"], host["classes"])), panoptic=bool(np.array_equal(res["panoptic"], host["panoptic"])),
                    segments=bool(res["segments"] == host["segments"]), areas=bool(np.array_equal(res["areas"], host["areas"])))
        print("%s: %d instances, %d things + %d stuff segments, %d rejected for overlap, %d trimmed; device against the host statement: %s"
              % (setting, n, sum(s["isthing"] for s in host["segments"]), sum(not s["isthing"] for s in host["segments"]), host["rejected"],
                 host["trimmed"], same), flush=True)
        assert all(same.values()), same
        fmasks, dscores = torch.from_numpy(res["masks"]).cuda().float(), torch.from_numpy(res["scores"]).cuda()
        bmasks = fmasks.bool()

        def torch_route():
            return H.torch_evaluator_route(dsem, dpal, fmasks, dscores, **kw)

        t_pan, t_seg, t_cls = torch_route()
        check = dict(same, instances=n, segments_count=len(host["segments"]),
                     torch_route_classes_equal=int((t_cls == res["classes"]).sum()), torch_route_panoptic_equal=bool(np.array_equal(t_pan, res["panoptic"])))
        print("torch route: %d of %d classes equal the device's, panoptic map equal: %s" % (check["torch_route_classes_equal"], n,
              check["torch_route_panoptic_equal"]), flush=True)

        def ours():
            return E.panoptic(dsem, dinst, **kw)

        def supplied():
            return E.panoptic(dsem, instances=dict(masks=bmasks, scores=res["scores"], classes=None), **kw)

        def device_launches():
            E._launch_panoptic(dsem, dinst, None, None, 80, merge, {})

        tail = E.PanopticDecode.out_bytes(h, w, len(pal), 80, 100)
        dec = E.InstanceDecode(dinst, None, 19.0, 2000, 100, "gaussian", 2.0, tail=tail)

        def pano_launches():
            E.PanopticDecode(dsem, dec, None, None, 80, **merge)

        # the stages alone, through their own entry points, on the decode's device-resident outputs
        words = (h * w + 31) // 32
        masks_p, scores_p, count_p = (dec.out.data_ptr() + o for o in (dec.obits, dec.o32, 0))
        sums = torch.empty((100, 80), dtype=torch.int64, device="cuda")
        classes = torch.empty(100, dtype=torch.int32, device="cuda")
        semmap = torch.empty((h, w), dtype=torch.int32, device="cuda")
        E.check(lib.pa_palette_argmin(dsem.data_ptr(), dpal.data_ptr(), semmap.data_ptr(), h, w, len(pal), 0, stream), "pa_palette_argmin")
        ws = torch.empty(lib.pa_pano_workspace_bytes(h, w, len(pal), 80, 100), dtype=torch.uint8, device="cuda")
        pan = torch.empty((h, w), dtype=torch.int32, device="cuda")
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        cnt = torch.empty(1, dtype=torch.int32, device="cuda")
        seg = torch.empty((100 + len(pal) - 80) * E.SEGMENT.itemsize, dtype=torch.uint8, device="cuda")

        def vote():
            E.check(lib.pa_pano_vote(dsem.data_ptr(), dpal.data_ptr(), masks_p, count_p, h, w, len(pal), 80, 0, 100, sums.data_ptr(),
                                     classes.data_ptr(), stream), "pa_pano_vote")

        def merge_stage(score_thr=kw["instances_score_thresh"]):
            E.check(lib.pa_pano_merge(semmap.data_ptr(), masks_p, scores_p, classes.data_ptr(), count_p, h, w, len(pal), 80, 100,
                                      kw["overlap_threshold"], float(kw["stuff_area_thresh"]), score_thr, ws.data_ptr(), pan.data_ptr(),
                                      rgb.data_ptr(), cnt.data_ptr(), seg.data_ptr(), stream), "pa_pano_merge")

        vote()
        merge_stage()
        assert np.array_equal(pan.cpu().numpy(), res["panoptic"]) and np.array_equal(classes.cpu().numpy()[:n], res["classes"])
        legs = {"torch_route_ms": torch_route, "panoptic_supplied_ms": supplied, "panoptic_ms": ours, "device_launches_ms": device_launches,
                "pano_launches_ms": pano_launches, "vote_ms": vote, "merge_ms": merge_stage, "merge_no_paste_ms": lambda: merge_stage(2.0)}
        for fn in legs.values():                                  # warm-up of every shape the timed passes use
            fn()
        times = {k: [] for k in legs}
        for r in range(a.rounds):
            for name, fn in legs.items():
                times[name].append(events_ms(fn, a.iters))
            print("%s round %d  " % (setting, r) + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
        mem = {"panoptic_peak_MiB": round(peak_mb(ours), 1), "panoptic_supplied_peak_MiB": round(peak_mb(supplied), 1),
               "torch_route_peak_MiB": round(peak_mb(torch_route), 1)}
        summary = {"what": "panoptic merge, %dx%d, %d colours, 80 things, %d instances, %s %s" % (h, w, len(pal), n, setting, kw),
                   "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "check": check, "memory": mem, "legs": {}}
        for name, v in times.items():
            summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        hi = summary["legs"]["torch_route_ms"]
        for leg in ("panoptic_supplied_ms", "panoptic_ms"):
            lo = summary["legs"][leg]
            summary[leg[:-3] + "_speedup_median"] = round(hi["median"] / lo["median"], 1)
            summary[leg[:-3] + "_faster_beyond_the_spread"] = bool(lo["max"] < hi["min"])
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
