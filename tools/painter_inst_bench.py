"""Measure the class-agnostic instance decode on one synthetic painted 480 x 640 picture, K = 6400 colours, thresholds [19.] (the
evaluator's defaults): painter_amd.painter_engine.instances against the evaluator's own op sequence run with torch on the same GPU
(tests/painter_inst_host.torch_evaluator_route: eight chunks of an [800][H][W][3] float32 difference tensor, float32 masks, a dense
fp32 torch.mm), in one process, legs alternated.

    python tools/painter_inst_bench.py [--rounds 5 --iters 5 --height 480 --width 640 --skip-host-check] -> lines per round, then one JSON line

Before anything is timed the device result is compared with the host statement (tests/painter_inst_host.decode: exact integers,
float64): kept candidates, masks and order equal, scores within 1e-9; and the torch leg's masks are compared with the device's (they may
differ where the float32 route breaks a tie differently: reported, not required).  Per leg: milliseconds per picture from HIP events
around `iters` back-to-back runs that end in their copy back, median and range over the rounds, and the peak of torch's allocator.  The
statistics and the intersection stage are also timed alone through their own entry points (on the survivors' masks of the decode), to
show which stage the time goes to."""
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
from tests import painter_inst_host as H          # noqa: E402

THR, NMS_PRE, MAX_NUM = [19.0], 2000, 100


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip-host-check", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_inst_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w = a.height, a.width
    pic = C.painted_picture(7, h, w, n_obj=24)
    pal = E.location_palette()
    dpic, dpal = torch.from_numpy(pic).cuda(), torch.from_numpy(pal.copy()).cuda()

    def ours():
        return E.instances(dpic, dist_thr=THR, nms_pre=NMS_PRE, max_num=MAX_NUM)

    def torch_route():
        scores, masks = H.torch_evaluator_route(dpic, dpal, THR, NMS_PRE, MAX_NUM)
        return scores.cpu().numpy(), masks.cpu().numpy()

    dec = E.InstanceDecode(dpic, None, THR, NMS_PRE, MAX_NUM, "gaussian", 2.0)
    res = dec.result(with_f64=True)
    live, n_surv = (int(v) for v in dec.section(2, np.int32, 2))
    print("picture %dx%d: %d live candidates, %d survivors, %d kept" % (h, w, live, n_surv, len(res["scores"])), flush=True)
    check = {"live": live, "n_survivors": n_surv}
    if not a.skip_host_check:
        t0 = time.perf_counter()
        host = H.decode(pic, pal, THR, NMS_PRE, MAX_NUM)
        print("host statement: %.1f s" % (time.perf_counter() - t0), flush=True)
        m = C.K * len(THR)
        same = dict(stats=bool(np.array_equal(dec.section(0, np.uint32, m), host["n"]) and np.array_equal(dec.section(1, np.uint64, m), host["s"])),
                    survivors=bool(np.array_equal(dec.section(3, np.int32, NMS_PRE)[:n_surv], host["survivors"])),
                    candidates=bool(np.array_equal(res["candidates"], host["candidates"])),
                    masks=bool(np.array_equal(res["masks"], host["masks"])),
                    score_err=float(np.abs(res["scores_f64"] - host["scores"]).max()))
        print("device against the host statement:", same, flush=True)
        assert same["stats"] and same["survivors"] and same["candidates"] and same["masks"] and same["score_err"] <= 1e-9, same
        check.update(same)
    t_scores, t_masks = torch_route()
    agree = int(sum(np.array_equal(x, y) for x, y in zip(t_masks, res["masks"])))
    check["torch_route_masks_equal_to_device_in_order"] = agree
    check["torch_route_score_err"] = float(np.abs(t_scores[:len(res["scores"])] - res["scores"]).max())
    print("torch route: %d of %d masks equal the device's at the same position, scores differ by %.3e" %
          (agree, len(res["scores"]), check["torch_route_score_err"]), flush=True)

    # the two big stages alone, through their own entry points
    stream = E._stream()
    thr = torch.tensor(THR, dtype=torch.float32, device="cuda")
    n_out = torch.empty(C.K, dtype=torch.int32, device="cuda")
    s_out = torch.empty(C.K, dtype=torch.int64, device="cuda")
    stride = int(lib.pa_inst_workspace_offset(*dec.shape, 9))
    off = lib.pa_inst_workspace_offset(*dec.shape, 6)
    bits = dec.workspace[off:off + 4 * n_surv * stride].clone()
    inter = torch.empty((n_surv, n_surv), dtype=torch.int32, device="cuda")

    def stats_stage():
        E.check(lib.pa_inst_stats(dpic.data_ptr(), dpal.data_ptr(), thr.data_ptr(), n_out.data_ptr(), s_out.data_ptr(), h, w, C.K, 1, stream), "pa_inst_stats")

    def inter_stage():
        E.check(lib.pa_inst_intersections(bits.data_ptr(), n_surv, stride, inter.data_ptr(), n_surv, stream), "pa_inst_intersections")

    def device_only():
        E.InstanceDecode(dpic, None, THR, NMS_PRE, MAX_NUM, "gaussian", 2.0)

    legs = {"instances_ms": ours, "torch_route_ms": torch_route, "device_decode_only_ms": device_only, "stats_stage_ms": stats_stage,
            "intersection_stage_ms": inter_stage}
    for fn in legs.values():                                  # warm-up of every shape the timed passes use
        fn()
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(events_ms(fn, a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
    mem = {"instances_peak_MiB": round(peak_mb(ours), 1), "torch_route_peak_MiB": round(peak_mb(torch_route), 1)}
    summary = {"what": "class-agnostic instance decode, %dx%d, K %d, thresholds %s, nms_pre %d, max_num %d" % (h, w, C.K, THR, NMS_PRE, MAX_NUM),
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "check": check, "memory": mem, "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    lo, hi = summary["legs"]["instances_ms"], summary["legs"]["torch_route_ms"]
    summary["speedup_median"] = round(hi["median"] / lo["median"], 1)
    summary["faster_beyond_the_spread"] = bool(lo["max"] < hi["min"])
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
