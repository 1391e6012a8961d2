"""Measure panoptic quality on the device (painter_amd.painter_engine.PanopticQuality, csrc/painter_pq.hip) against the host statement
(tests/painter_pq_host.py: numpy's np.unique over the picture and Python loops, what a panopticapi user runs today -- restated from
panopticapi's published source, unverified against panopticapi), in one process, legs alternated.

    python tools/painter_pq_bench.py [--rounds 5 --iters 5 --height 480 --width 640] -> lines per round, then ONE JSON line

Before anything is timed the device counts are compared with the host statement (integers equal, IoU sums equal as bytes), for every
form timed.  Legs, wall-clock milliseconds per picture between two device synchronisations around `iters` back-to-back runs, median and
range over the rounds; every window is preceded by one untimed run of its own leg, so that a host-bound leg before it does not leave
the device idle when the window opens:
  host_statement      a device-resident panoptic map copied back, then the host statement on it (its segment lists are on the host)
  add_lds, add_direct `PanopticQuality.add` + `counts()` from device-resident maps (about 20 predicted, 30 ground-truth segments): the
                      count kernel's bins in LDS, and the forced direct form
  add_lds_noisy, add_direct_noisy   the same two with a fifth of the pixels of both maps replaced at random: runs of one or two pixels
  add_caps_max        the first at the capacities 254 x 255, where the bins cannot be in LDS
  add_only_lds / add_only_direct   the launches of `add` without `counts()` (no copy back; the host enqueues and the loop ends in a
                      synchronisation)
  panoptic_then_host  `panoptic(semantic picture, instance picture)` with its copy back, then the host statement
  chained             `_launch_panoptic` + `PanopticQuality.add_decodes` + `counts()` from the same two pictures: nothing but the counts
                      is copied back"""
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
from tests import painter_pano_cases as PC        # noqa: E402
from tests import painter_pq_cases as C           # noqa: E402
from tests import painter_pq_host as H            # noqa: E402


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def equal(got, ref):
    return bool(all(np.array_equal(g, r) for g, r in zip(got[:3], ref[:3])) and got[3].tobytes() == ref[3].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_pq_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w = a.height, a.width
    case = C.case(5, h, w, 30, 20)
    ref, flags = H.pq([case["pred"]], [case["pred_segments"]], [case["gt"]], [case["gt_segments"]])
    assert flags == [0]
    dpred, dgt = torch.from_numpy(case["pred"]).cuda(), torch.from_numpy(case["gt"]).cuda()
    runs = int((np.diff(case["pred"].ravel()) != 0).sum() + 1)

    noisy = C.case(6, h, w, 30, 20, noise=0.2)
    nref, nflags = H.pq([noisy["pred"]], [noisy["pred_segments"]], [noisy["gt"]], [noisy["gt_segments"]])
    assert nflags == [0]
    npred, ngt = torch.from_numpy(noisy["pred"]).cuda(), torch.from_numpy(noisy["gt"]).cuda()

    def add(bins, caps, counts=True, which=None):
        s = E.PanopticQuality()
        s.bins, s.min_caps = bins, caps
        if which is None:
            s.add([dpred], [case["pred_segments"]], [dgt], [case["gt_segments"]])
        else:
            s.add([npred], [noisy["pred_segments"]], [ngt], [noisy["gt_segments"]])
        return s.counts() if counts else None

    def host_statement():
        return H.pq([dpred.cpu().numpy()], [case["pred_segments"]], [case["gt"]], [case["gt_segments"]])[0]

    check = dict(lds=equal(add(0, (1, 1)), ref), direct=equal(add(1, (1, 1)), ref), caps_max=equal(add(0, (254, 255)), ref),
                 tp=int(ref[0].sum()), fp=int(ref[1].sum()), fn=int(ref[2].sum()), predicted=len(case["pred_segments"]),
                 ground_truth=len(case["gt_segments"]), runs_of_equal_predicted_ids=runs,
                 noisy_lds=equal(add(0, (1, 1), which="noisy"), nref), noisy_direct=equal(add(1, (1, 1), which="noisy"), nref),
                 noisy_runs_of_equal_predicted_ids=int((np.diff(noisy["pred"].ravel()) != 0).sum() + 1))
    print("device against the host statement: %s" % check, flush=True)
    assert check["lds"] and check["direct"] and check["caps_max"] and check["noisy_lds"] and check["noisy_direct"]

    # the chain: two painted pictures -> panoptic map -> PQ
    sem, inst = PC.picture_pair(7, h, w, n_obj=24)
    dsem, dinst = torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda()
    merge = dict(dist_type="abs", overlap_threshold=0.5, stuff_area_thresh=8192, instances_score_thresh=0.55)
    res = E.panoptic(dsem, dinst)
    gt2, seg2 = C.gt_for_map(9, res["panoptic"], res["segments"])
    ref2, flags2 = H.pq([res["panoptic"]], [res["segments"]], [gt2], [seg2])
    assert flags2 == [0]
    dgt2 = torch.from_numpy(gt2).cuda()

    def panoptic_then_host():
        r = E.panoptic(dsem, dinst)
        return H.pq([r["panoptic"]], [r["segments"]], [gt2], [seg2])[0]

    def chained():
        dec = E._launch_panoptic(dsem, dinst, None, None, 80, merge, {})
        return E.PanopticQuality().add_decodes([dec], [dgt2], [seg2]).counts()

    check.update(chained=equal(chained(), ref2), panoptic_then_host=equal(panoptic_then_host(), ref2), chain_segments=len(res["segments"]),
                 chain_tp=int(ref2[0].sum()))
    print("chain: %s" % {k: check[k] for k in ("chained", "panoptic_then_host", "chain_segments", "chain_tp")}, flush=True)
    assert check["chained"] and check["panoptic_then_host"]

    legs = {"host_statement_ms": host_statement, "add_lds_ms": lambda: add(0, (1, 1)), "add_direct_ms": lambda: add(1, (1, 1)),
            "add_lds_noisy_ms": lambda: add(0, (1, 1), which="noisy"), "add_direct_noisy_ms": lambda: add(1, (1, 1), which="noisy"),
            "add_caps_max_ms": lambda: add(0, (254, 255)), "add_only_lds_ms": lambda: add(0, (1, 1), False),
            "add_only_direct_ms": lambda: add(1, (1, 1), False), "panoptic_then_host_ms": panoptic_then_host, "chained_ms": chained}
    for fn in legs.values():                                  # warm-up of every shape the timed passes use
        fn()
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(wall_ms(fn, a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (k, v[-1]) for k, v in times.items()), flush=True)
    summary = {"what": "panoptic quality, %dx%d, 133 classes" % (h, w), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
               "iters": a.iters, "check": check, "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    for lo, hi in (("add_lds_ms", "host_statement_ms"), ("add_direct_ms", "host_statement_ms"), ("add_lds_ms", "add_direct_ms"),
                   ("add_direct_ms", "add_lds_ms"), ("add_lds_noisy_ms", "add_direct_noisy_ms"), ("add_direct_noisy_ms", "add_lds_noisy_ms"), ("add_only_lds_ms", "add_only_direct_ms"), ("add_only_direct_ms", "add_only_lds_ms"),
                   ("chained_ms", "panoptic_then_host_ms")):
        x, y = summary["legs"][lo], summary["legs"][hi]
        summary["%s_faster_than_%s_beyond_both_spreads" % (lo[:-3], hi[:-3])] = bool(x["max"] < y["min"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
