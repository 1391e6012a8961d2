"""Measure instance mask AP on the device (painter_amd.painter_engine.InstanceAP, csrc/painter_ap.hip) against the host statement
(tests/painter_ap_host.py: numpy on copied-back masks and Python loops -- restated from pycocotools' published source, unverified against
pycocotools), in one process, legs alternated.

    python tools/painter_ap_bench.py [--rounds 5 --iters 5 --host-iters 1 --height 480 --width 640] -> lines per round, then ONE JSON line

What a COCOeval user runs today -- RLE-encode every mask, write and reload a JSON file, maskUtils.iou on RLE, evaluateImg -- CANNOT be
timed here: pycocotools is not installed where this project is measured.  The host legs below are the restated statement, not pycocotools.

Before anything is timed the device records are compared with the host statement as bytes, for every form timed.  Legs, wall-clock
milliseconds per picture between two device synchronisations around back-to-back runs (`iters`; `host-iters` for the legs that are
host-bound), median and range over the rounds; every window is preceded by one untimed run of its own leg:
  host_statement      100 device-resident bool masks copied back, then the numpy statement (intersections as an int64 matrix product,
                      IoUs and the matching in Python loops), both modes
  torch_same_ops      the intersections as torch on the same GPU (`masks.flatten(1).float() @ gt.flatten(1).float().T`, areas as row
                      sums), the 100 x 30 matrix copied back, the statement's matching on the host
  add_masks           `InstanceAP.add` from device-resident bool masks (packs them to bits first) + `records()`
  add_bits            the same from device-resident bit masks, as the instance decode leaves them
  add_only            the launches of `add` from bit masks without `records()` (no copy back; the loop ends in a synchronisation)
  panoptic_then_host  `panoptic(semantic picture, instance picture)` with its copy back, then the host statement
  chained             `_launch_panoptic` + `InstanceAP.add_decodes` + `records()` from the same two pictures: only records are copied back
bytes_back: what each route copies from the device per picture."""
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
from tests import painter_ap_cases as C           # noqa: E402
from tests import painter_ap_host as H            # noqa: E402
from tests import painter_pano_cases as PC        # noqa: E402


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def equal(got, ref):
    return bool(len(got) == len(ref) and all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--ground-truths", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_ap_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w, k = a.height, a.width, 80
    dets, gts = C.case(5, h, w, a.ground_truths, a.detections, crowd=2, k=k)
    ref = H.picture_records(dets, gts, k)
    assert ref[1] == 0
    ref = [ref[0]]
    dmasks, gmasks = torch.from_numpy(dets["masks"]).cuda(), torch.from_numpy(gts["masks"]).cuda()
    dbits, gbits = (torch.from_numpy(C.bits_of(m).view(np.int32)).cuda() for m in (dets["masks"], gts["masks"]))
    scorer = lambda: E.InstanceAP(k, H.MODES)

    def add(masks, truth, records=True, **kw):
        s = scorer().add([masks], [dets["scores"]], [dets["classes"]], [truth], [gts["annotations"]], **kw)
        return s.records() if records else None

    def host_statement():
        return [H.picture_records(dict(dets, masks=dmasks.cpu().numpy()), gts, k)[0]]

    def torch_same_ops():
        d, g = dmasks.flatten(1).float(), gmasks.flatten(1).float()
        nd, ng = d.shape[0], g.shape[0]
        counts = torch.cat([(d @ g.T).ravel(), d.sum(1), g.sum(1)]).cpu().numpy().astype(np.int64)          # exact: every count < 2^24
        return [H.records_from_counts(counts[:nd * ng].reshape(nd, ng), counts[nd * ng:nd * ng + nd], counts[nd * ng + nd:], dets, gts)]

    sizes = dict(sizes=[(h, w)])
    check = dict(add_masks=equal(add(dmasks, gmasks), ref), add_bits=equal(add(dbits, gbits, **sizes), ref),
                 host_statement=equal(host_statement(), ref), torch_same_ops=equal(torch_same_ops(), ref), detections=len(ref[0]),
                 ground_truths=len(gts["annotations"]), matched_at_half=int((ref[0]["matched"][:, 0] & np.uint64(1) != 0).sum()))
    print("device against the host statement: %s" % check, flush=True)
    assert check["add_masks"] and check["add_bits"] and check["host_statement"] and check["torch_same_ops"]

    # the chain: two painted pictures -> instances with classes -> records
    sem, inst = PC.picture_pair(7, h, w, n_obj=24)
    dsem, dinst = torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda()
    merge = dict(dist_type="abs", overlap_threshold=0.5, stuff_area_thresh=8192, instances_score_thresh=0.55)
    res = E.panoptic(dsem, dinst)
    truth = C.gt_for_instances(9, res["masks"], res["classes"])
    tmasks = torch.from_numpy(truth["masks"]).cuda()
    ref2 = [H.picture_records(dict(masks=res["masks"], scores=res["scores"], classes=res["classes"]), truth, k)[0]]

    def panoptic_then_host():
        r = E.panoptic(dsem, dinst)
        return [H.picture_records(dict(masks=r["masks"], scores=r["scores"], classes=r["classes"]), truth, k)[0]]

    def chained():
        dec = E._launch_panoptic(dsem, dinst, None, None, 80, merge, {})
        return scorer().add_decodes([dec], [tmasks], [truth["annotations"]]).records()

    check.update(chained=equal(chained(), ref2), panoptic_then_host=equal(panoptic_then_host(), ref2), chain_detections=len(ref2[0]),
                 chain_ground_truths=len(truth["annotations"]), chain_matched_at_half=int((ref2[0]["matched"][:, 1] & np.uint64(1) != 0).sum()))
    print("chain: %s" % {key: check[key] for key in check if key.startswith("chain") or key == "panoptic_then_host"}, flush=True)
    assert check["chained"] and check["panoptic_then_host"]

    one = scorer().add([dbits], [dets["scores"]], [dets["classes"]], [gbits], [gts["annotations"]], **sizes)
    bytes_back = dict(host_statement=int(dmasks.numel()), torch_same_ops=4 * (len(dets["scores"]) * len(gts["annotations"]) + len(dets["scores"]) + len(gts["annotations"])),
                      add=int(one._outs[0][0].numel()), records_alone=48 * len(ref[0]))

    host_bound = ("host_statement_ms", "torch_same_ops_ms", "panoptic_then_host_ms")
    legs = {"host_statement_ms": host_statement, "torch_same_ops_ms": torch_same_ops, "add_masks_ms": lambda: add(dmasks, gmasks),
            "add_bits_ms": lambda: add(dbits, gbits, **sizes), "add_only_ms": lambda: add(dbits, gbits, False, **sizes),
            "panoptic_then_host_ms": panoptic_then_host, "chained_ms": chained}
    times = {key: [] for key in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(wall_ms(fn, a.host_iters if name in host_bound else a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (key, v[-1]) for key, v in times.items()), flush=True)
    summary = {"what": "instance mask AP, %dx%d, %d detections, %d ground truths, both modes, 10 thresholds x 4 area ranges"
                       % (h, w, len(ref[0]), len(gts["annotations"])), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
               "iters": a.iters, "host_iters": a.host_iters, "check": check, "bytes_back": bytes_back,
               "not_measured": "the RLE / JSON / pycocotools route (pycocotools is not installed)", "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    for lo, hi in (("add_masks_ms", "host_statement_ms"), ("add_bits_ms", "host_statement_ms"), ("add_masks_ms", "torch_same_ops_ms"),
                   ("add_bits_ms", "torch_same_ops_ms"), ("torch_same_ops_ms", "add_bits_ms"), ("chained_ms", "panoptic_then_host_ms")):
        x, y = summary["legs"][lo], summary["legs"][hi]
        summary["%s_faster_than_%s_beyond_both_spreads" % (lo[:-3], hi[:-3])] = bool(x["max"] < y["min"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
