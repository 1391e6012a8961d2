"""Measure COCO keypoint AP on the device (painter_amd.painter_engine.KeypointAP, csrc/painter_kpt.hip) against the host statement
(tests/painter_kpt_host.py: numpy on copied-back preds / maxvals and Python loops -- restated from the published source of mmpose's oks_nms
and xtcocotools' COCOeval, unverified against mmpose / xtcocotools), in one process, legs alternated.

    python tools/painter_kpt_bench.py [--rounds 5 --iters 5 --host-iters 1 --photos 200 --boxes 12 --ground-truths 4] -> lines per round, then ONE JSON line

What a user of the reference runs today -- mmpose's oks_nms, a JSON file written and reloaded, xtcocotools' COCOeval -- CANNOT be timed
here: neither mmpose nor xtcocotools is installed where this project is measured.  The host legs below are the restated statement.

Before anything is timed the device records are compared with the host statement as bytes (the case is one whose decisions do not change
when every OKS is scaled by 1 -+ 1e-9, tests/painter_kpt_cases.py) and the OKS doubles of the workspace within 1e-12; the largest relative
difference is printed.  Legs, wall-clock milliseconds per data set between two device synchronisations around back-to-back runs (`iters`;
`host-iters` for the host-bound legs), median and range over the rounds; every window is preceded by one untimed run of its own leg:
  host_statement      device-resident preds / maxvals copied back, then the numpy statement: poses, rescoring, NMS, OKS, matching
  add_records         `KeypointAP.add` from the same device-resident preds / maxvals + `records()`: one copy back of the records
  add_only            the launches of `add` alone (no copy back; the loop ends in a synchronisation)
  run_pose_then_host  `PainterEngine.run_pose` (stand-in model of tests/painter_eval_cases.py, flip test by mirroring) with its copy back
                      per batch, then the host statement
  run_pose_ap         `PainterEngine.run_pose_ap` + `records()` on the same queries: only records are copied back
bytes_back: what each route copies from the device per data set."""
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
from tests import painter_eval_cases as PC        # noqa: E402
from tests import painter_kpt_cases as C          # noqa: E402
from tests import painter_kpt_host as H           # noqa: E402


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def equal(got, ref):
    return bool(sorted(got) == sorted(ref) and all(got[i].tobytes() == ref[i].tobytes() for i in ref))


def host_records(case, preds, maxvals, heat=C.HEAT):
    pose, scores, areas = H.poses(preds, maxvals, case["centers"], case["scales"], case["box_scores"], heat)
    out = H.dataset_records(pose, scores, areas, case["image_ids"], case["bbox_ids"], case["ground_truth"])
    return {i: r["records"] for i, r in out.items()}, out


def oks_difference(ap, ref):
    """The largest relative difference between the workspace's OKS doubles and the statement's."""
    _, _, ws, shape, images = ap._last_eval
    n, d_cap, g_cap, max_det = shape
    at = lib.pa_kpt_workspace_offset(*shape, 2)
    oks = ws[at:at + 8 * n * max_det * g_cap].cpu().numpy().view(np.float64).reshape(n, max_det, g_cap)
    worst = 0.0
    for j, image in enumerate(images):
        want = ref[image]["oks"]
        got = oks[j, :want.shape[0], :want.shape[1]]
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), image
        if (want > 0).any():
            worst = max(worst, float((np.abs(got - want)[want > 0] / want[want > 0]).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--photos", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--ground-truths", type=int, default=4)
    ap.add_argument("--queries", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_kpt_bench: needs the MI355X (nothing here is measured on a CPU)")
    case = C.dataset(21, [(a.boxes, a.ground_truths)] * a.photos)
    ref = {i: r["records"] for i, r in case["statement"].items()}
    dpreds, dmaxvals = torch.from_numpy(case["preds"]).cuda(), torch.from_numpy(case["maxvals"]).cuda()
    ids = (case["centers"], case["scales"], case["box_scores"], case["image_ids"])

    def add(records=True):
        s = E.KeypointAP(case["ground_truth"]).add(dpreds, dmaxvals, *ids)
        return s.records() if records else s

    def host_statement():
        return host_records(case, dpreds.cpu().numpy(), dmaxvals.cpu().numpy())[0]

    one = add(False)
    check = dict(add_records=equal(one.records(), ref), host_statement=equal(host_statement(), ref), photos=a.photos, boxes=len(case["image_ids"]),
                 evaluated=int(sum(len(r) for r in ref.values())), survivors=int(sum(one.survivors.values())),
                 matched_at_half=int(sum(int((r["matched"] & np.uint64(1) != 0).sum()) for r in ref.values())),
                 largest_relative_oks_difference=oks_difference(one, case["statement"]))
    print("device against the host statement: %s" % check, flush=True)
    assert check["add_records"] and check["host_statement"]

    # the chain: queries -> stand-in forward -> keypoint decode -> records
    rng = np.random.default_rng(4)
    queries = [PC.picture(200 + i, 64, 48) for i in range(a.queries)]
    people = [C.person(rng) for _ in range(a.queries)]
    chain = dict(centers=np.stack([p[1] for p in people]), scales=np.stack([p[2] for p in people]),
                 box_scores=(np.round(rng.uniform(0.25, 1, a.queries) * 8) / 8).astype(np.float32), image_ids=[i // 4 for i in range(a.queries)],
                 bbox_ids=None, ground_truth={i: [p[0] for p in people[4 * i:4 * i + 2]] for i in range((a.queries + 3) // 4)})
    engine = E.PainterEngine(PC.StandInModel(), "cuda", "coco_pose", *PC.prompt_pair(), input_size=PC.RES, batch_size=8)
    cids = (chain["centers"], chain["scales"], chain["box_scores"], chain["image_ids"])

    def run_pose_then_host():
        back = engine.run_pose(queries, "mirror")
        return host_records(chain, np.stack([b["preds"] for b in back]), np.stack([b["maxvals"] for b in back]))[0]

    def run_pose_ap():
        return engine.run_pose_ap(queries, *cids, E.KeypointAP(chain["ground_truth"]), "mirror").records()

    # the chain's case is not screened by the nudge condition: the two routes are compared, and a difference is reported, not asserted
    check.update(chain_equal=equal(run_pose_ap(), run_pose_then_host()), chain_queries=a.queries)
    print("chain: %s" % {key: check[key] for key in check if key.startswith("chain")}, flush=True)

    k = one.k
    bytes_back = dict(host_statement=int(4 * 3 * k * len(case["image_ids"])), add_records=int(sum(o.numel() for o, _, _ in one._outs)),
                      records_alone=32 * check["evaluated"], run_pose_then_host=int(4 * 3 * k * a.queries))
    host_bound = ("host_statement_ms", "run_pose_then_host_ms")
    legs = {"host_statement_ms": host_statement, "add_records_ms": add, "add_only_ms": lambda: add(False),
            "run_pose_then_host_ms": run_pose_then_host, "run_pose_ap_ms": run_pose_ap}
    times = {key: [] for key in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(wall_ms(fn, a.host_iters if name in host_bound else a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (key, v[-1]) for key, v in times.items()), flush=True)
    summary = {"what": "COCO keypoint AP, %d photos, %d boxes, %d ground truths, 17 keypoints, 10 thresholds x 3 area ranges, max_det 20; chain: %d "
                       "queries through the stand-in model" % (a.photos, len(case["image_ids"]), a.photos * a.ground_truths, a.queries),
               "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "host_iters": a.host_iters, "check": check,
               "bytes_back": bytes_back, "not_measured": "the mmpose oks_nms / JSON / xtcocotools route (neither is installed)", "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    for lo, hi in (("add_records_ms", "host_statement_ms"), ("run_pose_ap_ms", "run_pose_then_host_ms")):
        x, y = summary["legs"][lo], summary["legs"][hi]
        summary["%s_faster_than_%s_beyond_both_spreads" % (lo[:-3], hi[:-3])] = bool(x["max"] < y["min"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
