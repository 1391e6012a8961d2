"""Measure COCO RLE on the device (painter_amd.painter_engine.RleEncode / rle_decode, csrc/painter_rle.hip) against the host route the
evaluator scripts imply, in one process, legs alternated.

    python tools/painter_rle_bench.py [--rounds 5 --iters 5 --host-iters 1 --height 480 --width 640] -> lines per round, then ONE JSON line

What the scripts run -- pycocotools.mask.encode / decode, C loops over copied-back masks -- CANNOT be timed here: pycocotools is not
installed where this project is measured.  The host legs below are the vectorised numpy statement (tests/painter_rle_host.py:
`flatnonzero` of the column-major difference, `np.repeat`), restated from pycocotools' published maskApi.c; its string loop is Python.

Before anything is timed the device strings are compared with the host statement and decoded back, for every form timed.  Legs,
wall-clock milliseconds per picture between two device synchronisations around back-to-back runs (`iters`; `host-iters` for the
host-bound legs), median and range over the rounds; every window is preceded by one untimed run of its own leg.  Every leg starts from the
painted picture and includes the instance decode (max_num masks), so the legs differ only in what follows it:
  decode_only          InstanceDecode, nothing copied back (the common part)
  masks_back_host_rle  (a) `instances()`: the bool masks copied back, then the numpy statement's counts and strings of every mask
  masks_back_counts    (a) without the Python string loop: copy back + numpy counts only (a lower bound for any host encoder)
  chained_rle          (b) InstanceDecode + RleEncode chained behind it + `instance_results`' copies back (prefix, header, records, strings)
  checkerboard_rle     (b) on a same-shape batch of checkerboards from device-resident bits: the most runs a mask can have; the default
                       pool overflows, so this leg is two launches
  rle_decode           (c) the strings of (b) -> bit masks on the device (upload of the strings included)
  host_decode_upload   (c) numpy decode of the same strings + upload of the dense masks + packing them to bits
bytes_back / bytes_up: what each route copies from / to the device per picture."""
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
from tests import painter_inst_cases as IC        # noqa: E402
from tests import painter_rle_cases as C          # noqa: E402
from tests import painter_rle_host as H           # noqa: E402


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--max-num", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_rle_bench: needs the MI355X (nothing here is measured on a CPU)")
    h, w, m = a.height, a.width, a.max_num
    pic = torch.from_numpy(IC.painted_picture(7, h, w, n_obj=24)).cuda()
    args = dict(E.INSTANCE_DEFAULTS, max_num=m)
    decode = lambda: E.InstanceDecode(pic, *args.values())

    def masks_back_counts():
        return [H.encode_fast(mask) for mask in decode().result()["masks"]]

    def masks_back_host_rle():
        return [H.to_string(c).decode("ascii") for c in masks_back_counts()]

    def chained_rle():
        return E.instance_results(decode(), 0)

    ref = decode().result()
    n = len(ref["scores"])
    entries, host_strings = chained_rle(), masks_back_host_rle()
    strings = [e["segmentation"]["counts"] for e in entries]
    rles = [e["segmentation"] for e in entries]
    board = C.checkerboard(h, w)
    board_bits = torch.from_numpy(np.repeat(H.pack_bits(board[None]), m, 0).view(np.int32)).cuda()
    board_count = torch.tensor([m], dtype=torch.int32, device="cuda")
    board_string = H.to_string(H.encode_fast(board)).decode("ascii")

    def checkerboard_rle():
        enc = E.RleEncode(board_bits, board_count, h, w, m)
        return enc, enc.result()

    def rle_decode():
        return E.rle_decode(rles)

    def host_decode_upload():
        dense = np.stack([H.decode(H.from_string(s), h, w) for s in strings])
        return E._bit_masks(dense, h, w, pic.device)[0]

    enc, board_res = checkerboard_rle()
    want_bits = H.pack_bits(ref["masks"])
    check = dict(instances=n, strings_equal_host=strings == host_strings, scores_equal=[e["score"] for e in entries] == [float(s) for s in ref["scores"]],
                 checkerboard_equal_host=board_res["strings"] == [board_string] * m, checkerboard_launches=enc.launches,
                 checkerboard_runs_per_mask=int(board_res["records"]["runs"][0]),
                 rle_decode_equal=bool(np.array_equal(rle_decode().cpu().numpy().view(np.uint32), want_bits)),
                 host_decode_equal=bool(np.array_equal(host_decode_upload().cpu().numpy().view(np.uint32), want_bits)),
                 runs_per_mask_median=float(np.median([len(H.from_string(s)) for s in strings])), characters=sum(len(s) for s in strings))
    print("device against the host statement: %s" % check, flush=True)
    assert check["strings_equal_host"] and check["scores_equal"] and check["checkerboard_equal_host"] and check["rle_decode_equal"] and \
        check["host_decode_equal"] and check["checkerboard_launches"] == 2

    dec = decode()
    one = E.InstanceResults(dec, 0)
    head = one.encode.at["records"][0] + E.RLE_RECORD.itemsize * m
    bytes_back = dict(masks_back=int(dec.out.numel()), masks_alone=n * h * w,
                      chained_rle=int(dec.obits) + head + check["characters"],
                      checkerboard_rle=2 * head + len(board_string) * m)
    bytes_up = dict(rle_decode=check["characters"] + 16 * n, host_decode_upload=n * h * w)

    host_bound = ("masks_back_host_rle_ms", "masks_back_counts_ms", "host_decode_upload_ms")
    legs = {"decode_only_ms": decode, "masks_back_host_rle_ms": masks_back_host_rle, "masks_back_counts_ms": masks_back_counts,
            "chained_rle_ms": chained_rle, "checkerboard_rle_ms": checkerboard_rle, "rle_decode_ms": rle_decode,
            "host_decode_upload_ms": host_decode_upload}
    times = {key: [] for key in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(wall_ms(fn, a.host_iters if name in host_bound else a.iters))
        print("round %d  " % r + "  ".join("%s %.3f" % (key, v[-1]) for key, v in times.items()), flush=True)
    summary = {"what": "COCO RLE, %dx%d, %d instance masks of a painted picture; checkerboard: %d masks of %d runs" %
                       (h, w, n, m, check["checkerboard_runs_per_mask"]), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
               "iters": a.iters, "host_iters": a.host_iters, "check": check, "bytes_back": bytes_back, "bytes_up": bytes_up,
               "not_measured": "pycocotools.mask.encode / decode (pycocotools is not installed); the host legs are the numpy statement",
               "legs": {}}
    for name, v in times.items():
        summary["legs"][name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    for lo, hi in (("chained_rle_ms", "masks_back_host_rle_ms"), ("chained_rle_ms", "masks_back_counts_ms"),
                   ("checkerboard_rle_ms", "masks_back_counts_ms"), ("rle_decode_ms", "host_decode_upload_ms")):
        x, y = summary["legs"][lo], summary["legs"][hi]
        summary["%s_faster_than_%s_beyond_both_spreads" % (lo[:-3], hi[:-3])] = bool(x["max"] < y["min"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
