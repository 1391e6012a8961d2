"""Measure Painter task inference end to end (ADE20K semantic segmentation settings): the reference script's host path around the
model call, batch 1 -- what a user gets by running Painter/eval/ade20k_semantic/painter_inference_segm.py unchanged on this module --
against painter_amd.painter_engine.PainterEngine at batch 1, 8 and 32.  ViT-L, random weights, synthetic 640 x 480 pictures held in
memory (no file I/O), one process, legs alternated.

    python tools/painter_eval_bench.py [--pictures 64 --rounds 3 --batches 1,8,32] -> one line per leg and round, then one JSON line

Per leg: images/s end to end (wall clock around work that ends in a synchronise / the copy back) and, from a second, instrumented
pass, milliseconds per image in pre-processing, forward and post-processing: HIP events where the work is on the device, wall clock
where it is on the host.  The host leg uses the libraries the script uses (PIL.resize, numpy float64, F.interpolate on the CPU)
and its bytes are checked against the engine's before anything is timed.  class_map: pa_palette_argmin on a 512 x 683 picture, K =
150, against the evaluator's torch expression on the same GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from painter_amd import models_painter            # noqa: E402
from painter_amd import painter_engine as E       # noqa: E402

RES = 448
TASK = "ade20k_semseg"
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def picture(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // (w - 1), (yy * 255) // (h - 1), ((xx + yy) * 7) % 256], axis=-1)
    return np.clip(base // 2 + rng.integers(0, 128, (h // 8 + 1, w // 8 + 1, 3))[yy // 8, xx // 8], 0, 255).astype(np.uint8)


def sync():
    torch.cuda.synchronize()


class HostLeg:
    """What a user of the unchanged ADE20K script gets: per picture, batch 1, Pillow + numpy float64 before the forward and CPU torch
    float64 after it (file I/O left out).  Written with the same library calls as tests/painter_eval_host.py and its CPU test; the
    bytes are compared with the engine's before anything is timed."""

    def __init__(self, model, prompt, prompt_tgt):
        self.model = model
        self.prompt01, self.target01 = (self._unit(a) for a in (prompt, prompt_tgt))
        self.tokens = model.patch_embed.num_patches

    @staticmethod
    def _unit(pic):
        return np.asarray(Image.fromarray(pic).resize((RES, RES))) / 255.

    @staticmethod
    def _to_device(top01, bottom01):
        canvas = (np.concatenate((top01, bottom01), axis=0) - MEAN) / STD                  # float64 [2*RES][RES][3]
        return torch.from_numpy(canvas).permute(2, 0, 1)[None].float().to("cuda")

    @torch.no_grad()
    def one(self, pic, clock=None):
        stamps = [time.perf_counter()]
        h, w = pic.shape[:2]
        x = self._to_device(self.prompt01, self._unit(pic))
        t = self._to_device(self.target01, self.target01)
        masked = torch.zeros(1, self.tokens)
        masked[:, self.tokens // 2:] = 1
        valid = torch.ones(t.shape, dtype=torch.float64).float().to("cuda")               # the script builds it on the host, per picture
        masked = masked.to("cuda")
        if clock is not None:
            sync()
            stamps.append(time.perf_counter())
        y = self.model(x, t, masked, valid)[1]
        if clock is not None:
            sync()
            stamps.append(time.perf_counter())
        lower = self.model.unpatchify(y).permute(0, 2, 3, 1).cpu()[0, RES:]               # the whole canvas crosses PCIe, as float32
        shown = torch.clip((lower.double() * torch.from_numpy(STD) + torch.from_numpy(MEAN)) * 255, 0, 255)
        sized = F.interpolate(shown.permute(2, 0, 1)[None], size=(h, w), mode="bilinear")[0].permute(1, 2, 0)
        out = sized.to(torch.int32).numpy().astype(np.uint8)
        if clock is not None:
            stamps.append(time.perf_counter())
            for k, name in enumerate(("pre", "forward", "post")):
                clock[name] += stamps[k + 1] - stamps[k]
        return out

    def run(self, pictures):
        return [self.one(p) for p in pictures]

    def phases(self, pictures):
        clock = {"pre": 0.0, "forward": 0.0, "post": 0.0}
        for p in pictures:
            self.one(p, clock)
        return {k: v / len(pictures) * 1e3 for k, v in clock.items()}


class EngineLeg:
    def __init__(self, model, prompt, prompt_tgt, batch):
        self.eng = E.PainterEngine(model, "cuda", TASK, prompt, prompt_tgt, input_size=RES, batch_size=batch)
        self.batch = batch

    def run(self, pictures):
        return self.eng.run(pictures)

    @torch.no_grad()
    def phases(self, pictures):
        """PainterEngine._run_batch with an event at every phase boundary: device time per phase, plus the host's wall clock over
        the whole pass (the enqueue cost shows up as the difference)."""
        eng, io = self.eng, self.eng.io
        marks, n = [], 0
        sync()
        t0 = time.perf_counter()
        for i in range(0, len(pictures), self.batch):
            chunk = pictures[i:i + self.batch]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            queries = torch.stack([io.resize(io.upload(p), (RES, RES)) for p in chunk])
            plan = E.DecodePlan(TASK, [(p.shape[1], p.shape[0]) for p in chunk], eng.device)
            imgs, tgts = eng.stitch(queries)
            ev[1].record()
            y = E._forward(eng.model, imgs, tgts)
            ev[2].record()
            plan.launch(y, RES, RES, io.patch).pictures()
            ev[3].record()
            marks.append(ev)
            n += len(chunk)
        sync()
        wall = (time.perf_counter() - t0) / n * 1e3
        tot = [sum(ev[k].elapsed_time(ev[k + 1]) for ev in marks) / n for k in range(3)]
        return {"pre": tot[0], "forward": tot[1], "post": tot[2], "wall": wall}


def timed_run(leg, pictures):
    sync()
    t0 = time.perf_counter()
    outs = leg.run(pictures)
    sync()
    return len(pictures) / (time.perf_counter() - t0), outs


def class_map_bench(iters=20):
    rng = np.random.default_rng(3)
    sep = 256 // 6
    pal = np.array([(255 - (k // 36) * sep, 255 - ((k % 36) // 6) * sep, 255 - (k % 6) * sep) for k in range(150)], np.float32)
    pic = picture(5, 512, 683)
    pic[::2] = pal[rng.integers(0, 150, (256, 683))].astype(np.uint8)
    dpic, dpal = torch.from_numpy(pic).cuda(), torch.from_numpy(pal).cuda()
    out = torch.empty((512, 683), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        E.check(E.lib.pa_palette_argmin(dpic.data_ptr(), dpal.data_ptr(), out.data_ptr(), 512, 683, 150, 0, stream), "pa_palette_argmin")
        return out

    def evaluator():                                         # the evaluator's way ('abs'): a [H][W][K][3] float32 tensor, then argmin
        return (dpic.float()[:, :, None, :] - dpal[None, None]).abs().sum(-1).argmin(-1)

    same = bool((ours().long() == evaluator()).all())
    res = {"same_as_evaluator_expression": same}
    for name, fn in (("pa_palette_argmin_us", ours), ("evaluator_torch_gpu_us", evaluator)):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        sync()
        res[name] = round(s.elapsed_time(e) / iters * 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("painter_eval_bench: needs the MI355X (nothing here is measured on a CPU)")
    torch.manual_seed(0)
    model = models_painter.painter_vit_large_patch16_input896x448_win_dec64_8glb_sl1().to("cuda").eval()
    pictures = [picture(100 + i, 480, 640) for i in range(a.pictures)]
    prompt, prompt_tgt = picture(1, 375, 500), picture(2, 375, 500)
    legs = {"host_batch1": HostLeg(model, prompt, prompt_tgt)}
    for b in (int(v) for v in a.batches.split(",")):
        legs["engine_batch%d" % b] = EngineLeg(model, prompt, prompt_tgt, b)

    # same bytes first (this is also the warm-up of every shape the timed passes use)
    ref = legs["host_batch1"].run(pictures)
    same = {}
    for name, leg in legs.items():
        if name != "host_batch1":
            outs = leg.run(pictures)
            same[name] = sum(int(np.array_equal(x, y)) for x, y in zip(outs, ref))
    print("pictures identical to the host path's, of %d: %s" % (len(pictures), same), flush=True)

    rates = {k: [] for k in legs}
    phases = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, leg in legs.items():
            ips, _ = timed_run(leg, pictures)
            ph = leg.phases(pictures)
            rates[name].append(ips)
            phases[name].append(ph)
            print("round %d %-15s %8.1f images/s | ms/image %s" % (r, name, ips, " ".join("%s %.3f" % kv for kv in ph.items())), flush=True)
    summary = {"what": "Painter task inference end to end, ade20k_semseg settings, ViT-L random weights, 640x480 pictures in memory",
               "device": torch.cuda.get_device_name(0), "pictures": a.pictures, "rounds": a.rounds, "host_threads": torch.get_num_threads(),
               "identical_pictures": same, "legs": {}}
    for name in legs:
        summary["legs"][name] = {"images_per_s_median": round(statistics.median(rates[name]), 1),
                                 "images_per_s_all": [round(v, 1) for v in rates[name]],
                                 "ms_per_image_median": {k: round(statistics.median(p[k] for p in phases[name]), 3) for k in phases[name][0]}}
    summary["class_map_512x683_K150"] = class_map_bench()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
