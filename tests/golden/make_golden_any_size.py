"""Generate the any-input-size fixtures: the UNMODIFIED reference, built at one size and run at another, on the CPU in fp32.

Run in the build container only (needs the reference tree; seconds):

    python tests/golden/make_golden_any_size.py

The reference resizes the position grid bicubically (get_abs_pos) and every block's rel-pos tables linearly (get_rel_pos,
util/vitdet_utils.py:63-93) whenever the token grid of the run differs from the constructed one; nothing here touches it.  Cases,
parameters and inputs: tests/any_size_cases.py (seeds only; the parameters are oracle.painter_oracle.random_params of the BUILT
configuration, whose rel-pos tables are drawn non-zero -- the reference initialises them to zero, which would hide the bias).

Per case `X/`: loss (float64), pred (the full patchified prediction, float32), bf16_dev = the relative Frobenius deviation of the
reference's own pred under torch.autocast(bfloat16) from its fp32 pred (the bf16 build's yardstick), zero_tables_move = how far zeroing
the tables moves pred (asserted > 10 x the fp32 gate: a wrong bias is visible).  The reference's bf16-autocast pred itself goes to
painter_any_size_bf16.npz as bfloat16 bit patterns (uint16).  Three files, because no committed file may exceed 1 MiB:
painter_any_size.npz (A, B, C), painter_any_size_df.npz (D, F), painter_any_size_bf16.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import any_size_cases as C              # noqa: E402
from tests import golden_util as G                 # noqa: E402
from tests.golden import make_golden as MG         # noqa: E402


def run(model, cfg, name, autocast=False):
    imgs, tgts, mask, valid = C.inputs(name)
    Hp, Wp = C.run_config(name).grid
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        loss, pred, _ = model(imgs, tgts, bool_masked_pos=mask.reshape(C.BATCH, Hp, Wp), valid=valid)
    return float(loss), pred.detach().float()


def main():
    torch.set_num_threads(os.cpu_count())
    files, bf16 = {}, {}
    for name, (_, seed_p, _, size, fname) in C.CASES.items():
        cfg = C.config(name)
        model, _ = MG.build_reference(cfg, seed_p)
        model.eval()
        assert tuple(cfg.img_size) != tuple(size)
        loss, pred = run(model, cfg, name)
        _, pred_b = run(model, cfg, name, autocast=True)
        dev = G.rel_fro(pred_b, pred)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("rel_pos_h") or n.endswith("rel_pos_w"):
                    p.zero_()
        _, pred_z = run(model, cfg, name)
        moved = G.rel_err(pred_z, pred)
        assert moved > 10 * C.FP32_GATE, (name, moved)
        out = files.setdefault(fname, {})
        out[name + "/loss"] = np.float64(loss)
        out[name + "/pred"] = pred.numpy()
        out[name + "/bf16_dev"] = np.float64(dev)
        out[name + "/zero_tables_move"] = np.float64(moved)
        out[name + "/size"] = np.array(size, np.int64)
        bf16[name + "/pred_bf16_bits"] = pred_b.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        print("case %s at %s: loss %.6f, bf16 autocast deviation %.3e, zeroed tables move pred by %.3e" % (name, size, loss, dev, moved))
    files[C.BF16_FILE] = bf16
    for fname, out in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < (1 << 20), (fname, os.path.getsize(path))
        print("%s: %.0f KB" % (fname, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
