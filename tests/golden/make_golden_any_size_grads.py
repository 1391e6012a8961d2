"""Generate the any-input-size GRADIENT fixtures: the UNMODIFIED reference, built at one size and run at another, loss.backward() with imgs
and tgts as leaves, on the CPU in fp32.

Run in the build container only (needs the reference tree; seconds):

    python tests/golden/make_golden_any_size_grads.py

Under autograd the reference's get_abs_pos (bicubic) and get_rel_pos (F.interpolate(mode="linear"), util/vitdet_utils.py:63-93) carry the
gradients back into the stored pos_embed and rel-pos tables; nothing here touches the reference.  Cases, parameters and inputs are those
of the forward fixtures (tests/any_size_cases.py: A, B, C, D, F; seeds only).

Per case X two files, because no committed file may exceed 1 MiB:
  painter_any_size_grads_X.npz        loss (float64); make_golden.py's gradient digests of every parameter (grad_digest: norm, sum, probe
                                      dot; tensors of up to 4096 elements in full as grad/<name>, every 997th element of the larger
                                      ones), which hold every rel-pos table gradient in full (grad/ or grad_full/<name>); dtgts in full
  painter_any_size_grads_X_dimgs.npz  dimgs in full
The generator asserts that pos_embed and every rel-pos table get a non-zero gradient."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import any_size_cases as C                          # noqa: E402
from tests.golden import make_golden as MG                     # noqa: E402

FILE = "painter_any_size_grads_%s.npz"
FILE_DIMGS = "painter_any_size_grads_%s_dimgs.npz"


def main():
    torch.set_num_threads(os.cpu_count())
    for name, (_, seed_p, _, size, _) in C.CASES.items():
        cfg = C.config(name)
        assert tuple(cfg.img_size) != tuple(size)
        model, _ = MG.build_reference(cfg, seed_p)
        model.eval()
        imgs, tgts, mask, valid = C.inputs(name)
        xi, xt = imgs.clone().requires_grad_(True), tgts.clone().requires_grad_(True)
        loss, _, _ = model(xi, xt, bool_masked_pos=mask.reshape(C.BATCH, *C.run_config(name).grid), valid=valid.clone())
        loss.backward()
        out = {"loss": np.float64(loss.item()), "size": np.array(size, np.int64), "dtgts": xt.grad.numpy()}
        MG.grad_digest([(n, p.grad) for n, p in model.named_parameters()], out, "")
        for n, p in model.named_parameters():
            if n.endswith("rel_pos_h") or n.endswith("rel_pos_w") or n == "pos_embed":
                assert float(p.grad.abs().max()) > 0, (name, n)
            if n.endswith("rel_pos_h") or n.endswith("rel_pos_w"):       # in full, whatever its size
                assert ("grad/" + n in out) != ("grad_full/" + n in out), n
        for fname, data in ((FILE % name, out), (FILE_DIMGS % name, {"dimgs": xi.grad.numpy()})):
            path = os.path.join(HERE, fname)
            np.savez_compressed(path, **data)
            assert os.path.getsize(path) < (1 << 20), (fname, os.path.getsize(path))
            print("%s: %.0f KB" % (fname, os.path.getsize(path) / 1024))
        print("case %s at %s: loss %.6f, |d pos_embed| %.3e" % (name, size, loss.item(), float(dict(model.named_parameters())["pos_embed"].grad.norm())))


if __name__ == "__main__":
    main()
