"""Generate tests/golden/painter_restore.npz over the cases of tests/painter_restore_cases.py.

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_restore.py

The one piece of the UNMODIFIED reference's restoration scoring that can run here is `myPSNR` of Painter/eval/lol/painter_inference_lol.py
(:73-77); skimage and MATLAB are absent.  The script module guards its main body and is loaded with the stand-in modules of
tests/golden/make_golden_painter_eval_io.load_script (skimage.metrics among them).

Stored per case, no pictures (the cases are seeded):
  <case>.myPSNR                 float64: the REFERENCE's number, myPSNR(gt / 255., prediction) -- skimage cases only
  <case>.<metric>.sums          float64 [8]: the HOST STATEMENT's record (tests/painter_restore_host.sums, route "direct"), not the reference's
  <case>.<metric>.psnr, .ssim   float64: the HOST STATEMENT's scores, not the reference's
  <case>.<metric>.ssim_scipy    float64: the statement's SSIM by its scipy route
  <case>.clipped                int64 [2]: prediction elements below 0 and above 1
A case enters the fixture only after this script has ASSERTED that the statement's PSNR equals myPSNR's within 1e-12 relative (inf for
inf) and that its two window routes agree within 1e-12; over the set: a prediction clipped at both ends, a perfect one, a near-constant
pair and a Y case with tie colours."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import painter_restore_cases as C                                     # noqa: E402
from tests import painter_restore_host as H                                      # noqa: E402
from tests.golden.make_golden_painter_eval_io import load_script, save_npz       # noqa: E402


def main():
    my_psnr = load_script("lol").myPSNR
    out, kinds = {}, set()
    for name, (kind, seed, h, w, metrics) in C.FIXTURE.items():
        pred, gt = C.fixture_case(name)
        out[name + ".clipped"] = np.array([(pred < 0).sum(), (pred > 1).sum()], np.int64)
        for metric in metrics:
            p, g = C.inputs(pred, gt, metric)
            sums = H.sums(p, g, metric)
            psnr, ssim = (float(v) for v in H.metrics(sums, metric))
            ssim_scipy = H.scores(p, g, metric, route="scipy")[1]
            assert abs(ssim - ssim_scipy) <= 1e-12, (name, metric, ssim, ssim_scipy)
            if metric == "skimage":
                with np.errstate(divide="ignore"):
                    ref = float(my_psnr(gt / 255., pred))
                assert ref == psnr if np.isinf(ref) else abs(psnr - ref) <= 1e-12 * abs(ref), (name, psnr, ref)
                out[name + ".myPSNR"] = np.float64(ref)
            key = "%s.%s." % (name, metric)
            out[key + "sums"], out[key + "psnr"], out[key + "ssim"], out[key + "ssim_scipy"] = sums, np.float64(psnr), np.float64(ssim), \
                np.float64(ssim_scipy)
            print(name, metric, "psnr", psnr, "ssim", ssim, "routes differ by", abs(ssim - ssim_scipy), "clipped", out[name + ".clipped"])
        kinds.add(kind)
    assert {"natural", "perfect", "near_constant", "ties"} <= kinds
    assert any(out[n + ".clipped"].min() > 0 for n in C.FIXTURE)
    path = os.path.join(HERE, "painter_restore.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100000


if __name__ == "__main__":
    main()
