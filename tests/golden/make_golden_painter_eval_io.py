"""Generate tests/golden/painter_eval_io.npz by running the UNMODIFIED reference code on CPU: the `run_one_image` function of each of
the eight task scripts Painter/eval/*/painter_inference_*.py, `util/ddp_utils.DatasetTest` for the query side, and the colour list of
data/ade20k/gen_color_ade20k_sem.py.

Needs a reference checkout (oracle/ref_import.REFERENCE_ROOT):   python tests/golden/make_golden_painter_eval_io.py

The scripts guard their main body (`if __name__ == '__main__'`), so importing them defines their functions and nothing else; the
packages they import at the top and that may be absent (matplotlib, tqdm, requests, skimage, cv2; timm / detectron2 / fvcore /
fairscale through models_painter) are empty stand-in modules: run_one_image touches none of them.  The network is
tests/painter_eval_cases.StandInModel (a fixed float32 function of both canvases), the pictures are the seeded ones of
tests/painter_eval_cases.py, written as PNG files.  The scripts' main bodies need CUDA, DDP and the datasets; their prompt / canvas
step is done here with Pillow and numpy directly (`build_canvases`), not through tests/painter_eval_host.py.

The fixture stores SHA-256 digests of what each script handed the model and of the file / array it produced, [::11, ::11] samples of
the float64 outputs, small samples of the pictures for debugging, each script's settings as its source states them, and the palette.
"""
import importlib.util
import os
import re
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import                         # noqa: E402
from tests import painter_eval_cases as C             # noqa: E402
from tests import painter_eval_host as H              # noqa: E402  (only the table of script paths)

MEAN, STD = C.MEAN, C.STD                             # the ImageNet statistics every script normalises with


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except ImportError:
        pass
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    if "." in name:
        setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], m)


def install_script_stubs():
    ref_import.install_stubs()
    for name in ("matplotlib", "matplotlib.pyplot", "tqdm", "requests", "cv2", "skimage"):
        _stub(name)
    _stub("skimage.metrics", peak_signal_noise_ratio=None, structural_similarity=None)


def load_script(task):
    """-> the module object of the task's unmodified script (main body not run)."""
    install_script_stubs()
    path = os.path.join(ref_import.PAINTER_DIR, "eval", H.SCRIPTS[task][0])
    saved = list(sys.path)
    try:
        mod = ref_import._load("ref_painter_inference_" + task, path, ref_import.PAINTER_DIR)
    finally:
        sys.path[:] = saved                            # the scripts append '.' to sys.path
    sys.modules.pop("models_painter", None)            # the script's `import models_painter`: keep it private to the script
    return mod


def load_dataset_test():
    """-> util/ddp_utils.DatasetTest of the reference (through a script that imports it)."""
    return load_script("ade20k_semseg").DatasetTest


def load_palette():
    path = os.path.join(ref_import.PAINTER_DIR, "data", "ade20k", "gen_color_ade20k_sem.py")
    install_script_stubs()
    spec = importlib.util.spec_from_file_location("ref_gen_color_ade20k_sem", path)
    mod = importlib.util.module_from_spec(spec)
    saved = list(sys.path)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved
    return np.array(mod.PALETTE, dtype=np.int32)


def script_settings(task):
    """(resize mode, scale, clip, output kind) read off the script's own run_one_image source."""
    src = open(os.path.join(ref_import.PAINTER_DIR, "eval", H.SCRIPTS[task][0])).read()
    body = src[src.index("def run_one_image"):]
    body = body[:re.search(r"\n(?=\S)", body).start()]
    mode = re.search(r"mode='(\w+)'", body).group(1)
    clip = re.search(r"torch\.clip\(\(output \* imagenet_std \+ imagenet_mean\) \* (\d+), 0, (\d+)\)", body)
    scale = float(clip.group(1)) if clip else 1.0
    kind = "depth" if "mean(-1).int()" in body else ("u8" if "output.int()" in body else "f64")
    return mode, scale, bool(clip), kind


def _normalised(top, bottom):
    """Two [res][res][3] pictures in [0, 1] stacked along the height, then (v - mean) / std with numpy float64 broadcasting."""
    canvas = np.concatenate((top, bottom), axis=0)
    return (canvas - MEAN) / STD


def build_canvases(prompt, prompt_target, query01, res):
    """What a script's main body hands to run_one_image (the main bodies sit under `__main__` and cannot be imported): the prompt pair
    goes through Pillow's default `resize` and `/ 255.`, the query arrives from DatasetTest already in [0, 1]; the image canvas is
    [prompt ; query], the target canvas shows the prompt's target in both halves.  Written with Pillow and numpy directly, not through
    tests/painter_eval_host.py, so that the helper is checked against something it did not produce."""
    unit = [np.array(Image.fromarray(a).resize((res, res))) / 255. for a in (prompt, prompt_target)]
    assert all(u.shape == (res, res, 3) for u in unit) and query01.shape == (res, res, 3)
    return _normalised(unit[0], query01), _normalised(unit[1], unit[1])


def run_task(task, tmp):
    """-> [dict(x, tgt, masked, out, ...)] per query: the unmodified run_one_image of the task's script over the stand-in network."""
    mod = load_script(task)
    DatasetTest = load_dataset_test()
    p_img, p_tgt = C.prompt_pair()
    qdir = os.path.join(tmp, task)
    os.makedirs(qdir)
    for i, q in enumerate(C.query_pictures(task)):
        Image.fromarray(q).save(os.path.join(qdir, "q%d.png" % i))
    ds = DatasetTest(qdir, C.RES, ext_list=('*.png',))
    items = sorted((ds[i] for i in range(len(ds))), key=lambda it: it[1])
    assert len(items) == len(C.QUERIES[task])
    kind = script_settings(task)[3]
    uses_module = "model.module" in open(os.path.join(ref_import.PAINTER_DIR, "eval", H.SCRIPTS[task][0])).read()
    results = []
    for i, (img, img_path, size_org) in enumerate(items):
        s, h, w = C.QUERIES[task][i]
        assert size_org == (w, h)
        size = C.out_size(task, h, w)
        img, tgt = build_canvases(p_img, p_tgt, img, C.RES)
        net = C.StandInModel()
        model = C.Wrapped(net) if uses_module else net
        out_path = os.path.join(qdir, "out%d.png" % i)
        ret = mod.run_one_image(img, tgt, size, model, out_path, "cpu")
        assert len(net.calls) == 1
        call = net.calls[0]
        assert call["batch"] == 1 and call["valid_ok"] and call["second_half"] and call["mask_shape"] == (1, C.L), call
        if kind == "f64":
            assert ret.dtype == np.float64 and ret.shape == (size[1], size[0], 3)
            out = ret
        else:
            assert ret is None
            out = np.array(Image.open(out_path))
            if kind == "depth":                        # Pillow writes the int32 ('I') picture as a 16-bit PNG: same values
                assert out.dtype == np.uint16
                out = out.astype(np.int32)
        results.append(dict(x=call["x"], tgt=call["tgt"], masked=call["masked"], out=out, query_digest=C.digest(img[C.RES:])))
    return results


def save_npz(path, arrays):
    """np.savez_compressed with fixed member order and time stamps: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[k]), allow_pickle=False)


def main():
    out = {"palette": load_palette()}
    with tempfile.TemporaryDirectory() as tmp:
        for task in H.SCRIPTS:
            mode, scale, clip, kind = script_settings(task)
            out[task + ".settings"] = np.array([mode, repr(scale), repr(clip), kind])
            for i, r in enumerate(run_task(task, tmp)):
                key = "%s.%d." % (task, i)
                out[key + "x_digest"], out[key + "tgt_digest"], out[key + "masked"] = r["x"], r["tgt"], r["masked"]
                out[key + "query_digest"] = r["query_digest"]
                o = r["out"]
                out[key + "out_shape"] = np.array(o.shape)
                out[key + "out_dtype"] = str(o.dtype)
                if kind == "f64":
                    out[key + "out_sample"] = o[::C.SAMPLE_STRIDE, ::C.SAMPLE_STRIDE]
                    out[key + "saved_digest"] = C.digest((np.clip(o, 0, 1) * 255).astype(np.uint8))
                else:
                    out[key + "out_digest"] = C.digest(o)
                    out[key + "out_sample"] = o[::29, ::29]
    path = os.path.join(HERE, "painter_eval_io.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if "digest" in k:
            print(" ", k, str(out[k])[:16])


if __name__ == "__main__":
    main()
