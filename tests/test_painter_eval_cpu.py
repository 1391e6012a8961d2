"""CPU side of the Painter task-inference path: tests/painter_eval_host.py (what the GPU tests compare the device with) is pinned
against live CPU torch, against the digests the unmodified scripts produced (tests/golden/painter_eval_io.npz) and, where a reference
checkout is present, against the live scripts; painter_engine.TASKS against the scripts' own settings; the C ABI against the header.

If another host CPU made torch pick a different bilinear kernel, the live-torch leg could differ there; the fixture is the authority
(the GPU tests never call F.interpolate)."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import painter_eval_cases as C
from tests import painter_eval_host as H

BICUBIC_GATE = 1e-11          # x max(1, max |ref|): 31 float64 operations and a source coordinate whose fused / unfused forms differ by
                              # <= 448 * 2^-53 ~ 5e-14 times a weight slope <= 1.5 per axis; the restatement measures ~2.6e-13


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_eval_io.npz"))


def _torch_resize(pic, h, w, mode):
    return F.interpolate(torch.from_numpy(pic)[None].permute(0, 3, 1, 2), size=[h, w], mode=mode).permute(0, 2, 3, 1)[0]


def test_fma_emulation_is_correctly_rounded():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)
    b = rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)
    c = -(a * b) + rng.standard_normal(4000) * 10.0 ** rng.integers(-20, 2, 4000)         # heavy cancellation
    # ties of the unfused sum: a * b = 1 + 2^-52 + 2^-104 exactly, c = 2^-53 -> the fused result rounds up, double rounding does not
    a = np.concatenate([a, [1.0 + 2.0 ** -52, 3.0, 448 / 480]])
    b = np.concatenate([b, [1.0 + 2.0 ** -52, 1.0 / 3.0, 17.5]])
    c = np.concatenate([c, [2.0 ** -53, -1.0, -0.5]])
    got = H.fma(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert got[i] == float(exact), (i, a[i], b[i], c[i])                               # float(Fraction) rounds to nearest even


@pytest.mark.parametrize("h,w", C.SIZES)
def test_host_resizes_match_live_torch(h, w):
    for scale, seed in ((255.0, 1), (10000.0, 2)):
        y = H.lower_half(C.tokens(seed * 100 + h % 97)[0], C.RES, C.RES, C.PATCH).astype(np.float64) * H.STD + H.MEAN
        pic = np.clip(y * scale, 0, scale)
        assert 0.5 < float(((pic == 0) | (pic == scale)).mean()) < 0.9          # mostly saturated, as the issue's cases
        ref = _torch_resize(pic, h, w, "bilinear")
        assert np.array_equal(H.bilinear(pic, h, w), ref.numpy())
        assert np.array_equal(H.channel_mean(ref.numpy()), ref.mean(-1).numpy())
        assert np.array_equal(H.nearest(pic, h, w), _torch_resize(pic, h, w, "nearest").numpy())
        ref = _torch_resize(y, h, w, "bicubic").numpy()
        got = H.bicubic(y, h, w)
        assert np.abs(got - ref).max() <= BICUBIC_GATE * max(1.0, np.abs(ref).max())
        assert np.array_equal(H.saved_picture(got), H.saved_picture(ref))


def _host_run(task, i):
    """The helper's restatement of one fixture case -> (x, tgt float32 model inputs, output)."""
    prompt, prompt_tgt = C.prompt_pair()
    s, h, w = C.QUERIES[task][i]
    img, tgt = H.canvases(prompt, prompt_tgt, C.picture(s, h, w), C.RES)
    x, t = H.model_inputs(img, tgt)
    y = C.standin_tokens(torch.from_numpy(x), torch.from_numpy(t)).numpy()
    return x, t, H.decode(task, y[0], C.out_size(task, h, w), C.RES, C.RES, C.PATCH)


def _check_against_fixture(golden, task, i, x, t, out, masked=None):
    key = "%s.%d." % (task, i)
    assert C.digest(x) == str(golden[key + "x_digest"]) and C.digest(t) == str(golden[key + "tgt_digest"])
    if masked is not None:
        assert masked == int(golden[key + "masked"])
    assert int(golden[key + "masked"]) == C.L // 2
    assert tuple(golden[key + "out_shape"]) == out.shape and str(golden[key + "out_dtype"]) == str(out.dtype)
    if out.dtype == np.float64:
        ref = golden[key + "out_sample"]
        assert np.abs(out[::C.SAMPLE_STRIDE, ::C.SAMPLE_STRIDE] - ref).max() <= BICUBIC_GATE * max(1.0, np.abs(ref).max())
    else:
        assert C.digest(out) == str(golden[key + "out_digest"])


@pytest.mark.parametrize("task", list(H.SCRIPTS))
def test_host_restatement_matches_the_unmodified_scripts(golden, task):
    for i in range(len(C.QUERIES[task])):
        x, t, out = _host_run(task, i)
        _check_against_fixture(golden, task, i, x, t, out)
        if out.dtype == np.float64:
            assert C.digest(H.saved_picture(out)) == str(golden["%s.%d.saved_digest" % (task, i)])


def test_fixture_covers_the_interesting_values(golden):
    """480 x 640 and a down-scale are in; the stand-in's pictures saturate at both ends."""
    for task in H.SCRIPTS:
        shapes = [tuple(golden["%s.%d.out_shape" % (task, i)][:2]) for i in range(len(C.QUERIES[task]))]
        assert (480, 640) in shapes or task == "sidd"
        assert any(h < C.RES or w < C.RES for h, w in shapes)
    s = golden["ade20k_semseg.0.out_sample"]
    assert (s == 0).any() and (s == 255).any() and ((s > 0) & (s < 255)).any()
    d = golden["nyuv2_depth.0.out_sample"]
    assert d.dtype == np.int32 and (d == 0).any() and (d == 10000).any()


def test_tasks_table_matches_the_scripts_settings(golden):
    from painter_amd.painter_engine import TASKS
    assert list(TASKS) == list(H.SCRIPTS)
    for task, spec in TASKS.items():
        mode, scale, clip, kind = (str(v) for v in golden[task + ".settings"])
        assert (spec["resize"], repr(spec["scale"]), repr(spec["clip"]), spec["kind"]) == (mode, scale, clip, kind)
        assert H.SCRIPTS[task][1:] == (spec["resize"], spec["scale"], spec["clip"], spec["kind"])


def test_palette_is_the_ade20k_colour_list(golden):
    pal = golden["palette"]
    assert pal.shape == (150, 3) and pal.min() >= 0 and pal.max() == 255 and len({tuple(c) for c in pal}) == 150
    assert tuple(pal[0]) == (255, 255, 255)


def test_class_map_host_first_minimum():
    pal = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [5, 5, 0]], np.float32)
    pic = np.array([[[5, 0, 0], [5, 5, 0], [0, 5, 0], [9, 9, 9]]], np.uint8)
    assert H.class_map(pic, pal, "abs").tolist() == [[0, 3, 0, 3]]


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_painter_stitch", "pa_painter_decode_u8", "pa_painter_decode_depth", "pa_painter_decode_f64", "pa_palette_argmin"):
        assert name in protos
        assert getattr(lib, name) is not None
    assert lib.pa_abi_version() == 9


def test_engine_refuses_a_cpu_device():
    from painter_amd import painter_engine as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.PainterEngine(C.StandInModel(), "cpu", "ade20k_semseg", *C.prompt_pair())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.class_map(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.float32), device="cpu")
    with pytest.raises(KeyError):
        E.decode("no_such_task", torch.zeros(1), [(1, 1)], 448, 448, 16)


# ---- with a reference checkout: the live scripts
def _reference():
    from oracle import ref_import
    return os.path.isdir(os.path.join(ref_import.PAINTER_DIR, "eval", "ade20k_semantic"))


@pytest.mark.skipif(not _reference(), reason="needs the reference's Painter/eval scripts")
@pytest.mark.parametrize("task", list(H.SCRIPTS))
def test_live_scripts_match_helper_and_fixture(golden, task, tmp_path):
    from tests.golden import make_golden_painter_eval_io as G
    assert G.script_settings(task) == H.SCRIPTS[task][1:]
    for i, r in enumerate(G.run_task(task, str(tmp_path))):
        x, t, out = _host_run(task, i)
        assert (C.digest(x), C.digest(t)) == (r["x"], r["tgt"])
        if out.dtype == np.float64:
            assert np.abs(out - r["out"]).max() <= BICUBIC_GATE * max(1.0, np.abs(r["out"]).max())
            assert np.array_equal(H.saved_picture(out), H.saved_picture(r["out"]))
            assert np.array_equal(r["out"][::C.SAMPLE_STRIDE, ::C.SAMPLE_STRIDE], golden["%s.%d.out_sample" % (task, i)])
        else:
            assert np.array_equal(out, r["out"])
            assert C.digest(r["out"]) == str(golden["%s.%d.out_digest" % (task, i)])


@pytest.mark.skipif(not _reference(), reason="needs the reference's Painter/eval scripts")
def test_live_palette_matches_fixture(golden):
    from tests.golden import make_golden_painter_eval_io as G
    assert np.array_equal(G.load_palette(), golden["palette"])
