"""Instance decode by nearest colour without a GPU: the host statement (tests/painter_minmax_host.py) against the fixture the unmodified
reference produced (tests/golden/painter_minmax.npz), the C ABI of include/painter_minmax.h as far as the host reaches it, and the
keyword handling of `post_type`."""
import os
import types

import numpy as np
import pytest

from tests import painter_minmax_cases as C
from tests import painter_minmax_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINMAX_HEADER = os.path.join(ROOT, "include", "painter_minmax.h")
SYMBOLS = {"pa_minmax_nearest", "pa_minmax_workspace_bytes", "pa_minmax_decode", "pa_minmax_masks"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_minmax.npz"))


@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_the_host_statement_equals_the_reference(golden, name):
    from painter_amd.painter_engine import location_palette
    assert np.array_equal(golden["palette"], location_palette())
    pic = C.fixture_picture(name)
    assert np.array_equal(pic, golden[name + ".picture"])
    got = H.decode(pic, H.with_background(golden["palette"]))
    assert np.array_equal(got["label"], golden[name + ".pred_map"]) and golden[name + ".pred_map"].dtype == np.uint16
    assert np.array_equal(got["dist"], golden[name + ".dist_map"]) and golden[name + ".dist_map"].dtype == np.uint16
    ref = golden[name + ".scores"]
    assert ref.dtype == np.float32 and got["scores"].dtype == np.float32 and got["scores"].tobytes() == ref.tobytes()
    assert np.array_equal(got["classes"], golden[name + ".classes"])
    assert got["ties"] == int(golden[name + ".ties"]) and int(got["S"].max()) == int(golden[name + ".largest_sum"]) < 1 << 24
    assert np.array_equal(got["candidates"], np.unique(golden[name + ".pred_map"])) and got["count"] == len(ref)
    assert int(got["n"].sum()) == pic.shape[0] * pic.shape[1] and int(got["S"].sum()) == int(got["dist"].sum())


def test_the_fixture_holds_the_cases_the_route_needs(golden):
    assert {"thr19_a", "thr19_c", "few"} <= set(C.FIXTURE)
    assert any(int(golden[n + ".ties"]) > 0 for n in C.FIXTURE)
    assert golden["thr19_c.picture"].shape == (61, 83, 3) and len(golden["thr19_a.scores"]) == 683
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "painter_minmax.npz")) < 1000000


def test_the_statement_on_constructed_pictures():
    pic, pal = C.ties_case()
    got = H.decode(pic, pal)
    assert got["label"][:5, 0].tolist() == [1, 1, 1, 1, 0] and got["label"][5].tolist() == [2] * 4 + [4] * 4 and got["ties"] >= 8 * 5
    assert 3 not in got["candidates"] and got["slot"][3] == -1                    # the duplicated row never wins
    assert got["dist"][1, 0] == 60 and got["dist"][4, 0] == 115 and got["dist"][5, 0] == 135
    black = H.decode(np.zeros((5, 7, 3), np.uint8), H.with_background([[9, 9, 9]]))
    assert black["count"] == 1 and black["classes"].tolist() == [0] and black["records"]["neg"][0] == 0 and black["scores"][0] == 1.0
    pal = H.with_background(np.arange(60).reshape(20, 3) * 4)
    exact = H.decode(C.exact_colours_case(pal), pal)
    assert exact["count"] == 7 and (exact["scores"] == 1.0).all() and not exact["dist"].any()
    masks = H.masks_of(exact["label"], exact["slot"])
    assert masks.shape[0] == 7 and (masks.sum(0) == 1).all()                     # the masks partition the picture
    assert np.array_equal(H.masks_of(exact["label"], exact["slot"], 2, 3), masks[2:5])
    bits = H.pack_bits(masks.reshape(7, -1))
    assert bits.dtype == np.uint32 and bits.shape == (7, 30) and int(bits[0, 0]) & 1 == int(masks[0, 0, 0])
    label, dist, ties = H.constant_nearest((255, 255, 255), 3, 4, H.with_background([[0, 0, 1]]))
    assert label.tolist() == [[0] * 4] * 3 and dist[0, 0] == 764 and ties == 0


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd import _lib, build
    from painter_amd._lib import lib, parse_header
    from tests.guard_bands import abi_symbols
    protos = parse_header(MINMAX_HEADER)
    assert set(protos) == SYMBOLS == abi_symbols(open(MINMAX_HEADER).read())
    for name in SYMBOLS:
        assert getattr(lib, name) is not None                  # the built library exports them, the binding resolves them
    assert MINMAX_HEADER in [os.path.abspath(p) for p in _lib.MORE_HEADERS]
    assert not set(parse_header()) & SYMBOLS and not any(s.startswith("pa_minmax") for s in parse_header())          # the main header is as it was
    assert MINMAX_HEADER in build.headers() and build.EXTRA["painter_minmax.hip"] == ["-ffp-contract=off"]
    assert len(protos["pa_minmax_nearest"][1]) == 8 and len(protos["pa_minmax_decode"][1]) == 12 and len(protos["pa_minmax_masks"][1]) == 10
    assert lib.pa_abi_version() == 9


def test_the_record_layout_matches_the_header():
    from painter_amd import painter_engine as E
    assert E.MINMAX_RECORD == H.RECORD and E.MINMAX_RECORD.itemsize == 32
    assert [E.MINMAX_RECORD.fields[k][1] for k in ("colour", "cls", "n", "reserved", "S", "neg", "score")] == [0, 4, 8, 12, 16, 24, 28]
    assert E.MINMAX_DEFAULTS == dict(palette=None) and E.POST_TYPES == ("threshold", "minmax")


def test_size_helper():
    from painter_amd._lib import lib
    up16 = lambda x: -(-x // 16) * 16
    for h, w, k in ((1, 1, 1), (480, 640, 6401), (61, 83, 2), (16384, 1024, 16384), (4096, 4096, 5)):
        assert lib.pa_minmax_workspace_bytes(h, w, k) == up16(8 * k) + up16(4 * k), (h, w, k)
    for bad in ((0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, 5, 0), (5, 5, -2), (5, 5, 16385), (16385, 1, 3), (1, 16385, 3), (4097, 4096, 3),
                (16384, 1025, 3)):
        assert lib.pa_minmax_workspace_bytes(*bad) == -1, bad


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """hipErrorInvalidValue (1): no pointer is touched, so this needs no GPU."""
    from painter_amd._lib import lib
    a = 256
    ok = dict(image=a, palette=a, h=5, w=7, k=3, label=a, dist=a)
    near = lambda **kw: lib.pa_minmax_nearest(*dict(ok, **kw).values(), None)
    for bad in (dict(image=None), dict(palette=None), dict(label=None), dict(dist=None), dict(h=0), dict(w=0), dict(k=0), dict(k=16385),
                dict(h=16385), dict(h=8192, w=4096), dict(palette=a + 2), dict(label=a + 1), dict(dist=a + 1)):
        assert near(**bad) == 1, bad
    ok = dict(image=a, palette=a, h=5, w=7, k=3, ws=a, label=a, dist=a, count=a, records=a, slot=a)
    dec = lambda **kw: lib.pa_minmax_decode(*dict(ok, **kw).values(), None)
    for bad in (dict(image=None), dict(palette=None), dict(ws=None), dict(label=None), dict(dist=None), dict(count=None), dict(records=None),
                dict(slot=None), dict(h=0), dict(w=-1), dict(k=0), dict(k=16385), dict(w=16385), dict(h=4097, w=4096), dict(ws=a + 8),
                dict(records=a + 4), dict(count=a + 2), dict(slot=a + 2), dict(label=a + 1)):
        assert dec(**bad) == 1, bad
    ok = dict(label=a, slot=a, h=5, w=7, k=3, first=0, n_cap=2, bits=a, bytes=a)
    msk = lambda **kw: lib.pa_minmax_masks(*dict(ok, **kw).values(), None)
    for bad in (dict(label=None), dict(slot=None), dict(bits=None), dict(h=0), dict(w=0), dict(k=0), dict(k=16385), dict(first=-1), dict(n_cap=0),
                dict(n_cap=16385), dict(bits=a + 2), dict(slot=a + 2), dict(label=a + 1), dict(h=4097, w=4096)):
        assert msk(**bad) == 1, bad


def never(*a, **k):
    raise AssertionError("a forward was enqueued")


def test_post_type_keywords_are_refused_before_anything_is_enqueued():
    from painter_amd import painter_engine as E
    pictures = [np.zeros((4, 4, 3), np.uint8)]
    inst = types.SimpleNamespace(task="coco_pano_inst", _run=never, _launch_batch=never, batch_size=2, model=None)
    sem = types.SimpleNamespace(task="coco_pano_semseg", _run=never, _launch_batch=never, batch_size=2, model=None)
    for key, value in E.INSTANCE_DEFAULTS.items():
        if key == "palette":
            continue
        with pytest.raises(TypeError, match=key):
            E.PainterEngine.run_instances(inst, pictures, post_type="minmax", **{key: value})
        with pytest.raises(TypeError, match=key):
            E.run_instance_results(inst, pictures, [1], post_type="minmax", **{key: value})
    with pytest.raises(TypeError, match="nms_iou"):
        E.PainterEngine.run_instances(inst, pictures, post_type="minmax", nms_iou=0.5)
    with pytest.raises(TypeError, match="n_things"):
        E.run_instance_results(inst, pictures, [1], post_type="minmax", n_things=80)
    for post_type in ("topk", None, "MINMAX"):
        with pytest.raises(NotImplementedError):
            E.PainterEngine.run_instances(inst, pictures, post_type=post_type)
        with pytest.raises(NotImplementedError):
            E.run_instance_results(inst, pictures, [1], post_type=post_type)
    with pytest.raises(ValueError, match="semseg_engine"):
        E.run_instance_results(inst, pictures, [1], semseg_engine=sem, post_type="minmax")
    # the threshold route's own refusals are as they were, with and without the keyword
    for kw in (dict(), dict(post_type="threshold")):
        with pytest.raises(TypeError, match="nms_iou"):
            E.PainterEngine.run_instances(inst, pictures, nms_iou=0.5, **kw)
        with pytest.raises(NotImplementedError, match="cubic"):
            E.PainterEngine.run_instances(inst, pictures, kernel="cubic", **kw)
        with pytest.raises(TypeError, match="nms_iou"):
            E.run_instance_results(inst, pictures, [1], nms_iou=0.5, **kw)
    with pytest.raises(ValueError, match="coco_pano_inst"):
        E.PainterEngine.run_instances(sem, pictures, post_type="minmax")


def test_minmax_refuses_a_cpu_device_and_a_bad_palette():
    import torch
    from painter_amd import painter_engine as E
    pic = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.instances_minmax(pic, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.instances_minmax(torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(TypeError, match="MinmaxDecode"):
        E.instance_results(object(), 1)
