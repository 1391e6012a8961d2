"""CPU side of the class-agnostic instance decode: tests/painter_inst_host.py (the definition the GPU tests hold the device to) is
pinned against what the unmodified reference produced (tests/golden/painter_inst.npz) and, where a reference checkout is present,
against the live reference; `location_palette` against the reference's colour rule; the C ABI against the header.

The bars: masks and their order equal; scores within 2 x the deviation the reference's float32 arithmetic showed from the host statement
when the fixture was made (the reference is the only inexact side here)."""
import os

import numpy as np
import pytest

from tests import painter_inst_cases as C
from tests import painter_inst_host as H


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_inst.npz"))


def test_fixture_holds_the_required_cases(golden):
    names = list(C.FIXTURE)
    thr = {n: [float(t) for t in golden[n + ".thresholds"]] for n in names}
    assert sum(1 for n in names if thr[n] == [19.0]) >= 3 and any(t == [10.0, 19.0] for t in thr.values())
    assert int(golden["many.live"]) > 2000 > int(golden["few.live"]) and thr["few"] == [5.0]
    assert any(golden[n + ".picture"].shape[0] * golden[n + ".picture"].shape[1] % 64 for n in names)
    assert 0 < float(golden["deviation"]) < 1e-6
    for n in names:
        assert golden[n + ".picture"].dtype == np.uint8 and golden[n + ".picture"].shape[:2] == C.FIXTURE[n][1:3] and thr[n] == C.FIXTURE[n][3]
        assert max(golden[n + ".picture"].shape[:2]) <= 160


@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_host_statement_matches_the_unmodified_reference(golden, name):
    pic, thr = golden[name + ".picture"], [float(t) for t in golden[name + ".thresholds"]]
    host = H.decode(pic, golden["palette"], thr)
    assert host["live"] == int(golden[name + ".live"]) and len(host["scores"]) == 100
    assert np.array_equal(H.pack_bits(host["masks"].reshape(100, -1)), golden[name + ".masks"])          # the same masks in the same order
    err = float(np.abs(host["scores"] - golden[name + ".scores"]).max())
    print("%s: max |host - reference| %.3e, recorded %.3e" % (name, err, float(golden["deviation"])))
    assert err <= 2 * float(golden["deviation"])


def test_host_statement_details():
    pal = np.array([[10, 10, 10], [10, 10, 19], [200, 0, 0], [10, 10, 10]], np.float32)
    pic = np.array([[[10, 10, 10], [10, 10, 16], [10, 10, 22], [90, 90, 90]]], np.uint8)
    n, s = H.stats(pic, pal, [5.0, 2.0])                 # L1 / 3 < thr: L1 = 12 is inside thr 5, L1 = 6 is outside thr 2
    assert n.tolist() == [3, 3, 0, 3, 1, 2, 0, 1] and s.tolist() == [18, 15, 0, 18, 0, 6, 0, 0]
    assert H.survivors(n, s, 10).tolist() == [4, 7, 5, 1, 0, 3]                  # S / n = 0, 0, 3, 5, 6, 6: ties to the lower index
    assert H.survivors(n, s, 2).tolist() == [4, 7]
    bits = H.pack_bits(np.array([[1, 0, 1] + [0] * 30 + [1]], bool))
    assert bits.dtype == np.uint32 and bits.tolist() == [[5, 2]]
    m = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1]], bool)
    sc, keep, inter = H.matrix_nms(m, np.array([0.9, 0.8, 0.7]), max_num=2, sigma=2.0)
    assert inter.tolist() == [[3, 2, 0], [2, 2, 0], [0, 0, 1]] and keep.tolist() == [0, 2]
    assert sc.tolist() == [0.9, 0.7]
    sc = H.matrix_nms(m, np.array([0.9, 0.8, 0.7]), max_num=3, sigma=2.0)[0]
    assert abs(sc[2] - 0.8 * np.exp(-2.0 * (2 / 3) ** 2)) < 1e-15


def test_location_palette_is_the_reference_colour_rule(golden):
    from painter_amd.painter_engine import location_palette
    pal = location_palette()
    assert pal.dtype == np.float32 and pal.shape == (C.K, 3) and np.array_equal(pal, golden["palette"])
    assert tuple(pal[0]) == (255, 255, 255) and tuple(pal[1]) == (255, 255, 242) and tuple(pal[20]) == (255, 242, 255)
    assert tuple(pal[400]) == (240, 255, 255) and location_palette(16, 10).shape == (1600, 3)


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_inst_workspace_bytes", "pa_inst_workspace_offset", "pa_inst_stats", "pa_inst_intersections", "pa_inst_decode"):
        assert name in protos
        assert getattr(lib, name) is not None
    assert len(protos["pa_inst_decode"][1]) == 19
    assert lib.pa_inst_workspace_bytes(480, 640, 6400, 1, 2000) > 2000 * 480 * 640 // 8          # host only: no GPU needed
    assert lib.pa_inst_workspace_bytes(0, 640, 6400, 1, 2000) == -1 and lib.pa_inst_workspace_bytes(480, 640, 6400, 1, 4097) == -1
    assert lib.pa_abi_version() == 9


def test_instances_refuses_a_cpu_device():
    import torch
    from painter_amd import painter_engine as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.instances(np.zeros((4, 4, 3), np.uint8), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.instances(torch.zeros((4, 4, 3), dtype=torch.uint8))


# ---- with a reference checkout: the live reference
def _reference():
    from oracle import ref_import
    return os.path.isfile(os.path.join(ref_import.PAINTER_DIR, "eval", "coco_panoptic", "COCOCAInstSegEvaluatorCustom.py"))


@pytest.mark.skipif(not _reference(), reason="needs the reference's Painter/eval/coco_panoptic evaluator")
def test_live_reference_matches_fixture_and_host_statement(golden, tmp_path):
    from tests.golden import make_golden_painter_inst as G
    assert np.array_equal(G.load_palette(), golden["palette"])
    for name in ("thr19_c", "few"):
        rec, why = G.examine(golden[name + ".picture"], C.FIXTURE[name][3], str(tmp_path))
        assert not why, (name, why)
        assert np.array_equal(rec["masks"], golden[name + ".masks"]) and int(rec["live"]) == int(golden[name + ".live"])
        assert np.abs(rec["scores"].astype(np.float64) - golden[name + ".scores"]).max() <= 2 * float(golden["deviation"])
