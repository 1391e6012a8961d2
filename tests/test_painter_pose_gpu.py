"""GPU parity of the pose keypoint decode (csrc/painter_pose.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_pose_host.py -- the definition -- and against what the unmodified reference produced (tests/golden/painter_pose.npz).

The bar: everything is equal, no tolerance.  The heat values are table look-ups, one float32 add and an exact halving; the peak is an
argmax of those floats with the first index winning; the refinement is the sign of a float32 difference."""
import os

import numpy as np
import pytest
import torch

from tests import painter_pose_cases as C
from tests import painter_pose_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

INVALID = 1                                            # hipErrorInvalidValue
MODES = [("flip", True), ("flip", False), ("plain", True)]          # (flip test or not, shift): without flipped pictures the shift is moot


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_pose.npz"))


def _same(got, ref):
    assert got["preds"].dtype == got["maxvals"].dtype == np.float32
    assert got["preds"].shape == ref["preds"].shape and got["maxvals"].shape == ref["maxvals"].shape
    bad = np.argwhere((got["preds"] != ref["preds"]).any(-1) | (got["maxvals"] != ref["maxvals"]))
    assert len(bad) == 0, (bad[:5], got["preds"][tuple(bad[0])], ref["preds"][tuple(bad[0])], got["maxvals"][tuple(bad[0])],
                           ref["maxvals"][tuple(bad[0])])


# ---- 1. the unmodified reference
@pytest.mark.parametrize("name", C.FIXTURE + ["hand"])
@pytest.mark.parametrize("mode", ["flip", "plain"])
def test_pose_heatmaps_reproduce_the_reference(golden, name, mode):
    p, q = golden[name + ".pictures"], golden[name + ".flipped"]
    assert np.array_equal(golden["palette"], E.pose_palette())
    got = E.pose_heatmaps(p, q if mode == "flip" else None)
    ref = golden["%s.%s.heatmaps" % (name, mode)]
    assert got.dtype == np.float32 and got.shape == ref.shape and got.tobytes() == ref.tobytes()
    _same(E.keypoints(p, q if mode == "flip" else None), dict(preds=golden["%s.%s.preds" % (name, mode)],
                                                              maxvals=golden["%s.%s.maxvals" % (name, mode)]))


@pytest.mark.parametrize("mode", ["flip", "plain"])
def test_full_size_box_reproduces_the_reference(golden, mode):
    """256 x 192, 24 workgroups per box: maximum, first argmax and the peak's four neighbours of every channel as the reference has them."""
    p, q = golden["full.pictures"], golden["full.flipped"]
    q = q if mode == "flip" else None
    got = E.keypoints(p, q)
    _same(got, dict(preds=golden["full.%s.preds" % mode], maxvals=golden["full.%s.maxvals" % mode]))
    assert np.array_equal(got["maxvals"], golden["full.%s.max" % mode])
    maps = E.pose_heatmaps(p, q)
    flat = maps.reshape(1, C.K, -1)
    idx = golden["full.%s.argmax" % mode]
    assert np.array_equal(flat.argmax(2), idx)
    pad = np.pad(maps, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y, x = idx[0] // 192 + 1, idx[0] % 192 + 1
    k = np.arange(C.K)
    assert np.array_equal(np.stack([pad[0, k, y, x - 1], pad[0, k, y, x + 1], pad[0, k, y - 1, x], pad[0, k, y + 1, x]], -1),
                          golden["full.%s.neighbours" % mode][0])
    assert np.array_equal(maps, H.heatmaps(p, q, C.PALETTE, C.PAIR))


# ---- 2. the definition, over shapes and modes
@pytest.mark.parametrize("name", list(C.SHAPES) + ["hand"])
def test_keypoints_equal_the_host_statement(name):
    """3 x 3 (no pixel inside the border), 4 x 4 (one), 5 x 5, 8 x 6, 33 x 17 (odd), 70 x 61 (three chunks per box), 33 boxes."""
    p, q = C.hand_boxes()[:2] if name == "hand" else C.shape_pair(name)
    for mode, shift in MODES:
        twin = q if mode == "flip" else None
        ref = H.keypoints(p, twin, C.PALETTE, C.PAIR, shift=shift)
        _same(E.keypoints(p, twin, shift_heatmap=shift), ref)
        assert np.array_equal(E.pose_heatmaps(p, twin, shift_heatmap=shift), H.heatmaps(p, twin, C.PALETTE, C.PAIR, shift=shift)), (mode, shift)
        if name == "3x3":
            assert (ref["preds"] == np.floor(ref["preds"])).all()
    if name == "hand":
        preds, maxvals = C.hand_expected()
        _same(E.keypoints(p, q), dict(preds=preds, maxvals=maxvals))


def test_smallest_pictures_with_and_without_an_interior():
    """1 < px < w - 1 has no solution at 3 x 3 and exactly px = 2 at 4 x 4: the peak with a weaker left neighbour moves only there."""
    for w, expect in ((3, (1.0, 1.0)), (4, (1.75, 2.0))):
        p = np.zeros((1, w, w, 3), np.uint8)
        c = w // 2
        p[0, c, c], p[0, c, c - 1] = (200, 255, 255), (100, 255, 255)
        for twin in (None, np.zeros_like(p)):
            got = E.keypoints(p, twin)
            _same(got, H.keypoints(p, twin, C.PALETTE, C.PAIR))
            assert tuple(got["preds"][0, 0]) == expect and (got["preds"][0, 1:] == -1).all() and (got["maxvals"][0, 1:] == 0).all()


def test_boxes_do_not_share_state():
    """n = 1, 3, 33: every box of a batch equals the box alone; a list of pictures equals the stacked array."""
    p, q = C.shape_pair("many")
    whole = E.keypoints(p, q)
    for n in (1, 3):
        part = E.keypoints(p[:n], q[:n])
        assert np.array_equal(part["preds"], whole["preds"][:n]) and np.array_equal(part["maxvals"], whole["maxvals"][:n])
    last = E.keypoints([p[32]], [q[32]])
    assert np.array_equal(last["preds"][0], whole["preds"][32]) and np.array_equal(last["maxvals"][0], whole["maxvals"][32])
    assert len({whole["preds"][i].tobytes() for i in range(33)}) == 33


@pytest.mark.parametrize("k", [1, 17, 32])
def test_custom_palette(k):
    pal, pairs = C.custom_palette(k)
    p, q = C.painted_pair(40 + k, 3, 12, 10, palette=pal, pair=H.pair_table(pairs, k))
    pair = H.pair_table(pairs, k)
    for mode, shift in MODES:
        twin = q if mode == "flip" else None
        ref = H.keypoints(p, twin, pal, pair, shift=shift)
        assert ref["preds"].shape == (3, k, 2) and (ref["maxvals"] > 0).any()
        _same(E.keypoints(p, twin, palette=pal, flip_pairs=pairs, shift_heatmap=shift), ref)
        assert np.array_equal(E.pose_heatmaps(p, twin, palette=pal, flip_pairs=pairs, shift_heatmap=shift),
                              H.heatmaps(p, twin, pal, pair, shift=shift))


# ---- 3. determinism, inputs
def test_two_runs_give_identical_bytes_and_tensors_equal_arrays():
    p, q = C.full_pair()
    first = E.keypoints(p, q)
    again = E.keypoints(p, q)
    assert first["preds"].tobytes() == again["preds"].tobytes() and first["maxvals"].tobytes() == again["maxvals"].tobytes()
    dp, dq = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    dev = E.keypoints(dp, dq)
    assert first["preds"].tobytes() == dev["preds"].tobytes() and first["maxvals"].tobytes() == dev["maxvals"].tobytes()
    lists = E.keypoints([dp[0]], [dq[0]])
    assert first["preds"].tobytes() == lists["preds"].tobytes()
    assert E.pose_heatmaps(dp, dq).tobytes() == E.pose_heatmaps(p, q).tobytes()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.keypoints(p, q, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.keypoints(torch.from_numpy(p), None)


# ---- 4. the C ABI
def test_entry_points_refuse_bad_arguments():
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched."""
    a = 256                                            # a non-null, aligned, never dereferenced address
    ok = dict(n=2, h=8, w=6, k=17)

    def keyp(c, ptrs=None):
        pic, pal, pair, ws, preds, maxv = ptrs or [a] * 6
        return lib.pa_pose_keypoints(pic, 0, pal, pair, c["n"], c["h"], c["w"], c["k"], 1, ws, preds, maxv, 0)

    def heat(c, ptrs=None):
        pic, pal, pair, out = ptrs or [a] * 4
        return lib.pa_pose_heatmaps(pic, 0, pal, pair, c["n"], c["h"], c["w"], c["k"], 1, out, 0)

    for change in (dict(k=33), dict(k=0), dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15)):
        c = dict(ok, **change)
        assert keyp(c) == INVALID and heat(c) == INVALID, change
    for null in range(6):
        assert keyp(ok, [0 if i == null else a for i in range(6)]) == INVALID, null
    for null in range(4):
        assert heat(ok, [0 if i == null else a for i in range(4)]) == INVALID, null
    assert keyp(ok, [a, a, a, a + 4, a, a]) == INVALID                                 # misaligned workspace
    assert lib.pa_pose_workspace_bytes(2, 17) == 2 * 17 * 8
    assert lib.pa_pose_workspace_bytes(0, 17) == lib.pa_pose_workspace_bytes(2, 33) == lib.pa_pose_workspace_bytes(2, 0) == -1
    pal33 = np.concatenate([np.stack([np.arange(33) * 7 + 1, np.arange(33) * 5 + 2], -1), [[0, 0]]])
    with pytest.raises(RuntimeError, match="pa_pose_keypoints"):
        E.keypoints(np.zeros((1, 4, 4, 3), np.uint8), palette=pal33, flip_pairs=())
    with pytest.raises(RuntimeError, match="pa_pose_heatmaps"):
        E.pose_heatmaps(np.zeros((0, 4, 4, 3), np.uint8))


# ---- 5. the engine
def test_run_pose_equals_keypoints_of_the_pictures_run_returns():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48), PC.picture(92, 60, 80), PC.picture(93, 45, 70)]
    twins = [PC.picture(94, 64, 48), PC.picture(95, 60, 80), PC.picture(96, 45, 70)]
    sizes = [(24, 32)] * 3                              # (width, height): small painted pictures keep the stand-in model's test quick

    def engine(task, bs):
        return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)
    plain = engine("coco_pose", 8).run(queries, sizes)
    flipped = engine("coco_pose", 8).run(twins, sizes)
    assert plain[0].shape == (32, 24, 3) and plain[0].dtype == np.uint8
    ref = E.keypoints(plain, flipped)
    assert (ref["maxvals"] > 0).any()
    for bs in (1, 2, 8):
        got = engine("coco_pose", bs).run_pose(queries, twins, sizes)
        assert len(got) == 3 and sorted(got[0]) == ["maxvals", "preds"] and got[0]["preds"].shape == (17, 2)
        _same(dict(preds=np.stack([g["preds"] for g in got]), maxvals=np.stack([g["maxvals"] for g in got])), ref)
    alone = engine("coco_pose", 2).run_pose(queries, None, sizes, shift_heatmap=False)
    _same(dict(preds=np.stack([g["preds"] for g in alone]), maxvals=np.stack([g["maxvals"] for g in alone])), E.keypoints(plain))
    mirrored = engine("coco_pose", 4).run_pose(queries, "mirror", sizes)
    twin_pictures = engine("coco_pose", 8).run([np.ascontiguousarray(p[:, ::-1]) for p in queries], sizes)
    _same(dict(preds=np.stack([g["preds"] for g in mirrored]), maxvals=np.stack([g["maxvals"] for g in mirrored])),
          E.keypoints(plain, twin_pictures))
    assert engine("coco_pose", 2).run_pose([], None) == []


def test_run_pose_refuses_other_tasks_and_mixed_sizes():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48), PC.picture(92, 60, 80)]

    def engine(task):
        return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=2)
    with pytest.raises(ValueError, match="coco_pose"):
        engine("coco_pano_inst").run_pose(queries)
    with pytest.raises(AssertionError, match="one output size"):
        engine("coco_pose").run_pose(queries, None, [(24, 32), (32, 24)])
    with pytest.raises(ValueError, match="mirror"):
        engine("coco_pose").run_pose(queries, "flip")
    with pytest.raises(TypeError, match="unexpected"):
        engine("coco_pose").run_pose(queries, None, dist_thr=3.0)
    with pytest.raises(AssertionError):
        engine("coco_pose").run_pose(queries, queries[:1])
