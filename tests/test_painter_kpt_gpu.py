"""GPU parity of COCO keypoint AP (csrc/painter_kpt.hip through painter_engine.KeypointAP) against tests/painter_kpt_host.py -- the
definition, restated from the published source of mmpose's oks_nms and xtcocotools' COCOeval and unverified against mmpose / xtcocotools.

The bars.  Photo coordinates, rescored scores and box areas: bytes (every operation is stated).  The OKS doubles read from the workspace:
1e-12 relative -- both sides feed exp the same double and add at most 32 non-negative terms in the same order, so with each exp within
1 ulp of the true value (an assumption about numpy's libm and the device library, not checked here) two OKS values differ by a few tens
of ulps, about 5e-15.  Decisions -- order, survivors, rows, scores, areas, matched and ignored words -- are compared as bytes, which is
legitimate because tests/test_painter_kpt_cpu.py asserts for every case used here that no decision changes when every OKS is scaled by
1 -+ 1e-9 (the one exempt case is built from OKS exactly 1.0, where exp(-0.0) = 1 on both sides)."""
import numpy as np
import pytest
import torch

from tests import painter_kpt_cases as C
from tests import painter_kpt_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

OKS_BAR = 1e-12


def scorer(case, caps=(1, 1), ground_truth=None, **kw):
    ap = E.KeypointAP(case["ground_truth"] if ground_truth is None else ground_truth, **dict(case["settings"], **kw))
    ap.min_caps = caps
    return ap


def add(ap, case, rows=None, convert=lambda x: x):
    rows = np.arange(len(case["image_ids"])) if rows is None else np.asarray(rows)
    ids = None if case["bbox_ids"] is None and len(rows) == len(case["image_ids"]) else \
        [(i if case["bbox_ids"] is None else case["bbox_ids"][i]) for i in rows.tolist()]
    got = ap.add(convert(case["preds"][rows]), convert(case["maxvals"][rows]), case["centers"][rows], case["scales"][rows],
                 case["box_scores"][rows], [case["image_ids"][i] for i in rows.tolist()], ids)
    assert got is ap
    return ap


def same(got, ref):
    assert sorted(got) == sorted(ref)
    for image in ref:
        assert got[image].dtype == H.RECORD and got[image].tobytes() == ref[image]["records"].tobytes(), (image, got[image], ref[image]["records"])


def workspace(ap):
    """{image id: (order, survivor flags, OKS doubles)} of the last pa_kpt_evaluate, read from the workspace where the launch left them."""
    _, _, ws, shape, images = ap._last_eval
    n, d_cap, g_cap, max_det = shape
    a = ws.cpu().numpy()
    at = [lib.pa_kpt_workspace_offset(*shape, which) for which in range(3)]
    order = a[at[0]:at[0] + 4 * n * d_cap].view(np.int32).reshape(n, d_cap)
    alive = a[at[1]:at[1] + 4 * n * d_cap].view(np.int32).reshape(n, d_cap)
    oks = a[at[2]:at[2] + 8 * n * max_det * g_cap].view(np.float64).reshape(n, max_det, g_cap)
    return {image: (order[j], alive[j], oks[j]) for j, image in enumerate(images)}


def check_workspace(ap, ref, photos=None):
    """Order and survivors as integers, the OKS section within the bar -> the largest relative difference seen."""
    worst = 0.0
    ws = workspace(ap)
    for image in (ref if photos is None else photos):
        want = ref[image]
        d = len(want["order"])
        if d == 0:
            assert image not in ws
            continue
        order, alive, oks = ws[image]
        assert order[:d].tolist() == want["order"].tolist(), image
        assert alive[:d].tolist() == want["alive"].astype(int).tolist(), image
        e, g = want["oks"].shape
        got = oks[:e, :g]
        diff = np.abs(got - want["oks"])
        assert (diff <= OKS_BAR * np.abs(want["oks"])).all(), (image, float(diff.max()))
        if diff.size and (want["oks"] > 0).any():
            worst = max(worst, float((diff[want["oks"] > 0] / want["oks"][want["oks"] > 0]).max()))
    print("largest relative OKS difference: %.3g" % worst)
    return worst


def random_boxes(seed, n, k):
    rng = np.random.default_rng(seed)
    preds = (np.round(rng.uniform(-1, 255, (n, k, 2)) * 4) / 4).astype(np.float32)
    maxvals = (np.round(rng.uniform(0, 1, (n, k)) * 16) / 16).astype(np.float32)
    maxvals[0] = 0.125                                           # nothing above vis_thr: score 0
    return preds, maxvals, rng.uniform(0, 640, (n, 2)).astype(np.float32), rng.uniform(0.2, 3, (n, 2)).astype(np.float32), \
        rng.uniform(0.1, 1, n).astype(np.float32)


@pytest.mark.parametrize("n,k", [(1, 17), (65, 17), (3, 3)])
def test_poses_equal_the_statement(n, k):
    boxes = random_boxes(n + k, n, k)
    ap = E.KeypointAP({}, sigmas=H.SIGMAS[:k])
    ap.add(*boxes, [0] * n)
    want = H.poses(*boxes, C.HEAT)
    got = ap.poses()
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.tobytes() == w.tobytes()
    assert got[1][0] == 0 and (got[1][1:] > 0).any() if n > 1 else got[1][0] == 0
    for i in range(n):                                           # the project's own to_image, bit for bit
        assert got[0][i, :, :2].tobytes() == E.to_image(boxes[0][i], boxes[2][i], boxes[3][i], C.HEAT).astype(np.float32).tobytes()
    # CUDA tensors in place of numpy arrays
    dev = E.KeypointAP({}, sigmas=H.SIGMAS[:k]).add(torch.from_numpy(boxes[0]).cuda(), torch.from_numpy(boxes[1]).cuda(), *boxes[2:], [0] * n)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(dev.poses(), want))


def test_mixed_photos_in_one_call():
    """0 boxes / 2 ground truths, 3 / 0, 1 / 1, 65 / 9 and 130 / 5 in one call: 65 and 130 cross wave boundaries, equal scores occur."""
    case = C.case("mixed")
    ref = case["statement"]
    ap = add(scorer(case), case)
    got = ap.records()
    same(got, ref)
    assert len(got[100]) == 0 and len(got[101]) == 3 and len(got[104]) == 20
    assert ap.survivors[104] == int(ref[104]["alive"].sum()) and ap.survivors[100] == 0
    check_workspace(ap, ref)
    res = ap.result()
    want = H.keypoint_ap({i: r["records"] for i, r in ref.items()}, case["ground_truth"])
    assert sorted(res) == sorted(want) and 0 < res["AP"] < 1
    for key, v in want.items():
        assert np.array_equal(np.asarray(res[key]), np.asarray(v)), key


def test_ground_truths_of_the_second_word():
    """70 ground truths, 64 evaluated survivors: ground truths 64 .. 69 are the second 64-bit word of the walk's free / ignored / taken
    bits.  tests/test_painter_kpt_cpu.py asserts on the statement that one of them is taken at (all, 0.5), one is ignored in another
    range and one detection stays unmatched; here records, order and survivors are compared as bytes, the OKS within the bar."""
    case = C.case("second_word")
    ref = case["statement"]
    ap = add(scorer(case), case)
    got = ap.records()
    same(got, ref)
    assert len(got[100]) == 64 and ap._last_eval[3] == (1, 93, 70, 64)
    assert ap.survivors[100] == int(ref[100]["alive"].sum())
    check_workspace(ap, ref)


def test_caps_and_max_det():
    crowded = C.case("crowded")
    ref = crowded["statement"]
    ap = add(scorer(crowded), crowded)
    same(ap.records(), ref)
    assert ap._last_eval[3][1] == 1024 and 20 < ap.survivors[7] < 1024 and ap.survivors[7] == int(ref[7]["alive"].sum())
    check_workspace(ap, ref)
    more = C.case("twenty_one")                                  # 21 survivors: the 21st is never evaluated
    ap = add(scorer(more), more)
    same(ap.records(), more["statement"])
    assert ap.survivors[3] == 21 and len(ap.records()[3]) == 20
    check_workspace(ap, more["statement"])
    mixed = C.case("mixed_64")                                   # capacities above the tables change nothing; max_det at its cap
    ap = add(scorer(mixed, caps=(1024, 128)), mixed)
    same(ap.records(), mixed["statement"])
    assert ap._last_eval[3] == (4, 1024, 128, 64) and len(ap.records()[104]) == 64
    assert ap.records()[104][:20].tobytes() == C.statement(mixed, max_dets=(20,))[104]["records"].tobytes()
    check_workspace(ap, mixed["statement"])


def test_exact_cases():
    """Detections equal to their ground truths: OKS exactly 1.0, matched at every threshold, a caller's threshold of 1.0 included.
    Poses 10^4 pixels apart in tiny boxes: every term underflows, OKS exactly 0, no match and no suppression."""
    case = C.case("identical")
    ap = add(scorer(case), case)
    got = ap.records()[3]
    oks = workspace(ap)[3][2]
    assert oks[0, 0] == 1.0 and oks[1, 1] == 1.0                 # exp(-0.0) is exactly 1 on the device
    assert got["matched"][:2].tolist() == [0x1ff, 0x1ff] and got["matched"][2:].tolist() == [0, 0]
    same(ap.records(), case["statement"])
    far = C.case("far")
    ap = add(scorer(far), far)
    same(ap.records(), far["statement"])
    order, alive, oks = workspace(ap)[3]
    assert (oks[:5, :2] == 0.0).all() and alive[:5].tolist() == [1] * 5 and (ap.records()[3]["matched"] == 0).all()


def test_custom_settings():
    case = C.case("no_nms")                                      # use_nms=False: everything survives, equal scores to the lower row
    ap = add(scorer(case), case)
    same(ap.records(), case["statement"])
    check_workspace(ap, case["statement"])
    assert ap.survivors[100] == 12 and ap.survivors[101] == 9
    hand = C.case("hand_made")                                   # K = 3, custom sigmas, thresholds a millionth either side of the OKS
    ap = add(scorer(hand), hand)
    got = ap.records()[1]
    same(ap.records(), hand["statement"])
    assert got["matched"].tolist() == [1, 0] and got["row"].tolist() == [0, 1]
    assert abs(workspace(ap)[1][2][0, 0] - hand["oks"]) <= OKS_BAR * hand["oks"]
    assert ap.result()["AP50"] == -1.0                           # no threshold 0.5 among the caller's


def test_chaining_split_calls_two_runs_and_reset():
    case = C.case("chain")
    ref = case["statement"]
    pictures, flipped = torch.from_numpy(case["pictures"]).cuda(), torch.from_numpy(case["flipped"]).cuda()
    decodes = [E.PoseDecode(pictures[:4], flipped[:4]), E.PoseDecode(pictures[4:], flipped[4:])]
    before = [d.result() for d in decodes]
    assert np.concatenate([b["preds"] for b in before]).tobytes() == case["preds"].tobytes()
    ap = scorer(case).add_decodes(decodes, case["centers"], case["scales"], case["box_scores"], case["image_ids"], case["bbox_ids"])
    chained = ap.records()
    same(chained, ref)                                           # duplicate bbox_id 3 of photo 51: the first one stays
    assert sorted(chained[51]["row"].tolist()) == [1, 3] and len(chained[52]) == 0
    check_workspace(ap, ref)
    after = [d.result() for d in decodes]
    assert all(a[key].tobytes() == b[key].tobytes() for a, b in zip(after, before) for key in ("preds", "maxvals"))
    copied = E.keypoints(pictures, flipped)
    plain = scorer(case).add(copied["preds"], copied["maxvals"], case["centers"], case["scales"], case["box_scores"], case["image_ids"],
                             case["bbox_ids"])
    same(plain.records(), ref)
    # a photo's boxes split over two calls, and the same scorer run twice
    split = C.case("split")
    whole = add(scorer(split), split)
    halves = add(add(scorer(split), split, [0, 1, 2, 7, 8]), split, [3, 4, 5, 6, 9, 10, 11])
    same(whole.records(), split["statement"])
    first = {i: r.tobytes() for i, r in halves.records().items()}
    rows = [0, 1, 2, 7, 8, 3, 4, 5, 6, 9, 10, 11]               # a record's row is its position in the order of arrival
    for image, want in split["statement"].items():
        got = halves.records()[image]
        assert [rows[r] for r in got["row"].tolist()] == want["records"]["row"].tolist()
        assert all(got[name].tobytes() == want["records"][name].tobytes() for name in ("score", "area", "matched", "ignored"))
    halves._records = None
    assert {i: r.tobytes() for i, r in halves.records().items()} == first
    assert whole.reset() is whole and all(len(r) == 0 for r in whole.records().values())
    same(add(whole, split).records(), split["statement"])


@pytest.mark.parametrize("bit", [0, 1])
def test_a_flagged_photo_in_the_middle_emits_nothing(bit):
    case = C.case("flags")
    ref = case["statement"]
    bad, gt = dict(case), None
    if bit == 0:
        bad["preds"] = case["preds"].copy()
        bad["preds"][4, 2, 1] = np.nan                           # one coordinate of one box of photo 101
    else:
        gt = dict(case["ground_truth"])
        gt[101] = [dict(gt[101][0], area=-1.0)] + gt[101][1:]
    ap = add(scorer(case, ground_truth=gt), bad)
    with pytest.raises(ValueError, match=r"photo 101 is refused \(flag bit %d" % bit):
        ap.records()
    out, oat, (n, _, _, max_det) = ap._outs[0]
    a = out.cpu().numpy()
    images = ap._last_eval[4]
    counts, flags = E._section(a, oat, "counts"), E._section(a, oat, "flags")
    table = E._section(a, oat, "records").reshape(n, max_det)
    assert [int(flags[images.index(i)]) for i in (100, 101, 102)] == [0, 1 << bit, 0] and counts[images.index(101)] == 0
    for image in (100, 102):                                     # the neighbours still emit
        j = images.index(image)
        assert counts[j] > 0 and table[j, :counts[j]].tobytes() == ref[image]["records"].tobytes()


def test_run_pose_ap_equals_scoring_what_run_pose_returns():
    from tests import painter_eval_cases as PC
    rng = np.random.default_rng(8)
    queries = [PC.picture(91 + i, 64, 48) for i in range(5)]
    sizes = [C.CHAIN_HEAT] * 5
    people = [C.person(rng) for _ in range(5)]
    centers, scales = np.stack([p[1] for p in people]), np.stack([p[2] for p in people])
    box_scores = np.array([0.75, 0.5, 1.0, 0.625, 0.875], np.float32)
    image_ids, bbox_ids = [1, 2, 1, 2, 1], [4, 3, 2, 1, 0]

    def engine(task, bs):
        return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)
    back = engine("coco_pose", 8).run_pose(queries, "mirror", sizes)
    preds, maxvals = np.stack([b["preds"] for b in back]), np.stack([b["maxvals"] for b in back])
    assert (maxvals > 0.2).any()
    pose = H.poses(preds, maxvals, centers, scales, box_scores, C.CHAIN_HEAT)[0]
    truth = lambda i: dict(keypoints=np.concatenate([pose[i, :, :2].astype(np.float64), np.full((17, 1), 2.0)], 1).ravel().tolist(),
                           area=3000.0, bbox=[0, 0, 50, 60], iscrowd=0, num_keypoints=17)
    gt = {1: [truth(0)], 2: [truth(3), people[4][0]], 3: []}     # boxes 0 and 3 are ground truths: OKS exactly 1.0
    kw = dict(heatmap_size=C.CHAIN_HEAT)
    want = E.KeypointAP(gt, **kw).add(preds, maxvals, centers, scales, box_scores, image_ids, bbox_ids).records()
    assert any((r["matched"] != 0).any() for r in want.values()) and sum(len(r) for r in want.values()) >= 3
    for bs in (2, 8):
        score = E.KeypointAP(gt, **kw)
        assert engine("coco_pose", bs).run_pose_ap(queries, centers, scales, box_scores, image_ids, score, "mirror", sizes, bbox_ids) is score
        got = score.records()
        assert sorted(got) == [1, 2, 3] and all(got[i].tobytes() == want[i].tobytes() for i in want)
    with pytest.raises(ValueError, match="coco_pose"):
        engine("coco_pano_inst", 2).run_pose_ap(queries, centers, scales, box_scores, image_ids, E.KeypointAP(gt, **kw), None, sizes)
    with pytest.raises(ValueError, match="5 pictures, 4 boxes"):
        engine("coco_pose", 2).run_pose_ap(queries, centers[:4], scales[:4], box_scores[:4], image_ids, E.KeypointAP(gt, **kw), None, sizes)
    with pytest.raises(ValueError, match="4 image ids"):
        engine("coco_pose", 2).run_pose_ap(queries, centers, scales, box_scores, image_ids[:4], E.KeypointAP(gt, **kw), None, sizes)
    with pytest.raises(ValueError, match="image id 9 is not"):
        engine("coco_pose", 2).run_pose_ap(queries, centers, scales, box_scores, [1, 2, 9, 2, 1], E.KeypointAP(gt, **kw), None, sizes)
    with pytest.raises(ValueError, match="has boxes but is not in ground_truth"):
        E.KeypointAP(gt, **kw).add(preds, maxvals, centers, scales, box_scores, [1, 2, 9, 2, 1]).records()
