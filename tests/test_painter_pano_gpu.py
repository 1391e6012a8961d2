"""GPU parity of the panoptic merge (csrc/painter_pano.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_pano_host.py -- the definition: integer class vote, paste and stuff fill with the reference's own double comparisons -- and
against what the unmodified evaluators produced (tests/golden/painter_pano.npz).

The bars.  Vote sums, classes, panoptic map, ids, categories, instance ids, areas, the id2rgb picture: equal, no tolerance.  A thing's
score in the segment list is the instance decode's float32 score: against the fixture within 4 x the deviation the reference's own
float32 arithmetic showed (the bar of tests/test_painter_inst_gpu.py); where the scores are supplied, equal.  No fixture case is skipped."""
import os

import numpy as np
import pytest
import torch

from tests import painter_inst_cases as IC
from tests import painter_inst_host as IH
from tests import painter_pano_cases as C
from tests import painter_pano_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

K, T = C.K, C.N_THINGS
INVALID = 1                                            # hipErrorInvalidValue


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_pano.npz"))


@pytest.fixture(scope="module")
def score_bar(golden_dir):
    return 4 * float(np.load(os.path.join(golden_dir, "painter_inst.npz"))["deviation"])


def _check_result(res, h, w):
    """What every result of `panoptic` must satisfy by itself."""
    pan, seg = res["panoptic"], res["segments"]
    assert pan.dtype == np.int32 and pan.shape == (h, w) and res["rgb"].dtype == np.uint8
    assert np.array_equal(res["rgb"], E.id2rgb(pan)) and np.array_equal(H.rgb2id(res["rgb"]), pan)
    assert [s["id"] for s in seg] == list(range(1, len(seg) + 1)) and set(np.unique(pan).tolist()) <= set(range(len(seg) + 1))
    assert len(res["areas"]) == len(seg)
    for s, a in zip(seg, res["areas"]):
        assert int((pan == s["id"]).sum()) == a
        assert sorted(s) == (["category_id", "id", "instance_id", "isthing", "score"] if s["isthing"] else ["area", "category_id", "id", "isthing"])
        assert s["isthing"] or s["area"] == a
    assert res["classes"].dtype == np.int32 and len(res["classes"]) == len(res["scores"]) == len(res["masks"])
    assert res["masks"].dtype in (bool, torch.bool) and res["scores"].dtype == np.float32


def _same_segments(got, ref, score_tol=0.0):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert set(g) == set(r) and all(g[k] == r[k] for k in r if k != "score"), (g, r)
        assert abs(g.get("score", 0.0) - r.get("score", 0.0)) <= score_tol, (g, r)


# ---- 1. the unmodified reference
@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_panoptic_reproduces_the_reference(golden, score_bar, name):
    _, h, w, thr, merge, _ = C.FIXTURE[name]
    sem, inst = golden[name + ".semseg"], golden[name + ".inst"]
    assert np.array_equal(golden["palette"], E.semantic_palette()) and sem.shape[:2] == (h, w)
    res = E.panoptic(sem, inst, dist_thr=thr, overlap_threshold=merge[0], stuff_area_thresh=merge[1], instances_score_thresh=merge[2])
    _check_result(res, h, w)
    assert np.array_equal(IH.pack_bits(res["masks"].reshape(100, -1)), golden[name + ".masks"])          # the same 100 instances
    assert np.array_equal(res["classes"], golden[name + ".classes"])
    assert np.array_equal(res["panoptic"], golden[name + ".panoptic"]) and np.array_equal(res["areas"], golden[name + ".areas"])
    ref = []
    for (sid, isthing, cat, iid, area), score in zip(golden[name + ".segments"].tolist(), golden[name + ".segment_scores"].tolist()):
        ref.append(dict(id=sid, isthing=True, score=score, category_id=cat, instance_id=iid) if isthing else
                   dict(id=sid, isthing=False, category_id=cat, area=area))
    _same_segments(res["segments"], ref, score_bar)
    print("%s: %d things, %d stuff segments" % (name, sum(s["isthing"] for s in ref), sum(not s["isthing"] for s in ref)))


# ---- 2. the vote alone
_decoded = {}


def _instances_of(name):
    """Device-decoded instances of a tie-heavy instance case with its semantic picture (inputs of the vote; computed once)."""
    if name not in _decoded:
        thr = IC.DECODE[name][3]
        sem, inst = C.decode_pair(name)
        dec = E.InstanceDecode(torch.from_numpy(inst).cuda(), None, thr, 2000, 100, "gaussian", 2.0)
        _decoded[name] = (sem, dec.result(with_bits=True))
    return _decoded[name]


def _device_vote(sem, bits, n, n_things, dist_type, max_inst=None, pal=None):
    pal = E.semantic_palette() if pal is None else pal
    m = max_inst or max(len(bits), 1)
    rows = np.zeros((m, bits.shape[1]), np.uint32)
    rows[:len(bits)] = bits
    dbits = torch.from_numpy(rows.view(np.int32)).cuda()
    dsem, dpal = torch.from_numpy(sem).cuda(), torch.from_numpy(np.array(pal, np.float32)).cuda()
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    sums = torch.full((m, n_things), -1, dtype=torch.int64, device="cuda")
    cls = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    assert lib.pa_pano_vote(dsem.data_ptr(), dpal.data_ptr(), dbits.data_ptr(), count.data_ptr(), sem.shape[0], sem.shape[1], len(pal), n_things,
                            E.DIST_TYPES[dist_type], m, sums.data_ptr(), cls.data_ptr(), E._stream()) == 0
    return sums.cpu().numpy(), cls.cpu().numpy()


@pytest.mark.parametrize("name", ["ties_thr5", "ties_two_thr", "odd_size"])
@pytest.mark.parametrize("dist_type", ["abs", "square", "mean"])
def test_vote_entry_point(name, dist_type):
    sem, inst = _instances_of(name)
    n = len(inst["masks"])
    assert n > 20
    sums, cls = _device_vote(sem, inst["bits"], n, T, dist_type, max_inst=n + 3)
    ref_s, ref_c = H.vote(sem, E.semantic_palette(), inst["masks"], T, dist_type)
    assert np.array_equal(sums[:n], ref_s) and np.array_equal(cls[:n], ref_c)
    assert not sums[n:].any() and not cls[n:].any()                                     # slots past the count: cleared, class 0
    print("%s %s: %d instances, %d distinct classes, largest sum %d" % (name, dist_type, n, len(set(ref_c.tolist())), ref_s.max()))


def test_vote_with_every_colour_a_thing_ties_and_empty_masks():
    sem, inst = _instances_of("odd_size")
    h, w = sem.shape[:2]
    masks = inst["masks"][:6].copy()
    masks[2] = False                                                                    # an empty mask: class 0
    flat = np.full((h, w, 3), 255, np.uint8)                                            # colour 0 everywhere ...
    pal = E.semantic_palette().copy()
    pal[5] = pal[0]                                                                     # ... which two classes share: ties to the lower
    bits = IH.pack_bits(masks.reshape(6, -1))
    bits[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(h * w % 32)                       # padding bits set: they must not count
    sums, cls = _device_vote(flat, bits, 6, K, "abs", pal=pal)
    ref_s, ref_c = H.vote(flat, pal, masks, K, "abs")
    assert np.array_equal(sums, ref_s) and np.array_equal(cls, ref_c) and cls.tolist() == [0] * 6 and not sums[2].any()
    sums, cls = _device_vote(sem, bits, 6, K, "mean")
    ref_s, ref_c = H.vote(sem, E.semantic_palette(), masks, K, "mean")
    assert np.array_equal(sums, ref_s) and np.array_equal(cls, ref_c)
    assert _device_vote(sem, bits, 0, T, "abs")[1].tolist() == [0] * 6                  # n == 0
    got = E.classify_instances(sem, masks)
    assert got.dtype == np.int32 and np.array_equal(got, H.vote(sem, E.semantic_palette(), masks, T)[1])
    assert np.array_equal(E.classify_instances(torch.from_numpy(sem).cuda(), IH.pack_bits(masks.reshape(6, -1))), got)
    assert np.array_equal(E.classify_instances(sem, torch.from_numpy(masks).cuda(), dist_type="square"),
                          H.vote(sem, E.semantic_palette(), masks, T, "square")[1])
    assert E.classify_instances(sem, np.zeros((0, h, w), bool)).shape == (0,)


# ---- 3. the merge alone
def _device_merge(semmap, masks, scores, classes, n_things=T, n_colours=K, merge=(0.5, 8192, 0.55), n=None, garbage=False, rgb=True):
    """pa_pano_merge on supplied instances -> dict(panoptic, rgb, segments (table rows), count)."""
    h, w = semmap.shape
    n = len(masks) if n is None else n
    m = max(len(masks), 1)
    bits = np.zeros((m, (h * w + 31) // 32), np.uint32)
    if len(masks):
        bits[:len(masks)] = IH.pack_bits(np.asarray(masks).reshape(len(masks), -1))
    if garbage and h * w % 32:
        bits[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(h * w % 32)
    sc, cl = np.zeros(m, np.float32), np.zeros(m, np.int32)
    sc[:len(masks)], cl[:len(masks)] = scores, classes
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dsem, dbits, dsc, dcl = dev(semmap.astype(np.int32)), dev(bits.view(np.int32)), dev(sc), dev(cl)
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.pa_pano_workspace_bytes(h, w, n_colours, n_things, m), dtype=torch.uint8, device="cuda")
    cap = m + n_colours - n_things
    pan = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    pic = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    seg = torch.full((max(cap, 1) * E.SEGMENT.itemsize,), 255, dtype=torch.uint8, device="cuda")
    assert lib.pa_pano_merge(dsem.data_ptr(), dbits.data_ptr(), dsc.data_ptr(), dcl.data_ptr(), count.data_ptr(), h, w, n_colours, n_things, m,
                             float(merge[0]), float(merge[1]), float(merge[2]), ws.data_ptr(), pan.data_ptr(), pic.data_ptr() if rgb else None,
                             out_n.data_ptr(), seg.data_ptr(), E._stream()) == 0
    table = seg.cpu().numpy()[:cap * E.SEGMENT.itemsize].view(E.SEGMENT)
    cnt = int(out_n.cpu()[0])
    assert not table[cnt:].view(np.uint8).any()                                         # entries past the count are cleared
    return dict(panoptic=pan.cpu().numpy(), rgb=pic.cpu().numpy(), table=table[:cnt], count=cnt)


def _compare_merge(got, semmap, masks, scores, classes, n_things=T, n_colours=K, merge=(0.5, 8192, 0.55)):
    ref = H.merge(semmap, np.asarray(masks, bool), scores, classes, n_things, n_colours, *merge)
    assert np.array_equal(got["panoptic"], ref["panoptic"]) and got["count"] == len(ref["segments"])
    for row, s, a in zip(got["table"], ref["segments"], ref["areas"]):
        assert (row["id"], bool(row["isthing"]), row["category_id"], row["area"]) == (s["id"], s["isthing"], s["category_id"], a)
        assert row["instance_id"] == s.get("instance_id", -1) and float(row["score"]) == s.get("score", 0.0)
    return ref


def _random_instances(seed, h, w, n, side=0.5):
    """Random boxes with many overlaps, scores in [0, 1) rounded to 1 / 16 so that equal scores occur."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, h, w), bool)
    for m in masks:
        y, x = rng.integers(0, h), rng.integers(0, w)
        m[y:y + rng.integers(1, max(2, int(h * side))), x:x + rng.integers(1, max(2, int(w * side)))] = True
    scores = (rng.integers(0, 16, n) / 16.0).astype(np.float32)
    semmap = rng.integers(0, K, (h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w].astype(np.int32)
    return semmap, masks, scores, rng.integers(0, T, n).astype(np.int32)


@pytest.mark.parametrize("merge", [(0.5, 64, 0.55), (0.1, 1, 0.0), (0.9, 300, 0.25), (0.0, 0, 0.0)])
def test_merge_entry_point_unsorted_equal_scores(merge):
    """61 x 83 = 5063 pixels (a last word with 7 pixels, its padding bits set), 60 boxes in random score order with equal scores, an
    all-zero mask, more than one block of every pass."""
    semmap, masks, scores, classes = _random_instances(5, 61, 83, 60, side=0.4)
    masks[7] = False
    got = _device_merge(semmap, masks, scores, classes, merge=merge, garbage=True)
    ref = _compare_merge(got, semmap, masks, scores, classes, merge=merge)
    assert np.array_equal(got["rgb"], E.id2rgb(got["panoptic"]))
    assert len(set(scores.tolist())) < 20 and not np.array_equal(H.visiting_order(scores), np.arange(60))
    print("merge %s: %d segments, %d rejected, %d trimmed, %d / %d stuff kept" % (merge, got["count"], ref["rejected"], ref["trimmed"],
          len(ref["kept_stuff"]), len(ref["kept_stuff"]) + len(ref["dropped_stuff"])))
    if merge == (0.1, 1, 0.0):
        assert ref["rejected"] >= 5 and ref["trimmed"] >= 1
    if merge == (0.9, 300, 0.25):
        assert ref["rejected"] >= 5 and ref["trimmed"] >= 5
    if merge == (0.5, 64, 0.55):
        assert 0 < sum(s["isthing"] for s in ref["segments"]) < 59 and ref["kept_stuff"] and ref["dropped_stuff"]


def test_merge_edge_cases():
    semmap, masks, scores, classes = _random_instances(6, 40, 52, 12)
    base = (0.5, 16, 0.55)
    # n == 0 (the masks are there, the device count says none), all scores below the threshold: stuff only
    for got in (_device_merge(semmap, masks, scores, classes, merge=base, n=0), _device_merge(semmap, masks, scores * 0.5, classes, merge=base)):
        ref = _compare_merge(got, semmap, masks[:0], scores[:0], classes[:0], merge=base)
        assert got["count"] > 0 and not any(s["isthing"] for s in ref["segments"])
    got = _device_merge(semmap, masks[:0], scores[:0], classes[:0], merge=base)         # no instance at all
    _compare_merge(got, semmap, masks[:0], scores[:0], classes[:0], merge=base)
    # every colour a thing: no stuff
    got = _device_merge(semmap, masks, scores, classes, n_things=K, merge=(0.5, 0, 0.0), rgb=False)
    ref = _compare_merge(got, semmap, masks, scores, classes, n_things=K, merge=(0.5, 0, 0.0))
    assert all(s["isthing"] for s in ref["segments"]) and (got["panoptic"] == 0).any() and (got["rgb"] == 77).all()          # rgb is optional
    # a ratio exactly equal to the threshold is not rejected: 4 of 8 pixels at 0.5, 1 of 10 at 0.1 (0.1 is no binary fraction:
    # (double)1 / (double)10 is the double 0.1 itself)
    m = np.zeros((3, 8, 16), bool)
    m[0, 0, :8], m[1, 0, 4:12], m[2, 1, :10] = True, True, True
    m[0, 1, 0] = True
    sm = np.full((8, 16), 100, np.int32)
    for thr, kept in ((0.5, 3), (0.49999999999999994, 2), (0.1, 2), (0.09999999999999999, 1)):
        got = _device_merge(sm, m, [0.9, 0.8, 0.7], [1, 2, 3], merge=(thr, 1, 0.0))
        ref = _compare_merge(got, sm, m, [0.9, 0.8, 0.7], [1, 2, 3], merge=(thr, 1, 0.0))
        assert sum(s["isthing"] for s in ref["segments"]) == kept, (thr, ref["segments"])
    # the score threshold compares the float32 score widened to double: float32(0.55) > 0.55 > float32(0.55) - 1 ulp
    f = np.float32(0.55)
    below = np.nextafter(f, np.float32(0))
    assert float(f) > 0.55 > float(below)
    for s, kept in ((f, 1), (below, 0)):
        got = _device_merge(sm, m[:1], [s], [1], merge=(0.5, 1, 0.55))
        _compare_merge(got, sm, m[:1], [s], [1], merge=(0.5, 1, 0.55))
        assert int(got["table"]["isthing"].sum()) == kept


def test_pack_mask_bits_entry_point():
    rng = np.random.default_rng(3)
    masks = rng.random((5, 61, 83)) < 0.3
    assert 61 * 83 == 5063
    src = torch.from_numpy(masks.view(np.uint8) * rng.integers(1, 256, masks.shape).astype(np.uint8)).cuda()          # any non-zero byte
    out = torch.full((5, (5063 + 31) // 32), -1, dtype=torch.int32, device="cuda")
    assert lib.pa_pack_mask_bits(src.data_ptr(), 5, 61, 83, out.data_ptr(), E._stream()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), IH.pack_bits(masks.reshape(5, -1)))


# ---- 4. the routes of `panoptic`
def test_precomputed_instances_route():
    sem, inst = _instances_of("ties_two_thr")
    h, w = sem.shape[:2]
    masks = inst["masks"][:40]
    rng = np.random.default_rng(9)
    order = rng.permutation(40)                                                          # as a detections file has them: unsorted
    masks, scores = masks[order], (rng.integers(2, 16, 40) / 16.0).astype(np.float32)
    # five detections twice: the first copies score 0.9 and are visited early; whatever becomes of one, its second copy (0.3125, still
    # above the threshold) then overlaps the union by at least as much as the first did, or entirely -- so at least 5 are rejected
    assert masks[:5].reshape(5, -1).any(1).all()
    masks, scores = np.concatenate([masks, masks[:5]]), np.concatenate([scores, np.full(5, 0.3125, np.float32)])
    scores[:5] = 0.9
    kw = dict(overlap_threshold=0.3, stuff_area_thresh=100, instances_score_thresh=0.3)
    given = rng.integers(0, T, 45).astype(np.int32)
    for classes in (None, given):
        res = E.panoptic(sem, instances=dict(masks=masks, scores=scores, classes=classes), **kw)
        _check_result(res, h, w)
        ref = H.panoptic(sem, E.semantic_palette(), masks, scores, classes, **kw)
        assert np.array_equal(res["panoptic"], ref["panoptic"]) and np.array_equal(res["classes"], ref["classes"])
        assert np.array_equal(res["areas"], ref["areas"]) and np.array_equal(res["masks"], masks) and np.array_equal(res["scores"], scores)
        _same_segments(res["segments"], ref["segments"])
        assert sum(s["isthing"] for s in ref["segments"]) >= 1 and ref["rejected"] >= 5
    assert not np.array_equal(H.vote(sem, E.semantic_palette(), masks)[1], given)        # given classes do skip the vote
    dev = E.panoptic(torch.from_numpy(sem).cuda(), instances=dict(masks=torch.from_numpy(masks).cuda(), scores=scores, classes=given), **kw)
    assert np.array_equal(dev["panoptic"], res["panoptic"]) and dev["segments"] == res["segments"]
    with pytest.raises(TypeError):
        E.panoptic(sem)
    with pytest.raises(TypeError):
        E.panoptic(sem, sem, instances=dict(masks=masks, scores=scores))
    with pytest.raises(TypeError):
        E.panoptic(sem, sem, nms_iou=0.5)
    with pytest.raises(NotImplementedError):
        E.panoptic(sem, sem, dist_type="cosine")


def test_instance_route_against_the_host_statement_and_all_dist_types():
    name = "odd_size"
    sem, inst = _instances_of(name)
    _, inst_pic = C.decode_pair(name)
    h, w = sem.shape[:2]
    for dist_type in ("abs", "square", "mean"):
        kw = dict(dist_type=dist_type, overlap_threshold=0.2, stuff_area_thresh=150, instances_score_thresh=0.3)
        res = E.panoptic(sem, inst_pic, dist_thr=IC.DECODE[name][3], **kw)
        _check_result(res, h, w)
        assert np.array_equal(res["masks"], inst["masks"]) and np.array_equal(res["scores"], inst["scores"])
        ref = H.panoptic(sem, E.semantic_palette(), inst["masks"], inst["scores"], None, **kw)
        assert np.array_equal(res["panoptic"], ref["panoptic"]) and np.array_equal(res["classes"], ref["classes"])
        _same_segments(res["segments"], ref["segments"])


def test_a_pair_without_instance_candidates_gives_stuff_only():
    sem, _ = C.decode_pair("odd_size")
    h, w = sem.shape[:2]
    res = E.panoptic(sem, np.zeros((h, w, 3), np.uint8), dist_thr=5.0, stuff_area_thresh=100)
    _check_result(res, h, w)
    assert res["scores"].tolist() == [0.0] and res["classes"].tolist() == [0] and res["masks"].shape == (1, h, w) and not res["masks"].any()
    ref = H.panoptic(sem, E.semantic_palette(), np.zeros((1, h, w), bool), [0.0], None, stuff_area_thresh=100)
    assert np.array_equal(res["panoptic"], ref["panoptic"]) and res["segments"] == ref["segments"] and len(ref["segments"]) >= 2


# ---- 5. determinism, other streams
def test_two_runs_give_the_same_bytes_also_beside_a_busy_stream():
    sem, inst = (torch.from_numpy(p).cuda() for p in C.decode_pair("odd_size"))
    merge = dict(dist_type="abs", overlap_threshold=0.2, stuff_area_thresh=150, instances_score_thresh=0.2)

    def launch():
        return E._launch_panoptic(sem, inst, None, None, T, merge, {})
    first = launch()
    ref_out = first.out.clone()
    assert int(ref_out[first.base:first.base + 4].cpu().numpy().view(np.int32)[0]) > 5
    assert torch.equal(launch().out, ref_out)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda", dtype=torch.bfloat16)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):
            a = (a @ a).clamp_(-1, 1)
    beside = launch()
    with torch.cuda.stream(side):                        # and on a stream of its own
        there = launch()
    torch.cuda.synchronize()
    assert torch.equal(beside.out, ref_out) and torch.equal(there.out, ref_out)


# ---- 6. the C ABI
def test_entry_points_refuse_bad_arguments():
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched."""
    p = 256                                            # a non-null, aligned, never dereferenced address
    ok = dict(h=8, w=8, k=133, t=80, dist=0, m=10)
    bad = [dict(h=0), dict(w=0), dict(h=4097, w=4096), dict(k=1025), dict(t=1), dict(t=134), dict(k=1, t=1), dict(m=0), dict(m=1025)]

    def decode(a, ptrs=None, ws=p, thr=(0.5, 8192.0, 0.55)):
        img, pal, masks, sc, n, pan, cnt, seg, cls = ptrs or [p] * 9
        return lib.pa_pano_decode(img, pal, masks, sc, n, 0, a["h"], a["w"], a["k"], a["t"], a["dist"], a["m"], *thr, ws, pan, 0, cnt, seg, cls, 0)

    def merge(a, ptrs=None, ws=p, thr=(0.5, 8192.0, 0.55)):
        sem, masks, sc, cl, n, pan, cnt, seg = ptrs or [p] * 8
        return lib.pa_pano_merge(sem, masks, sc, cl, n, a["h"], a["w"], a["k"], a["t"], a["m"], *thr, ws, pan, 0, cnt, seg, 0)

    def vote(a, ptrs=None):
        img, pal, masks, n, s, cls = ptrs or [p] * 6
        return lib.pa_pano_vote(img, pal, masks, n, a["h"], a["w"], a["k"], a["t"], a["dist"], a["m"], s, cls, 0)

    for change in bad + [dict(dist=3), dict(dist=-1)]:
        a = dict(ok, **change)
        assert decode(a) == INVALID and vote(a) == INVALID, change
        if "dist" not in change:
            assert merge(a) == INVALID and lib.pa_pano_workspace_bytes(a["h"], a["w"], a["k"], a["t"], a["m"]) == -1, change
    for null in range(9):                              # every required pointer (given classes and the rgb picture are optional)
        assert decode(ok, [0 if i == null else p for i in range(9)]) == INVALID, null
    for null in range(8):
        assert merge(ok, [0 if i == null else p for i in range(8)]) == INVALID, null
    for null in range(6):
        assert vote(ok, [0 if i == null else p for i in range(6)]) == INVALID, null
    assert decode(ok, ws=0) == INVALID and merge(ok, ws=0) == INVALID
    assert decode(ok, ws=p + 4) == INVALID and merge(ok, ws=p + 128) == INVALID          # misaligned workspace
    nan = float("nan")
    for thr in ((nan, 1.0, 0.5), (0.5, nan, 0.5), (0.5, 1.0, nan)):
        assert decode(ok, thr=thr) == INVALID and merge(ok, thr=thr) == INVALID
    for src, rows, h, w, out in ((0, 1, 8, 8, p), (p, 1, 8, 8, 0), (p, 0, 8, 8, p), (p, 1025, 8, 8, p), (p, 1, 0, 8, p), (p, 1, 8, 0, p),
                                 (p, 1, 4097, 4096, p)):
        assert lib.pa_pack_mask_bits(src, rows, h, w, out, 0) == INVALID, (src, rows, h, w, out)
    pic = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(RuntimeError, match="pa_pack_mask_bits"):
        E.panoptic(pic, instances=dict(masks=np.zeros((1025, 4, 4), bool), scores=np.zeros(1025)))
    with pytest.raises(RuntimeError, match="pa_pano_decode"):
        E.panoptic(pic, pic, n_things=1)


def test_workspace_stays_near_its_budget():
    for h, w, k, t, m in ((480, 640, 133, 80, 100), (120, 160, 133, 80, 100), (61, 83, 133, 133, 7), (1080, 1920, 1024, 512, 1024)):
        budget = m * t * 8 + h * w * (4 + 1 / 8) + 8 * k + 4 * m + 64          # vote sums, semantic map, union bits; two tables per colour, one per instance
        got = lib.pa_pano_workspace_bytes(h, w, k, t, m)
        print("%dx%d K %d things %d max_inst %d: %d bytes, budget %d" % (h, w, k, t, m, got, budget))
        assert budget / 2 <= got <= 2 * budget


# ---- 7. the engines
@pytest.mark.parametrize("batch_size", [2, 8])
def test_run_panoptic_equals_panoptic_of_the_pictures_run_returns(batch_size):
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70), PC.picture(83, 64, 48)]
    # score threshold 0: every instance is visited, so the first of each picture (nothing pasted yet) is a thing
    kw = dict(dist_thr=[30.0], nms_pre=150, max_num=20, stuff_area_thresh=64, instances_score_thresh=0.0, overlap_threshold=0.4)
    target = PC.picture(PC.PROMPT[0] + 200, PC.PROMPT[1], PC.PROMPT[2], flat=True)      # each engine has its own prompt target

    def engine(task, bs, tgt=None):
        img, own = PC.prompt_pair()
        return E.PainterEngine(PC.StandInModel(), "cuda", task, img, own if tgt is None else tgt, input_size=PC.RES, batch_size=bs)
    sems = engine("coco_pano_semseg", 8).run(pictures)
    insts = engine("coco_pano_inst", 8, target).run(pictures)
    got = E.run_panoptic(engine("coco_pano_semseg", batch_size), engine("coco_pano_inst", batch_size, target), pictures, **kw)
    assert len(got) == 3
    things = 0
    for g, sem, inst in zip(got, sems, insts):
        ref = E.panoptic(sem, inst, **kw)
        _check_result(g, *sem.shape[:2])
        assert sorted(g) == sorted(ref) == ["areas", "classes", "masks", "panoptic", "rgb", "scores", "segments"]
        for k in ref:
            assert g[k] == ref[k] if k == "segments" else np.array_equal(g[k], ref[k]), k
        things += sum(s["isthing"] for s in g["segments"])
    assert things >= 3
    if batch_size == 2:
        mixed = E.run_panoptic(engine("coco_pano_semseg", 3), engine("coco_pano_inst", 2, target), pictures, **kw)          # unequal batches
        assert all(np.array_equal(a["panoptic"], b["panoptic"]) and a["segments"] == b["segments"] for a, b in zip(mixed, got))
        with pytest.raises(ValueError):
            E.run_panoptic(engine("coco_pano_inst", 2), engine("coco_pano_inst", 2), pictures)
        with pytest.raises(ValueError):
            E.run_panoptic(engine("coco_pano_semseg", 2), engine("ade20k_semseg", 2), pictures)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E.panoptic(sems[0], insts[0], device="cpu")
