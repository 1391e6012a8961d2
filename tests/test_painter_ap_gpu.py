"""GPU parity of instance mask AP (csrc/painter_ap.hip through painter_engine.InstanceAP) against tests/painter_ap_host.py -- the
definition, restated from pycocotools' published source and unverified against pycocotools.

The bar: a picture's records equal the statement's as bytes.  Order, areas, matched and ignored bits are integers; the IoUs behind the
bits are correctly rounded quotients of integers, compared with the same threshold doubles."""
import os

import numpy as np
import pytest
import torch

from tests import painter_ap_cases as C
from tests import painter_ap_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

RANGES = C.SMALL_RANGES


def scorer(k=C.K, modes=H.MODES, ranges=RANGES, caps=(1, 1), **kw):
    ap = E.InstanceAP(k, modes, area_ranges=ranges, **kw)
    ap.min_caps = caps
    return ap


def add(ap, pictures, convert=lambda x: x):
    got = ap.add([convert(d["masks"]) for d, _ in pictures], [d["scores"] for d, _ in pictures], [d["classes"] for d, _ in pictures],
                 [convert(g["masks"]) for _, g in pictures], [g["annotations"] for _, g in pictures])
    assert got is ap
    return ap


def statement(pictures, k=C.K, modes=H.MODES, ranges=RANGES, iou_thrs=H.IOU_THRS):
    out = [H.picture_records(d, g, k, modes, iou_thrs, ranges) for d, g in pictures]
    return [r for r, _ in out], [f for _, f in out]


def same(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == H.RECORD and a.tobytes() == b.tobytes(), (i, a, b)


def intersections(ap, picture=0):
    """I of a picture of the last call, read from the workspace where the launch left it."""
    n, d_cap, g_cap = ap._outs[-1][2]
    off = lib.pa_ap_workspace_offset(n, d_cap, g_cap, 0)
    ws = ap._last[4][off:off + 4 * n * d_cap * g_cap].cpu().numpy().view(np.uint32).reshape(n, d_cap, g_cap)
    return ws[picture]


def nothing(h, w):
    return dict(masks=np.zeros((0, h, w), bool), scores=np.zeros(0, np.float32), classes=np.zeros(0, np.int32)), \
        dict(masks=np.zeros((0, h, w), bool), annotations=[])


@pytest.fixture(scope="module")
def odd():
    """61 x 83 = 5063 pixels: 159 words, the last one holds 7 pixels; 7 ground truths (one crowd region), 12 detections, equal scores."""
    pic = C.case(1, 61, 83, 7, 12)
    assert C.not_vacuous(*pic)
    ref, flags = statement([pic])
    assert flags == [0]
    return pic, ref


@pytest.fixture(scope="module")
def mixed():
    pictures = [nothing(1, 1), C.case(31, 1, 300, 2, 3, crowd=0), C.case(32, 300, 1, 4, 2), C.case(33, 9, 7, 3, 0), C.case(34, 9, 7, 0, 5),
                C.case(1, 61, 83, 7, 12)]
    assert len({len(g["annotations"]) for _, g in pictures[1:]} | {len(d["scores"]) for d, _ in pictures[1:]}) >= 7
    ref, flags = statement(pictures)
    assert flags == [0] * 6 and [len(r) for r in ref] == [0, 3, 2, 0, 5, 12]
    return pictures, ref


def test_odd_size_equals_the_statement(odd):
    pic, ref = odd
    ap = add(scorer(), [pic])
    same(ap.records(), ref)
    inter, darea, gpix = H.intersections(*pic)
    assert np.array_equal(intersections(ap)[:12, :7], inter) and inter.max() > 0
    assert np.array_equal(ap.records()[0]["area"], darea[ref[0]["index"]])
    got = ap.result()
    for mode in H.MODES:
        want = H.instance_ap([pic], C.K, mode, area_ranges=RANGES)
        for key, v in want.items():
            assert np.array_equal(np.asarray(got[mode][key]), np.asarray(v)), (mode, key)
    for modes in (("agnostic",), ("per_class",)):                      # a mode that is not asked for leaves its words empty
        same(add(scorer(modes=modes), [pic]).records(), statement([pic], modes=modes)[0])
    # the 25 padding bits of the last word set on both sides: they are no pixels
    d, g = pic
    dbits, gbits = C.bits_of(d["masks"]), C.bits_of(g["masks"])
    dbits[:, -1] |= np.uint32(0xFFFFFF80)
    gbits[:, -1] |= np.uint32(0xFFFFFF80)
    padded = scorer().add([dbits], [d["scores"]], [d["classes"]], [gbits], [g["annotations"]], sizes=[(61, 83)])
    same(padded.records(), ref)


def test_mixed_batch_equals_the_statement(mixed):
    pictures, ref = mixed
    ap = add(scorer(), pictures)
    same(ap.records(), ref)
    res = ap.result()
    want = H.instance_ap(pictures, C.K, "agnostic", area_ranges=RANGES)
    assert all(res["agnostic"][key] == want[key] for key in ("AP", "AP50", "APs", "AR1", "AR100", "ARl"))


def test_tile_edges():
    """9 detections and 9 ground truths: one more than the 8 x 8 pair tile; 2 x 32770: 2049 words, one more than a workgroup's share of
    2048; 100 detections and 93 ground truths at 32 x 40."""
    for pic in (C.case(41, 20, 30, 9, 9), C.case(42, 2, 32770, 2, 3), C.case(43, 32, 40, 93, 100, crowd=2)):
        ref, flags = statement([pic])
        assert flags == [0] and sum(int(r["matched"][:, 0].any()) for r in ref) >= 1
        ap = add(scorer(), [pic])
        same(ap.records(), ref)
        inter = H.intersections(*pic)[0]
        assert np.array_equal(intersections(ap)[:inter.shape[0], :inter.shape[1]], inter)
    # the same with capacities above the tables: the call's tiles beyond a job's own sizes add nothing
    same(add(scorer(caps=(128, 128)), [pic]).records(), ref)


def test_uniform_input():
    """Every mask covers 96 x 128: every I is 12288 and every IoU exactly 1.0, for the crowd ground truth (U = the detection's area) as
    for the other."""
    ones = np.ones((2, 96, 128), bool)
    pic = (dict(masks=ones, scores=np.array([0.5, 0.75], np.float32), classes=np.array([0, 1], np.int32)),
           dict(masks=ones, annotations=[dict(category_id=0, iscrowd=1, area=None), dict(category_id=1, iscrowd=0, area=None)]))
    ref, flags = statement([pic])
    ap = add(scorer(), [pic])
    same(ap.records(), ref)
    assert (intersections(ap)[:2, :2] == 12288).all() and (ap.records()[0]["area"] == 12288).all()
    rec = ap.records()[0]
    T = len(H.IOU_THRS)
    every = np.uint64((1 << T) - 1)                                     # range `all`: matched at every threshold, 0.95 included
    assert (rec["matched"][:, 0] & every == every).all() and rec["index"].tolist() == [1, 0]
    assert rec["ignored"][1, 0] & every == every and rec["ignored"][0, 0] & every == 0        # the second in order gets the crowd region


def test_thresholds():
    """Ten pairs with IoU exactly 10/20 .. 19/20 against the ten thresholds numpy's linspace gives: the matched bits equal the
    statement's, whichever way each comparison falls."""
    gm, dm = np.zeros((10, 10, 24), bool), np.zeros((10, 10, 24), bool)
    for r in range(10):
        gm[r, r, :20] = True
        dm[r, r, :10 + r] = True
    pic = (dict(masks=dm, scores=np.linspace(0.9, 0.1, 10).astype(np.float32), classes=np.zeros(10, np.int32)),
           dict(masks=gm, annotations=[dict(category_id=0, iscrowd=0, area=None) for _ in range(10)]))
    ref, flags = statement([pic])
    bits = [int(w) & 1023 for w in ref[0]["matched"][:, 0]]
    assert bits[0] == 1 and bits[9] in (511, 1023) and all(b in ((1 << r) - 1, (1 << (r + 1)) - 1) for r, b in enumerate(bits))
    ap = add(scorer(), [pic])
    same(ap.records(), ref)
    assert np.array_equal(np.diag(intersections(ap)[:10, :10]), np.arange(10, 20))
    # thresholds of the caller's own, placed on and next to the quotients
    thrs = np.array([11 / 20, np.nextafter(11 / 20, 1), 15 / 20, np.nextafter(15 / 20, 0), 1.0])
    own = E.InstanceAP(C.K, H.MODES, iou_thrs=thrs, area_ranges=RANGES[:2])
    same(add(own, [pic]).records(), statement([pic], ranges=RANGES[:2], iou_thrs=thrs)[0])


def test_two_runs_give_identical_bytes_and_tensors_equal_arrays(mixed):
    pictures, ref = mixed
    a, b = add(scorer(), pictures).records(), add(scorer(), pictures).records()
    same(a, b)
    dev = add(scorer(), pictures, lambda m: torch.from_numpy(m).cuda()).records()
    same(dev, a)
    as_bits = scorer().add([C.bits_of(d["masks"]) for d, _ in pictures], [d["scores"] for d, _ in pictures],
                           [d["classes"] for d, _ in pictures], [g["masks"] for _, g in pictures], [g["annotations"] for _, g in pictures])
    same(as_bits.records(), a)
    d, g = pictures[5]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scorer().add([torch.from_numpy(d["masks"])], [d["scores"]], [d["classes"]], [g["masks"]], [g["annotations"]])


def test_repeated_adds_and_reset(mixed):
    pictures, ref = mixed
    ap = add(scorer(), pictures[:2])
    add(ap, pictures[2:])
    same(ap.records(), ref)
    one = add(scorer(), pictures).result()
    two = ap.result()
    assert all(np.array_equal(np.asarray(one[m][k]), np.asarray(two[m][k])) for m in one for k in one[m])
    ap.reset()
    assert ap.records() == [] and ap.add([], [], [], [], []) is ap and ap.records() == []
    assert ap.result()["agnostic"]["AP"] == -1.0


FLAG_CASES = [(0, dict(scores=np.array([np.nan], np.float32))), (1, dict(classes=np.array([C.K], np.int32))), (2, dict(gt_class=C.K))]


@pytest.mark.parametrize("bit,change", FLAG_CASES)
def test_each_flag_bit_from_its_smallest_input(bit, change):
    one = np.ones((1, 1, 2), bool)
    make = lambda scores=np.array([0.5], np.float32), classes=np.array([0], np.int32), gt_class=0: (
        dict(masks=one, scores=scores, classes=classes), dict(masks=one, annotations=[dict(category_id=gt_class, iscrowd=0, area=None)]))
    pictures = [make(), make(**change), make()]
    ref, flags = statement(pictures)
    assert flags == [0, 1 << bit, 0] and [len(r) for r in ref] == [1, 0, 1]
    ap = add(scorer(), pictures)
    with pytest.raises(ValueError, match=r"picture 1 is refused \(flag bit %d," % bit):
        ap.records()
    with pytest.raises(ValueError, match="picture 1 "):
        ap.result()
    out, at, shape = ap._outs[0]
    a = out.cpu().numpy()
    assert E._section(a, at, "flags").tolist() == flags and E._section(a, at, "counts").tolist() == [1, 0, 1]
    table = E._section(a, at, "records").reshape(shape[0], shape[1])
    same([table[i, :len(ref[i])] for i in range(3)], ref)               # the flagged picture emitted nothing, the others did
    if bit == 1:                                                        # agnostic alone does not read the classes' range
        same(add(scorer(modes=("agnostic",)), pictures).records(), statement(pictures, modes=("agnostic",))[0])


def test_categories_table_maps_data_set_ids(odd):
    pic, ref = odd
    ids = [1000 + 7 * c for c in range(C.K)]
    d, g = pic
    ap = E.InstanceAP(modes=H.MODES, area_ranges=RANGES, categories=ids)
    ap.add([d["masks"]], [d["scores"]], [[ids[c] for c in d["classes"]]], [g["masks"]],
           [[dict(a, category_id=ids[a["category_id"]]) for a in g["annotations"]]])
    same(ap.records(), ref)
    unknown = E.InstanceAP(modes=H.MODES, area_ranges=RANGES, categories=ids).add([d["masks"]], [d["scores"]], [d["classes"]], [g["masks"]],
                                                                                   [g["annotations"]])
    with pytest.raises(ValueError, match="flag bit 1"):
        unknown.records()


def same_result(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key] == b[key] if key == "segments" else np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def test_chained_behind_the_decodes(golden_dir):
    """add_decodes on a launched decode equals add on what was copied back, and the decode's own result is untouched by it."""
    golden = np.load(os.path.join(golden_dir, "painter_pano.npz"))
    sem, inst = golden["defaults.semseg"], golden["defaults.inst"]
    plain = E.instances(inst)
    assert len(plain["scores"]) >= 3
    truth = C.gt_for_instances(11, plain["masks"], None)
    ref, flags = statement([(dict(plain, classes=None), truth)], 80, ("agnostic",), H.AREA_RANGES)
    assert flags == [0] and ref[0]["matched"][:, 0].any()
    ranges = dict(ranges=H.AREA_RANGES)
    copied = scorer(80, ("agnostic",), **ranges).add([plain["masks"]], [plain["scores"]], None, [truth["masks"]], [truth["annotations"]])
    same(copied.records(), ref)
    dec = E.InstanceDecode(torch.from_numpy(inst).cuda(), *E.INSTANCE_DEFAULTS.values())
    chained = scorer(80, ("agnostic",), **ranges).add_decodes([dec], [truth["masks"]], [truth["annotations"]])
    same_result(dec.result(), plain)
    same(chained.records(), ref)
    with pytest.raises(ValueError, match="per_class"):
        scorer(80, **ranges).add_decodes([dec], [truth["masks"]], [truth["annotations"]])
    # behind the panoptic decode: the classes are those of its vote
    kw = dict(overlap_threshold=0.5, stuff_area_thresh=256, instances_score_thresh=0.55)
    pano = E.panoptic(sem, inst, **kw)
    truth = C.gt_for_instances(12, pano["masks"], pano["classes"])
    det = dict(masks=pano["masks"], scores=pano["scores"], classes=pano["classes"])
    ref, flags = statement([(det, truth)], 80, H.MODES, H.AREA_RANGES)
    assert flags == [0] and ref[0]["matched"][:, 1].any() and len(set(pano["classes"].tolist())) >= 2
    copied = scorer(80, **ranges).add([det["masks"]], [det["scores"]], [det["classes"]], [truth["masks"]], [truth["annotations"]])
    same(copied.records(), ref)
    dec = E._launch_panoptic(torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda(), None, None, 80, dict(dist_type="abs", **kw), {})
    chained = scorer(80, **ranges).add_decodes([dec], [truth["masks"]], [truth["annotations"]])
    same_result(dec.result(), pano)
    same(chained.records(), ref)


def test_zero_count_decode_scores_as_one_empty_detection():
    """A black picture is farther than a threshold of 5 from every location colour: the decode's count is 0."""
    black = np.zeros((20, 30, 3), np.uint8)
    dec = E.InstanceDecode(torch.from_numpy(black).cuda(), *dict(E.INSTANCE_DEFAULTS, dist_thr=5.0).values())
    truth = dict(masks=np.ones((1, 20, 30), bool), annotations=[dict(category_id=0, iscrowd=0, area=None)])
    ap = scorer(80, ("agnostic",)).add_decodes([dec], [truth["masks"]], [truth["annotations"]])
    res = dec.result()
    assert int(E._section(dec.out.cpu().numpy(), dec.at, "count")[0]) == 0 and res["candidates"].tolist() == [-1]
    rec = ap.records()
    assert len(rec) == 1 and len(rec[0]) == 1
    assert (rec[0]["score"][0], rec[0]["area"][0], rec[0]["category"][0], rec[0]["index"][0]) == (0.0, 0, 0, 0)
    same(rec, statement([(H.empty_detections(20, 30), truth)], 80, ("agnostic",))[0])
    assert ap.result()["agnostic"]["AP"] == 0.0
    # handed over as what instances() returns for such a picture, it is the same detection
    same(scorer(80, ("agnostic",)).add([res["masks"]], [res["scores"]], None, [truth["masks"]], [truth["annotations"]]).records(), rec)


def test_run_instance_ap_equals_scoring_what_the_runs_return():
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70), PC.picture(83, 64, 48)]
    ikw = dict(dist_thr=[30.0], nms_pre=150, max_num=20)
    kw = dict(ikw, stuff_area_thresh=64, instances_score_thresh=0.0, overlap_threshold=0.4)
    target = PC.picture(PC.PROMPT[0] + 200, PC.PROMPT[1], PC.PROMPT[2], flat=True)

    def engine(task, bs, tgt=None):
        img, own = PC.prompt_pair()
        return E.PainterEngine(PC.StandInModel(), "cuda", task, img, own if tgt is None else tgt, input_size=PC.RES, batch_size=bs)
    # instances alone, agnostic
    results = engine("coco_pano_inst", 8, target).run_instances(pictures, **ikw)
    truths = [C.gt_for_instances(50 + i, r["masks"], None) for i, r in enumerate(results)]
    ref, flags = statement([(dict(r, classes=None), t) for r, t in zip(results, truths)], 80, ("agnostic",), H.AREA_RANGES)
    assert flags == [0, 0, 0] and sum(int(r["matched"][:, 0].any()) for r in ref) >= 1
    gm, ga = [t["masks"] for t in truths], [t["annotations"] for t in truths]
    for bs in (2, 8):
        ap = E.InstanceAP(modes=("agnostic",))
        assert E.run_instance_ap(engine("coco_pano_inst", bs, target), pictures, gm, ga, ap, **ikw) is ap
        same(ap.records(), ref)
    # with the semantic engine: classes from the panoptic decode, both modes
    results = E.run_panoptic(engine("coco_pano_semseg", 8), engine("coco_pano_inst", 8, target), pictures, **kw)
    truths = [C.gt_for_instances(60 + i, r["masks"], r["classes"]) for i, r in enumerate(results)]
    ref, flags = statement([(dict(masks=r["masks"], scores=r["scores"], classes=r["classes"]), t) for r, t in zip(results, truths)], 80, H.MODES,
                           H.AREA_RANGES)
    assert flags == [0, 0, 0] and sum(int(r["matched"][:, 1].any()) for r in ref) >= 1
    gm, ga = [t["masks"] for t in truths], [t["annotations"] for t in truths]
    for bs in (2, 8):
        ap = E.InstanceAP(modes=H.MODES)
        E.run_instance_ap(engine("coco_pano_inst", bs, target), pictures, gm, ga, ap, semseg_engine=engine("coco_pano_semseg", bs), **kw)
        same(ap.records(), ref)
    # wrong tasks, a mode without classes, mismatched lists
    with pytest.raises(ValueError, match="coco_pano_inst"):
        E.run_instance_ap(engine("coco_pano_semseg", 2), pictures, gm, ga, E.InstanceAP())
    with pytest.raises(ValueError, match="coco_pano_semseg"):
        E.run_instance_ap(engine("coco_pano_inst", 2, target), pictures, gm, ga, E.InstanceAP(), semseg_engine=engine("coco_pano_inst", 2, target))
    with pytest.raises(ValueError, match="per_class"):
        E.run_instance_ap(engine("coco_pano_inst", 2, target), pictures, gm, ga, E.InstanceAP(modes=H.MODES))
    with pytest.raises(ValueError, match="3 pictures, 2 lists"):
        E.run_instance_ap(engine("coco_pano_inst", 2, target), pictures, gm[:2], ga, E.InstanceAP())
    with pytest.raises(ValueError, match="annotation lists"):
        E.InstanceAP().add([gm[0]], [np.ones(len(gm[0]), np.float32)], None, [gm[0]], [])
