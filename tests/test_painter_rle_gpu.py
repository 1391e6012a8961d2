"""GPU parity of COCO RLE on the device (csrc/painter_rle.hip through the C ABI of include/painter_rle.h and through
painter_amd/painter_engine.py) against tests/painter_rle_host.py -- the definition, restated from pycocotools' published maskApi.c and
unverified against pycocotools.

The bar: everything is integers and bytes, so everything is equal -- strings, run counts, areas, boxes, offsets, totals, decoded words
(padding bits zero), flags.  No case is skipped or sampled: every shape of tests/painter_rle_cases.py runs in both directions."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import painter_rle_cases as C
from tests import painter_rle_host as H
from tests.guard_bands import abi_symbols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from tests.test_guard_bands_engines_gpu import Ctx, run_case, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [name for name, _ in C.cases()]
POISON = 0xA5


def mask_of(name):
    return dict(C.cases())[name]


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """The statement's encode of a case, computed once."""
    return H.encode_mask(mask_of(name))


@functools.lru_cache(maxsize=None)
def batch_refs():
    return [H.encode_mask(m) for m in C.batch()]


def words_of(h, w):
    return (h * w + 31) // 32


def dirty_bits(masks, n_cap):
    """pack_bits with everything the encode must not read set: the padding bits of the last word and every slot past the masks."""
    n, h, w = masks.shape
    bits = np.full((n_cap, words_of(h, w)), 0xFFFFFFFF, np.uint32)
    bits[:n] = H.pack_bits(masks)
    if h * w % 32:
        bits[:n, -1] |= np.uint32((0xFFFFFFFF << (h * w % 32)) & 0xFFFFFFFF)
    return bits


def encode_direct(c, masks, refs, n_cap=None, count=None, char_cap=None):
    """pa_rle_encode through the C ABI with every buffer at its exact size; char_cap None: exactly the characters of the first `count`
    masks.  Checks header, records, pool against the statement and that nothing else was written.  -> dict of host arrays."""
    n, h, w = masks.shape
    n_cap = n if n_cap is None else n_cap
    count = n if count is None else count
    live = max(0, min(count, n_cap))
    want = [r["counts"].encode("ascii") for r in refs[:live]]
    total = sum(len(s) for s in want)
    char_cap = total if char_cap is None else char_cap
    dbits, dcount = c.dev(dirty_bits(masks, n_cap).view(np.int32), "bits"), c.dev(np.array([count], np.int32), "count")
    nbytes = c.lib.pa_rle_encode_workspace_bytes(h, w, n_cap)
    ws = c.buf(nbytes, torch.uint8, POISON)
    c.holds("pa_rle_encode's workspace", ws, nbytes)
    header = c.buf(4, torch.int64, -1)
    records = c.buf(E.RLE_RECORD.itemsize * n_cap, torch.uint8, POISON)
    pool = c.buf(max(char_cap, 1), torch.uint8, POISON)
    err = c.lib.pa_rle_encode(dbits.data_ptr(), dcount.data_ptr(), h, w, n_cap, ws.data_ptr(), char_cap, header.data_ptr(), records.data_ptr(),
                              pool.data_ptr(), None)
    assert err == 0
    torch.cuda.synchronize()
    header, records, pool = header.cpu().numpy(), records.cpu().numpy().view(E.RLE_RECORD), pool.cpu().numpy()
    assert header.tolist() == [sum(r["runs"] for r in refs[:live]), total, int(total > char_cap), live]
    lengths = np.array([len(s) for s in want], np.int64)
    assert np.array_equal(records["char_count"][:live], lengths) and np.array_equal(records["char_offset"][:live], np.cumsum(lengths) - lengths)
    assert records["runs"][:live].tolist() == [r["runs"] for r in refs[:live]]
    assert records["area"][:live].tolist() == [r["area"] for r in refs[:live]]
    assert records["bbox"][:live].tolist() == [r["bbox"] for r in refs[:live]]
    assert (records[live:].view(np.uint8) == POISON).all()                               # records beyond count are untouched
    if total > char_cap:
        assert (pool == POISON).all()                                                    # overflow: not one byte of the pool
    else:
        assert pool[:total].tobytes() == b"".join(want) and (pool[total:] == POISON).all()          # packed in mask order, nothing past it
    return dict(header=header, records=records[:live], pool=pool)


def decode_direct(c, items, h, w, compressed, spans=None, run_cap=None, pool_len=None):
    """pa_rle_decode through the C ABI, workspace at its exact size.  items: bytes (compressed) or lists of ints -> (bits uint32
    [n][words], flags int32 [n])."""
    n = len(items) if spans is None else len(spans)
    if compressed:
        pool = np.frombuffer(b"".join(items), np.uint8).copy()
    else:
        pool = np.array([v for it in items for v in it], np.uint32)
    lengths = np.array([len(it) for it in items], np.int64)
    if spans is None:
        spans = np.stack([np.cumsum(lengths) - lengths, lengths], 1)
    pool_len = len(pool) if pool_len is None else pool_len
    run_cap = pool_len if run_cap is None else run_cap
    pool = pool if len(pool) else np.zeros(1, pool.dtype)
    dpool = c.dev(pool.view(np.int32) if not compressed else pool, "pool")
    dspans = c.dev(np.ascontiguousarray(spans, dtype=np.int64), "spans")
    nbytes = c.lib.pa_rle_decode_workspace_bytes(n, h, w, run_cap)
    ws = c.buf(nbytes, torch.uint8, POISON)
    c.holds("pa_rle_decode's workspace", ws, nbytes)
    bits = c.buf((n, words_of(h, w)), torch.int32, -1)
    flags = c.buf(n, torch.int32, -1)
    err = c.lib.pa_rle_decode(dpool.data_ptr(), int(compressed), dspans.data_ptr(), n, h, w, pool_len, run_cap, ws.data_ptr(), bits.data_ptr(),
                              flags.data_ptr(), None)
    assert err == 0
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint32), flags.cpu().numpy()


# ---- 1. encode, every case against the statement as bytes
@pytest.mark.parametrize("name", NAMES)
def test_encode_case(name):
    mask, ref = mask_of(name), ref_of(name)
    got = encode_direct(Ctx(), mask[None], [ref])
    assert got["pool"][:len(ref["counts"])].tobytes().decode("ascii") == ref["counts"]


def test_table_strings_come_from_the_device():
    for name, mask, counts, string in C.table():
        rles, areas, boxes = E.rle_encode(np.array(mask[None]))
        assert rles == [{"size": list(mask.shape), "counts": string}] and areas.tolist() == [int(mask.sum())], name


# ---- 2. batches
def test_batch_of_100_slots_37_masks():
    masks, refs = C.batch(), batch_refs()
    runs = [r["runs"] for r in refs]
    assert len(masks) == 37 and min(runs) == 1 and max(runs) > 1000
    a = encode_direct(Ctx(), masks, refs, n_cap=100, count=37)
    b = encode_direct(Ctx(), masks, refs, n_cap=100, count=37)                          # two runs give identical bytes
    same_bytes("batch", a, b)
    roomy = encode_direct(Ctx(), masks, refs, n_cap=100, count=37, char_cap=int(a["header"][1]) + 1000)
    assert roomy["pool"][:int(a["header"][1])].tobytes() == a["pool"][:int(a["header"][1])].tobytes()


def test_count_beyond_the_slots_is_clamped():
    masks, refs = C.batch(), batch_refs()
    got = encode_direct(Ctx(), masks, refs, n_cap=37, count=1000)
    assert got["header"][3] == 37
    assert encode_direct(Ctx(), masks, refs, n_cap=37, count=-5)["header"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("count", [0, 1])
def test_count_0_and_1(count):
    masks, refs = C.batch(), batch_refs()
    got = encode_direct(Ctx(), masks[3:12], refs[3:12], n_cap=9, count=count)
    assert got["header"][3] == count and len(got["records"]) == count


# ---- 3. overflow
def test_overflow_reports_exact_totals_and_writes_no_character():
    masks, refs = C.batch(), batch_refs()
    total = sum(len(r["counts"]) for r in refs)
    for cap in (0, 1, total - 1):
        got = encode_direct(Ctx(), masks, refs, char_cap=cap)
        assert got["header"].tolist()[1:3] == [total, 1]


def test_checkerboard_batch_takes_the_second_launch():
    board = C.checkerboard(48, 64)
    masks = np.stack([board, ~board, board, board, ~board])
    refs = [H.encode_mask(m) for m in masks[:2]]
    refs = [refs[0], refs[1], refs[0], refs[0], refs[1]]
    total = sum(len(r["counts"]) for r in refs)
    assert refs[0]["runs"] == 48 * 64 - 63 and total > E.rle_default_chars(64, 5)
    bits = torch.from_numpy(H.pack_bits(masks).view(np.int32)).cuda()
    count = torch.tensor([5], dtype=torch.int32, device="cuda")
    enc = E.RleEncode(bits, count, 48, 64, 5)
    _, header = enc._head()
    assert header["overflow"] == 1 and header["chars"] == total and header["runs"] == sum(r["runs"] for r in refs) and enc.launches == 1
    res = enc.result()
    assert enc.launches == 2 and enc.char_cap == total and res["header"]["overflow"] == 0
    assert res["strings"] == [r["counts"] for r in refs]
    exact = E.RleEncode(bits, count, 48, 64, 5, char_cap=total)
    res2 = exact.result()
    assert exact.launches == 1 and res2["pool"].tobytes() == res["pool"].tobytes() and res2["records"].tobytes() == res["records"].tobytes()


# ---- 4. decode
@pytest.mark.parametrize("name", NAMES)
def test_decode_case(name):
    mask, ref = mask_of(name), ref_of(name)
    h, w = mask.shape
    want = H.pack_bits(mask[None])                                                       # padding bits of the last word are zero
    bits, flags = decode_direct(Ctx(), [ref["counts"].encode("ascii")], h, w, True)
    assert flags.tolist() == [0] and np.array_equal(bits, want)
    bits, flags = decode_direct(Ctx(), [ref["cnts"]], h, w, False)
    assert flags.tolist() == [0] and np.array_equal(bits, want)


def test_decode_batch_and_zero_counts_inside():
    masks, refs = C.batch(), batch_refs()
    h, w = masks.shape[1:]
    bits, flags = decode_direct(Ctx(), [r["counts"].encode("ascii") for r in refs], h, w, True)
    assert not flags.any() and np.array_equal(bits, H.pack_bits(masks))
    again, _ = decode_direct(Ctx(), [r["counts"].encode("ascii") for r in refs], h, w, True)
    assert again.tobytes() == bits.tobytes()
    cnts = [10, 0, 0, 5, 0, 7, h * w - 22]                                               # legal for maskApi.c: runs of no pixels
    assert H.check(cnts, h, w) == 0 and H.check(H.to_string(cnts), h, w) == 0
    want = H.pack_bits(H.decode(cnts, h, w)[None])
    for items, compressed in (([H.to_string(cnts)], True), ([cnts], False)):
        bits, flags = decode_direct(Ctx(), items, h, w, compressed)
        assert flags.tolist() == [0] and np.array_equal(bits, want)


def malformed_batch(c, h=9, w=7):
    """Every malformed string between two good neighbours, then the flags that come from the spans and the workspace.  -> dict."""
    bad = [m for m in C.malformed(h, w)]
    good_mask = np.zeros((h, w), bool)
    good_mask[2:5, 1:4] = True
    good = H.to_string(H.encode(good_mask))
    want_good = H.pack_bits(good_mask[None])[0]
    out = {}
    for compressed in (True, False):
        these = [(n, s, f) for n, s, f in bad if isinstance(s, bytes) == compressed]
        ok = good if compressed else H.encode(good_mask)
        items, want = [ok], [0]
        for _, s, f in these:
            items += [s, ok]
            want += [f, 0]
            assert H.check(s, h, w) == f
        bits, flags = decode_direct(c, items, h, w, compressed)
        assert flags.tolist() == want, (flags.tolist(), want)
        for i, f in enumerate(want):
            assert np.array_equal(bits[i], want_good) if f == 0 else not bits[i].any(), i          # refused: bits zero; neighbours decode
        out["bits%d" % compressed], out["flags%d" % compressed] = bits, flags
    assert {f for _, _, f in bad} == {1, 2, 3, 4, 7}
    # 5: the workspace holds fewer runs than the pool has elements -- the masks beyond it are refused, the ones inside decode
    items = [good, good, good]
    bits, flags = decode_direct(c, items, h, w, True, run_cap=2 * len(good) + 1)
    assert flags.tolist() == [0, 0, 5] and np.array_equal(bits[1], want_good) and not bits[2].any()
    out["bits5"], out["flags5"] = bits, flags
    # 6: spans that do not lie inside the pool
    n = len(good)
    spans = np.array([[0, n], [-1, n], [n, n], [2 * n, n + 1], [3 * n + 1, 0], [2 * n, n], [1 << 40, 1]], np.int64)
    bits, flags = decode_direct(c, items, h, w, True, spans=spans)
    assert flags.tolist() == [0, 6, 0, 6, 6, 0, 6] and not bits[[1, 3, 4, 6]].any() and all(np.array_equal(bits[i], want_good) for i in (0, 2, 5))
    out["bits6"], out["flags6"] = bits, flags
    return out


def test_malformed_masks_are_refused_and_their_neighbours_decode():
    a = malformed_batch(Ctx())
    b = malformed_batch(Ctx())
    same_bytes("malformed", a, b)


# ---- 5. through painter_engine
def engine_round_trip(c=None):
    c = c or Ctx()
    masks, refs = C.batch(), batch_refs()
    n, h, w = masks.shape
    rles, areas, boxes = E.rle_encode(c.dev(masks.view(np.uint8), "masks"))
    assert rles == [{"size": [h, w], "counts": r["counts"]} for r in refs]
    assert areas.tolist() == [r["area"] for r in refs] and boxes.tolist() == [[float(v) for v in r["bbox"]] for r in refs]
    assert boxes.dtype == np.float64 and areas.dtype == np.int64
    bits = E.rle_decode(rles)
    assert bits.dtype == torch.int32 and bits.is_cuda and np.array_equal(bits.cpu().numpy().view(np.uint32), H.pack_bits(masks))
    from_bits, _, _ = E.rle_encode(c.dev(H.pack_bits(masks).view(np.int32), "bits"), size=(h, w))
    assert from_bits == rles
    mixed = [dict(r, counts=ref["cnts"]) if i % 3 == 0 else dict(r, counts=r["counts"].encode("ascii")) if i % 3 == 1 else r
             for i, (r, ref) in enumerate(zip(rles, refs))]
    both = E.rle_decode(mixed)
    assert torch.equal(both, bits)
    return dict(bits=bits, both=both, areas=areas, boxes=boxes, strings=np.frombuffer("".join(r["counts"] for r in rles).encode(), np.uint8))


def test_rle_encode_and_rle_decode():
    engine_round_trip()
    masks = np.array(C.batch())                                                          # (a writable copy: torch.from_numpy warns otherwise)
    assert E.rle_encode(masks[:4])[0] == E.rle_encode(masks[:4].astype(np.uint8))[0] == E.rle_encode(torch.from_numpy(masks[:4].copy()).cuda())[0]
    json.dumps(E.rle_encode(masks[:2])[0])                                               # what the evaluator dumps
    h, w = masks.shape[1:]
    good = E.rle_encode(masks[:3])[0]
    for name, counts, flag in C.malformed(h, w):
        with pytest.raises(ValueError, match=r"mask 1 is refused \(flag bit %d" % flag):
            E.rle_decode([good[0], {"size": [h, w], "counts": counts}, good[2]])
    with pytest.raises(ValueError, match="one size"):
        E.rle_decode([good[0], {"size": [w, h], "counts": good[1]["counts"]}])
    with pytest.raises(ValueError, match="non-empty"):
        E.rle_decode([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rle_encode(torch.from_numpy(masks[:2].copy()))


# ---- 6. end to end on the fixtures
@pytest.fixture(scope="module")
def inst_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_inst.npz"))


@pytest.fixture(scope="module")
def pano_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_pano.npz"))


def check_entries(entries, inst, image_id, categories):
    n, h, w = inst["masks"].shape
    assert len(entries) == n
    for e, score, mask, cat in zip(entries, inst["scores"], inst["masks"], categories):
        assert sorted(e) == ["bbox", "category_id", "image_id", "score", "segmentation"]
        assert e["image_id"] == image_id and e["category_id"] == cat and type(e["category_id"]) is int and e["bbox"] == [0.0, 0.0, 0.0, 0.0]
        assert type(e["score"]) is float and e["score"] == float(score)
        seg = e["segmentation"]
        assert seg["size"] == [h, w] and type(seg["counts"]) is str
        assert np.array_equal(H.decode(H.from_string(seg["counts"]), h, w), mask)
    json.dumps(entries)


def instance_results_of(c, pic, thr, image_id=42):
    dec = E.InstanceDecode(c.dev(pic, "picture"), None, thr, 2000, 100, "gaussian", 2.0)
    job = E.InstanceResults(dec, image_id)
    entries = job.result()
    return dec, job, entries


def test_instance_results_of_the_instance_fixture(inst_golden):
    from tests import painter_inst_cases as IC
    for name in IC.FIXTURE:
        pic, thr = inst_golden[name + ".picture"], [float(t) for t in inst_golden[name + ".thresholds"]]
        dec, job, entries = instance_results_of(Ctx(), pic, thr)
        inst = dec.result()
        assert len(inst["scores"]) == 100
        check_entries(entries, inst, 42, [1] * 100)
        assert job.encode.launches == 1                                                  # ordinary masks fit the default pool
        assert E.instance_results(dec, "again") == [dict(e, image_id="again") for e in entries]


def test_rle_dicts_feed_panoptic_classify_and_instance_ap(pano_golden):
    from tests import painter_ap_cases as AC
    from tests import painter_pano_cases as PC
    for name in PC.FIXTURE:
        _, h, w, thr, merge, _ = PC.FIXTURE[name]
        sem, inst = pano_golden[name + ".semseg"], pano_golden[name + ".inst"]
        kw = dict(overlap_threshold=merge[0], stuff_area_thresh=merge[1], instances_score_thresh=merge[2])
        dec = E._launch_panoptic(torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda(), None, None, 80, dict(dist_type="abs", **kw),
                                 dict(dist_thr=thr))
        entries = E.instance_results(dec, name)
        pano = dec.result()
        check_entries(entries, pano, name, pano["classes"].tolist())
        assert len(set(pano["classes"].tolist())) >= 2
        rles = [e["segmentation"] for e in entries]
        scores = [e["score"] for e in entries]
        dense = E.panoptic(sem, instances=dict(masks=pano["masks"], scores=pano["scores"]), **kw)
        from_rle = E.panoptic(sem, instances=dict(masks=rles, scores=scores), **kw)
        assert from_rle["masks"] is rles
        for key in ("panoptic", "classes", "scores", "rgb", "areas"):
            assert np.array_equal(dense[key], from_rle[key]) and dense[key].dtype == from_rle[key].dtype, key
        assert dense["segments"] == from_rle["segments"] and len(dense["segments"]) >= 2
        assert np.array_equal(E.classify_instances(sem, rles), E.classify_instances(sem, pano["masks"]))
    # InstanceAP with RLE ground truth (the last pair): crowd regions as uncompressed counts, the others as strings
    truth = AC.gt_for_instances(12, pano["masks"], pano["classes"])
    assert len(truth["masks"]) >= 2
    gt_rles = [{"size": [h, w], "counts": H.encode_fast(m) if a.get("iscrowd") else H.encode_mask(m)["counts"]}
               for m, a in zip(truth["masks"], truth["annotations"])]
    want = E.InstanceAP(80, ("agnostic", "per_class")).add([pano["masks"]], [pano["scores"]], [pano["classes"]], [truth["masks"]],
                                                           [truth["annotations"]]).records()
    got = E.InstanceAP(80, ("agnostic", "per_class")).add([pano["masks"]], [pano["scores"]], [pano["classes"]], [gt_rles],
                                                          [truth["annotations"]]).records()
    both = E.InstanceAP(80, ("agnostic", "per_class")).add([rles], [pano["scores"]], [pano["classes"]], [gt_rles], [truth["annotations"]]).records()
    assert len(want) == 1 and want[0].tobytes() == got[0].tobytes() == both[0].tobytes() and want[0]["matched"].any()
    with pytest.raises(ValueError, match="ground truth"):
        E.InstanceAP(80).add([pano["masks"]], [pano["scores"]], None, [[dict(g, size=[w, h]) for g in gt_rles]], [truth["annotations"]])


def empty_prediction(c=None):
    c = c or Ctx()
    dec, job, entries = instance_results_of(c, np.zeros((37, 53, 3), np.uint8), [5.0], image_id=7)
    assert entries == [dict(image_id=7, category_id=0, bbox=[0.0, 0.0, 0.0, 0.0], score=0.0,
                            segmentation={"size": [37, 53], "counts": H.to_string([37 * 53]).decode("ascii")})]
    return dict(count=job.encode.result()["header"])


def test_the_empty_prediction_gives_the_single_zero_entry():
    got = empty_prediction()
    assert got["count"]["count"] == 0 and got["count"]["chars"] == 0
    sem = np.zeros((37, 53, 3), np.uint8)
    dec = E._launch_panoptic(torch.from_numpy(sem).cuda(), torch.from_numpy(sem).cuda(), None, None, 80, dict(dist_type="abs"), dict(dist_thr=5.0))
    assert E.instance_results(dec, 7)[0]["category_id"] == 0 and len(E.instance_results(dec, 7)) == 1


def test_run_instance_results_equals_the_runs():
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70), PC.picture(83, 64, 48)]
    ids = [101, "b", 103]
    ikw = dict(dist_thr=[30.0], nms_pre=150, max_num=20)
    kw = dict(ikw, stuff_area_thresh=64, instances_score_thresh=0.0, overlap_threshold=0.4)
    target = PC.picture(PC.PROMPT[0] + 200, PC.PROMPT[1], PC.PROMPT[2], flat=True)

    def engine(task, bs, tgt=None):
        img, own = PC.prompt_pair()
        return E.PainterEngine(PC.StandInModel(), "cuda", task, img, own if tgt is None else tgt, input_size=PC.RES, batch_size=bs)
    results = engine("coco_pano_inst", 8, target).run_instances(pictures, **ikw)
    for bs in (2, 8):
        flat = E.run_instance_results(engine("coco_pano_inst", bs, target), pictures, ids, **ikw)
        at = 0
        for r, image_id in zip(results, ids):
            check_entries(flat[at:at + len(r["scores"])], r, image_id, [int(v) for v in r["labels"]])
            at += len(r["scores"])
        assert at == len(flat)
    pano = E.run_panoptic(engine("coco_pano_semseg", 8), engine("coco_pano_inst", 8, target), pictures, **kw)
    flat = E.run_instance_results(engine("coco_pano_inst", 2, target), pictures, ids, semseg_engine=engine("coco_pano_semseg", 2), **kw)
    at = 0
    for r, image_id in zip(pano, ids):
        check_entries(flat[at:at + len(r["scores"])], r, image_id, r["classes"].tolist())
        at += len(r["scores"])
    assert at == len(flat)
    with pytest.raises(ValueError, match="coco_pano_inst"):
        E.run_instance_results(engine("coco_pano_semseg", 2), pictures, ids)
    with pytest.raises(ValueError, match="3 pictures, 2 image ids"):
        E.run_instance_results(engine("coco_pano_inst", 2, target), pictures, ids[:2])
    with pytest.raises(TypeError):
        E.run_instance_results(engine("coco_pano_inst", 2, target), pictures, ids, nms_iou=0.5)


# ---- 7. guard bands: exact-size workspaces and pools between 4 MiB of 0xFF, results byte-identical to the ordinary run
def _guard_encode(c):
    return encode_direct(c, C.batch(), batch_refs(), n_cap=41, count=37)


def _guard_encode_overflow(c):
    return encode_direct(c, C.batch(), batch_refs(), char_cap=100)


def _guard_encode_wide(c):
    return encode_direct(c, mask_of("wide-3x2500")[None], [ref_of("wide-3x2500")])


def _guard_instance_results(c):
    pic = np.load(os.path.join(ROOT, "tests", "golden", "painter_inst.npz"))["thr19_c.picture"]
    dec, job, entries = instance_results_of(c, pic, [19.0])
    text = json.dumps(entries).encode()
    empty = empty_prediction(c)
    return dict(text=np.frombuffer(text, np.uint8), out=job.encode.out[:job.encode.at["pool"][0] + int(job.encode.result()["header"]["chars"])],
                empty=np.array(empty["count"].tolist()))


GUARD_CASES = [
    ("encode-exact-capacity-41-slots-37-masks", _guard_encode, [], ("pa_rle_encode", "pa_rle_encode_workspace_bytes")),
    ("encode-overflow-writes-no-character", _guard_encode_overflow, [], ("pa_rle_encode",)),
    ("encode-more-columns-than-a-scan-chunk", _guard_encode_wide, [], ("pa_rle_encode",)),
    ("decode-malformed-batch", malformed_batch, [], ("pa_rle_decode", "pa_rle_decode_workspace_bytes")),
    ("engine-rle_encode-rle_decode", engine_round_trip, ["painter_engine"],
     ("pa_rle_encode", "pa_rle_encode_workspace_bytes", "pa_rle_decode", "pa_rle_decode_workspace_bytes")),
    ("engine-instance_results", _guard_instance_results, ["painter_engine"], ("pa_inst_decode", "pa_rle_encode", "pa_rle_encode_workspace_bytes")),
]


@pytest.mark.parametrize("fn,modules,symbols", [pytest.param(f, m, s, id=i) for i, f, m, s in GUARD_CASES])
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, tuple(modules), tuple(symbols), monkeypatch)


def test_every_symbol_of_the_rle_header_is_guarded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_rle.h")).read())
    assert abi == {"pa_rle_encode", "pa_rle_encode_workspace_bytes", "pa_rle_decode", "pa_rle_decode_workspace_bytes"}
    claimed = set()
    for _, _, _, symbols in GUARD_CASES:
        claimed |= {s for s in symbols if s.startswith("pa_rle_")}
    helpers = {s for s in abi if s.endswith("_workspace_bytes")}                         # host only: size helpers; their cases allocate exactly what they return
    assert abi - claimed == set() and helpers <= claimed
