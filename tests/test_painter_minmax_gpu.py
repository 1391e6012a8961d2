"""GPU parity of the nearest-colour (minmax) instance decode (csrc/painter_minmax.hip through the C ABI of include/painter_minmax.h and
through painter_amd/painter_engine.py) against tests/painter_minmax_host.py -- the definition -- and against the fixture the unmodified
reference produced (tests/golden/painter_minmax.npz).

The bar: everything is integers, so everything is compared with np.array_equal.  The one float32 comparison, the score, is equality too:
both sides do the same three correctly rounded operations (float64 division rounded to float32, float32 division, float32 subtraction)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import painter_minmax_cases as C
from tests import painter_minmax_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from tests.test_guard_bands_engines_gpu import Ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
NAMES = list(C.FIXTURE) + list(C.DECODE)


def up16(x):
    return -(-x // 16) * 16


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "painter_minmax.npz"))


@functools.lru_cache(maxsize=None)
def default_palette():
    from painter_amd.painter_engine import location_palette
    pal = H.with_background(location_palette())
    pal.setflags(write=False)
    return pal


@functools.lru_cache(maxsize=None)
def case(name):
    """(picture, the statement's decode of it with the default palette), computed once and never modified."""
    pic = C.fixture_picture(name) if name in C.FIXTURE else C.decode_picture(name)
    return pic, H.decode(pic, default_palette())


def direct(c, pic, pal, want, first=0, n_cap=None):
    """pa_minmax_decode, pa_minmax_nearest and pa_minmax_masks through the C ABI with every buffer at its exact size.  Checks every output
    against the statement's decode `want` and that nothing past the count was written.  -> dict of host arrays."""
    h, w = pic.shape[:2]
    k, hw, words = len(pal), h * w, (h * w + 31) // 32
    img, dpal = c.dev(pic, "picture"), c.dev(np.asarray(pal, np.float32), "palette")
    nbytes = c.lib.pa_minmax_workspace_bytes(h, w, k)
    ws = c.buf(nbytes, torch.uint8, POISON)
    c.holds("pa_minmax_decode's workspace", ws, nbytes)
    label, dist = c.buf(hw, torch.int16, -1), c.buf(hw, torch.int16, -1)
    count, records, slot = c.buf(1, torch.int32, -1), c.buf(H.RECORD.itemsize * k, torch.uint8, POISON), c.buf(k, torch.int32, -7)
    assert c.lib.pa_minmax_decode(img.data_ptr(), dpal.data_ptr(), h, w, k, ws.data_ptr(), label.data_ptr(), dist.data_ptr(), count.data_ptr(),
                                  records.data_ptr(), slot.data_ptr(), None) == 0
    label2, dist2 = c.buf(hw, torch.int16, -1), c.buf(hw, torch.int16, -1)
    assert c.lib.pa_minmax_nearest(img.data_ptr(), dpal.data_ptr(), h, w, k, label2.data_ptr(), dist2.data_ptr(), None) == 0
    torch.cuda.synchronize()
    n = int(count.cpu()[0])
    out = dict(label=label.cpu().numpy().view(np.uint16), dist=dist.cpu().numpy().view(np.uint16), count=np.array([n]),
               records=records.cpu().numpy(), slot=slot.cpu().numpy(), ws=ws.cpu().numpy())
    assert np.array_equal(out["label"], want["label"].ravel()) and np.array_equal(out["dist"], want["dist"].ravel())
    assert np.array_equal(label2.cpu().numpy(), label.cpu().numpy()) and np.array_equal(dist2.cpu().numpy(), dist.cpu().numpy())
    assert np.array_equal(out["ws"][:8 * k].view(np.uint64), want["S"]) and np.array_equal(out["ws"][up16(8 * k):][:4 * k].view(np.uint32), want["n"])
    assert n == want["count"]
    rec = out["records"].view(H.RECORD)
    assert rec[:n].tobytes() == want["records"].tobytes()                                  # colour, class, n, S, neg and score: every bit
    assert np.array_equal(rec[:n]["score"], want["scores"]) and np.array_equal(rec[:n]["cls"], want["classes"])
    assert (out["records"][H.RECORD.itemsize * n:] == POISON).all()                        # records beyond the count are untouched
    assert np.array_equal(out["slot"], want["slot"])
    n_cap = n - first if n_cap is None else n_cap
    bits, dense = c.buf((n_cap, words), torch.int32, -1), c.buf((n_cap, hw), torch.uint8, POISON)
    bits_only = c.buf((n_cap, words), torch.int32, -1)
    assert c.lib.pa_minmax_masks(label.data_ptr(), slot.data_ptr(), h, w, k, first, n_cap, bits.data_ptr(), dense.data_ptr(), None) == 0
    assert c.lib.pa_minmax_masks(label.data_ptr(), slot.data_ptr(), h, w, k, first, n_cap, bits_only.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    masks = H.masks_of(want["label"], want["slot"], first, n_cap).reshape(n_cap, hw)
    out["bits"], out["bytes"] = bits.cpu().numpy().view(np.uint32), dense.cpu().numpy()
    assert np.array_equal(out["bits"], H.pack_bits(masks)) and np.array_equal(out["bytes"], masks.astype(np.uint8))
    assert np.array_equal(bits_only.cpu().numpy().view(np.uint32), out["bits"])
    return out


def check_result(res, want, h, w):
    """What `instances_minmax` / `MinmaxDecode.result()` return against the statement."""
    assert sorted(res) == ["areas", "candidates", "dist_map", "labels", "masks", "pred_map", "scores"]
    n = want["count"]
    assert res["scores"].dtype == np.float32 and res["scores"].tobytes() == want["scores"].tobytes()
    assert res["labels"].dtype == np.float32 and np.array_equal(res["labels"], want["classes"].astype(np.float32))
    assert res["candidates"].dtype == np.int32 and np.array_equal(res["candidates"], want["candidates"])
    assert res["areas"].dtype == np.int32 and np.array_equal(res["areas"], want["areas"])
    assert res["pred_map"].dtype == np.int32 and res["pred_map"].shape == (h, w) and np.array_equal(res["pred_map"], want["label"])
    assert res["dist_map"].dtype == np.float32 and res["dist_map"].shape == (h, w) and np.array_equal(res["dist_map"], want["dist"].astype(np.float32))
    assert res["masks"].dtype == np.bool_ and res["masks"].shape == (n, h, w)
    assert np.array_equal(res["masks"], H.masks_of(want["label"], want["slot"]))


# ---- 1. the fixture and a second set, with the default palette: K + 1 = 6401, no multiple of the four-colour read
@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_the_statement_and_the_reference(name):
    pic, want = case(name)
    h, w = pic.shape[:2]
    direct(Ctx(), pic, default_palette(), want)
    res = E.instances_minmax(pic)
    check_result(res, want, h, w)
    if name in C.FIXTURE:                                                   # the unmodified reference's own arrays
        g = golden()
        assert np.array_equal(pic, g[name + ".picture"])
        assert np.array_equal(res["pred_map"], g[name + ".pred_map"]) and np.array_equal(res["dist_map"], g[name + ".dist_map"].astype(np.float32))
        assert res["scores"].tobytes() == g[name + ".scores"].tobytes() and np.array_equal(res["labels"], g[name + ".classes"].astype(np.float32))
        assert np.array_equal(res["candidates"], np.unique(g[name + ".pred_map"]))


def test_the_fixture_has_tied_pixels_and_many_instances():
    assert case("thr19_a")[1]["ties"] == int(golden()["thr19_a.ties"]) == 2 and case("thr19_a")[1]["count"] == 683


# ---- 2. constructed pictures
def test_ties_go_to_the_lowest_index():
    pic, pal = C.ties_case()
    want = H.decode(pic, pal)
    assert want["ties"] >= 40 and 3 not in want["candidates"]
    out = direct(Ctx(), pic, pal, want)
    assert out["label"].reshape(8, 8)[:5, 0].tolist() == [1, 1, 1, 1, 0] and out["slot"][3] == -1
    check_result(E.instances_minmax(pic, palette=pal[:-1]), want, 8, 8)
    sub = direct(Ctx(), pic, pal, want, first=1, n_cap=2)                   # a window of slots; a window past the last slot stays empty
    assert np.array_equal(sub["bits"], out["bits"][1:3])
    past = Ctx()
    label, slot = past.dev(want["label"].astype(np.int16).ravel()), past.dev(want["slot"])
    bits = past.buf((3, 2), torch.int32, -1)
    assert past.lib.pa_minmax_masks(label.data_ptr(), slot.data_ptr(), 8, 8, 5, want["count"] - 1, 3, bits.data_ptr(), None, None) == 0
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), np.concatenate([out["bits"][-1:], np.zeros((2, 2), np.uint32)]))


def test_one_pixel():
    pic = np.array([[[7, 200, 90]]], np.uint8)
    for pal in (default_palette(), H.with_background([[7, 200, 91]])):
        want = H.decode(pic, pal)
        assert want["count"] == 1
        direct(Ctx(), pic, pal, want)
        check_result(E.instances_minmax(pic, palette=pal[:-1]), want, 1, 1)


def test_all_black_is_one_background_instance_with_score_one():
    pic = np.zeros((37, 53, 3), np.uint8)
    want = H.decode(pic, default_palette())
    out = direct(Ctx(), pic, default_palette(), want)
    rec = out["records"].view(H.RECORD)[0]
    assert out["count"][0] == 1 and rec["colour"] == 6400 and rec["cls"] == 0 and rec["n"] == 37 * 53 and rec["S"] == 0
    assert rec["neg"] == 0 and rec["score"] == 1.0
    res = E.instances_minmax(pic)
    assert res["scores"].tolist() == [1.0] and res["labels"].tolist() == [0.0] and res["masks"].all()


def test_exact_palette_colours_score_exactly_one():
    pal = default_palette()
    pic = C.exact_colours_case(pal)
    want = H.decode(pic, pal)
    assert want["count"] == 7 and not want["dist"].any()
    out = direct(Ctx(), pic, pal, want)
    assert (out["records"].view(H.RECORD)[:7]["score"] == 1.0).all()           # the max(., 1) branch: 1 - 0 / 1
    res = E.instances_minmax(pic)
    assert (res["scores"] == 1.0).all() and len(res["scores"]) == 7


def test_a_palette_at_the_capacity():
    pic, pal = C.capacity_case()
    assert len(pal) == 16384
    want = H.decode(pic, pal)
    assert {16382, 16383} <= set(want["candidates"].tolist()) and want["count"] > 100
    direct(Ctx(), pic, pal, want)
    check_result(E.instances_minmax(pic, palette=pal[:-1]), want, 16, 16)
    with pytest.raises(RuntimeError, match="pa_minmax_decode"):
        E.instances_minmax(pic, palette=np.zeros((16384, 3), np.float32))      # 16385 rows with the background


def test_two_rows_and_6401_rows():
    pic = C.decode_picture("odd_37x53")
    pal = H.with_background([[250, 240, 230]])                                 # K + 1 = 2
    want = H.decode(pic, pal)
    assert want["count"] == 2 and want["classes"].tolist() == [1, 0]
    direct(Ctx(), pic, pal, want)
    check_result(E.instances_minmax(pic, palette=pal[:-1]), want, 37, 53)
    assert len(default_palette()) == 6401 and 6401 % 4 == 1                    # (test 1 runs every case at 6401)
    last = np.tile(default_palette()[6399].astype(np.uint8), (3, 5, 1))        # the row before the background, in the last partial read
    want = H.decode(last, default_palette())
    assert want["candidates"].tolist() == [6399]
    direct(Ctx(), last, default_palette(), want)


# ---- 3. sums beyond 2^24 and 2^32 are carried exactly (against the statement alone: the reference's float32 sums are not exact there)
def constant_case(colour, h, w, pal):
    pic = np.empty((h, w, 3), np.uint8)
    pic[:] = colour
    return pic, H.decode(pic, pal, maps=H.constant_nearest(colour, h, w, pal))


def test_a_sum_beyond_2_to_24():
    pal = H.with_background([[130, 140, 140], [90, 255, 0], [255, 255, 30]])
    pic, want = constant_case((200, 200, 200), 512, 512, pal)
    assert want["count"] == 1 and int(want["S"][0]) == 190 * 512 * 512 > 1 << 24
    out = direct(Ctx(), pic, pal, want)
    assert out["records"].view(H.RECORD)[0]["neg"] == 190.0 and out["records"].view(H.RECORD)[0]["score"] == 0.0


def test_a_sum_beyond_2_to_32():
    """765 is the largest distance there is, so the background row can only tie with row 0; the lower index keeps every pixel."""
    pal = H.with_background([[0, 0, 0]])
    pic, want = constant_case((255, 255, 255), 4096, 4096, pal)
    assert want["count"] == 1 and int(want["S"][0]) == 765 << 24 > 1 << 32 and want["candidates"].tolist() == [0]
    dec = E.MinmaxDecode(torch.from_numpy(pic).cuda(), pal[:-1])
    a = dec.out.cpu().numpy()
    rec = E._section(a, dec.at, "records", 1)
    assert dec.count() == 1 and rec.tobytes() == want["records"].tobytes() and int(rec["S"][0]) == 765 << 24 and rec["n"][0] == 1 << 24
    assert (E._section(a, dec.at, "label") == 0).all() and (E._section(a, dec.at, "dist") == 765).all()
    assert np.array_equal(E._section(a, dec.at, "slot"), want["slot"])
    bits, dense, n = dec.bits(with_bytes=True)
    assert n == 1 and bool((bits == -1).all()) and bool(dense.all()) and tuple(dense.shape) == (1, 4096, 4096)


# ---- 4. reproducible
def test_two_launches_give_the_same_bytes():
    pic = torch.from_numpy(C.fixture_picture("thr19_a")).cuda()
    a, b = E.MinmaxDecode(pic), E.MinmaxDecode(pic)
    assert torch.equal(a.out, b.out) and torch.equal(a.workspace, b.workspace)
    (abits, abytes, an), (bbits, bbytes, bn) = a.bits(with_bytes=True), b.bits(with_bytes=True)
    assert an == bn == 683 and torch.equal(abits, bbits) and torch.equal(abytes, bbytes)
    assert a.bits()[0] is abits                                                # the count and the masks are made once


# ---- 5. results JSON
def check_entries(entries, want, h, w, image_id):
    from tests import painter_rle_host as R
    masks = H.masks_of(want["label"], want["slot"])
    assert len(entries) == want["count"]
    for e, score, cls, mask in zip(entries, want["scores"], want["classes"], masks):
        assert sorted(e) == ["bbox", "category_id", "image_id", "score", "segmentation"]
        assert e["image_id"] == image_id and e["category_id"] == int(cls) and type(e["category_id"]) is int and e["bbox"] == [0.0, 0.0, 0.0, 0.0]
        assert type(e["score"]) is float and e["score"] == float(score)
        assert e["segmentation"] == {"size": [h, w], "counts": R.encode_mask(mask)["counts"]}
    json.dumps(entries)


def test_instance_results_of_a_minmax_decode():
    for name in ("thr19_c", "few"):
        pic, want = case(name)
        h, w = pic.shape[:2]
        dpic = torch.from_numpy(pic).cuda()
        threshold = E.InstanceDecode(dpic, None, [19.0], 2000, 100, "gaussian", 2.0)
        before = json.dumps(E.instance_results(threshold, 5))
        dec = E.MinmaxDecode(dpic)
        entries = E.instance_results(dec, "id-%s" % name)
        check_entries(entries, want, h, w, "id-%s" % name)
        assert 0 in [e["category_id"] for e in entries] and 1 in [e["category_id"] for e in entries]
        assert E.instance_results(dec, 9) == [dict(e, image_id=9) for e in entries]
        assert json.dumps(E.instance_results(threshold, 5)) == before          # the threshold route is as it was
        fresh = E.InstanceDecode(dpic, None, [19.0], 2000, 100, "gaussian", 2.0)
        assert json.dumps(E.instance_results(fresh, 5)) == before


# ---- 6. through the engine
def test_engine_runs_with_post_type():
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70)]
    ids = [101, "b"]
    target = PC.picture(PC.PROMPT[0] + 200, PC.PROMPT[1], PC.PROMPT[2], flat=True)
    pal = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128], [200, 180, 40]], np.float32)

    def engine(bs):
        img, _ = PC.prompt_pair()
        return E.PainterEngine(PC.StandInModel(), "cuda", "coco_pano_inst", img, target, input_size=PC.RES, batch_size=bs)
    decoded = engine(8).run(pictures)
    assert [d.shape for d in decoded] == [(60, 80, 3), (45, 70, 3)]
    for palette in (None, pal):
        wants = [E.instances_minmax(d, palette=palette) for d in decoded]
        for bs in (1, 8):
            got = engine(bs).run_instances(pictures, post_type="minmax", palette=palette)
            assert len(got) == 2
            for g, want in zip(got, wants):
                assert g.keys() == want.keys()
                for key in want:
                    assert g[key].dtype == want[key].dtype and np.array_equal(g[key], want[key]), key
            flat = E.run_instance_results(engine(bs), pictures, ids, post_type="minmax", palette=palette)
            expect = [e for d, i in zip(decoded, ids) for e in E.instance_results(E.MinmaxDecode(torch.from_numpy(d).cuda(), palette), i)]
            assert flat == expect and len(flat) == sum(len(w["scores"]) for w in wants)
    assert len(wants[0]["scores"]) >= 2
    ikw = dict(dist_thr=[30.0], nms_pre=150, max_num=20)
    plain, named = engine(8).run_instances(pictures, **ikw), engine(8).run_instances(pictures, post_type="threshold", **ikw)
    for a, b in zip(plain, named):
        assert a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert json.dumps(E.run_instance_results(engine(2), pictures, ids, **ikw)) == \
        json.dumps(E.run_instance_results(engine(2), pictures, ids, post_type="threshold", **ikw))
