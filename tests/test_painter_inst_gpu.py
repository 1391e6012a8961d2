"""GPU parity of the class-agnostic instance decode (csrc/painter_inst.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_inst_host.py -- the definition: exact integers, rational maskness order, stable sorts, float64 NMS -- and against what the
unmodified reference produced (tests/golden/painter_inst.npz).

The bars.  n, S, the survivor list and its order, areas, bit masks, the intersection matrix, the kept candidates and their masks: equal,
no tolerance.  Scores before the NMS: 4 ulp of float64 (two divisions and a subtraction, each correctly rounded on both sides).  Scores
after it: 1e-9 before the float32 cast (device exp against libm's), the order compared after grouping host scores closer than 1e-9.
Against the fixture: the same masks in the same order, scores within 4 x the deviation the reference's own float32 arithmetic showed
from the host statement when the fixture was made (two float32-versus-exact paths may lie on opposite sides of the exact value, and
the device's float32 cast adds half an ulp).  No fixture case is skipped."""
import os

import numpy as np
import pytest
import torch

from tests import painter_inst_cases as C
from tests import painter_inst_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

SCORE_TOL = 1e-9
_cache = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_inst.npz"))


def _palette():
    return E.location_palette()


def _host(name):
    """The host statement of a DECODE case, computed once and never modified."""
    if name not in _cache:
        _, _, _, thr, nms_pre, max_num = C.DECODE[name]
        _cache[name] = (C.decode_picture(name), H.decode(C.decode_picture(name), _palette(), thr, nms_pre, max_num))
    return _cache[name]


def _device(pic, thr, nms_pre=2000, max_num=100, kernel="gaussian", sigma=2.0):
    return E.InstanceDecode(torch.from_numpy(pic).cuda(), None, thr, nms_pre, max_num, kernel, sigma)


def _compare_result(res, host, max_num):
    """Kept set, masks, scores and order (after grouping host scores closer than SCORE_TOL) of a device result against the host's."""
    hs, hc = host["scores"], host["candidates"]
    assert len(res["candidates"]) == len(hc) <= max_num
    assert set(res["candidates"].tolist()) == set(hc.tolist())
    pos = {int(c): p for p, c in enumerate(hc)}
    at = np.array([pos[int(c)] for c in res["candidates"]])
    assert np.array_equal(np.isnan(res["scores_f64"]), np.isnan(hs[at]))
    err = float(np.nan_to_num(np.abs(res["scores_f64"] - hs[at])).max())
    print("scores: max |device - host| %.3e (bar %.1e)" % (err, SCORE_TOL))
    assert err <= SCORE_TOL
    assert np.array_equal(res["masks"], host["masks"][at])
    assert np.array_equal(res["bits"], H.pack_bits(res["masks"].reshape(len(at), -1)))          # both forms of the masks
    with np.errstate(invalid="ignore"):                # NaN scores sort first and form one group
        group = np.concatenate([[0], np.cumsum(np.abs(np.diff(np.where(np.isnan(hs), np.inf, hs))) >= SCORE_TOL)])
    assert np.array_equal(group[at], group), "order differs beyond ties of the host scores"
    assert np.array_equal(res["scores"], res["scores_f64"].astype(np.float32), equal_nan=True)
    assert res["labels"].dtype == np.float32 and (res["labels"] == 1).all() and res["masks"].dtype == bool
    assert res["scores"].dtype == np.float32 and res["candidates"].dtype == np.int32


# ---- 1. every stage of one decode, then its result
@pytest.mark.parametrize("name", list(C.DECODE))
def test_stages_and_result_match_the_host_statement(name):
    _, h, w, thr, nms_pre, max_num = C.DECODE[name]
    pic, host = _host(name)
    dec = _device(pic, thr, nms_pre, max_num)
    res = dec.result(with_f64=True, with_bits=True)
    m = len(thr) * C.K
    assert np.array_equal(dec.section(0, np.uint32, m), host["n"]) and np.array_equal(dec.section(1, np.uint64, m), host["s"])
    live, n_surv = dec.section(2, np.int32, 2)
    cand = host["survivors"]
    print("%s: %d live candidates, %d survivors" % (name, live, n_surv))
    assert live == host["live"] and n_surv == len(cand) == min(live, nms_pre)
    assert np.array_equal(dec.section(3, np.int32, nms_pre)[:n_surv], cand)
    assert np.array_equal(dec.section(4, np.int32, nms_pre)[:n_surv], host["areas"])
    pre = dec.section(5, np.float64, nms_pre)[:n_surv]
    assert np.abs(pre - host["survivor_scores"]).max() <= 4 * np.finfo(np.float64).eps
    stride = int(lib.pa_inst_workspace_offset(*dec.shape, 9))
    words = (h * w + 31) // 32
    assert stride % 4 == 0 and words <= stride < words + 4
    bits = dec.section(6, np.uint32, nms_pre * stride).reshape(nms_pre, stride)[:n_surv]
    assert np.array_equal(bits[:, :words], H.pack_bits(host["survivor_masks"])) and not bits[:, words:].any()
    inter = dec.section(7, np.int32, nms_pre * nms_pre).reshape(nms_pre, nms_pre)[:n_surv, :n_surv]
    upper = np.triu(np.ones((n_surv, n_surv), bool), 1)
    assert np.array_equal(inter[upper], host["inter"][upper])
    _compare_result(res, host, max_num)
    plain = E.instances(pic, dist_thr=thr if len(thr) > 1 else thr[0], nms_pre=nms_pre, max_num=max_num)
    assert sorted(plain) == ["candidates", "labels", "masks", "scores"]
    for k in plain:
        assert plain[k].dtype == res[k].dtype and np.array_equal(plain[k], res[k])


def test_cases_cover_what_they_are_for():
    assert C.DECODE["odd_size"][1] * C.DECODE["odd_size"][2] % 64 != 0 and C.DECODE["odd_caps"][4:] == (300, 7)
    assert _host("odd_caps")[1]["live"] > 300 and _host("ties_thr5")[1]["live"] < 2000
    for name in ("ties_thr5", "ties_two_thr"):          # exact maskness ties among the survivors
        host = _host(name)[1]
        n, s, c = host["n"], host["s"], host["survivors"]
        assert (s[c][1:] * n[c][:-1] == s[c][:-1] * n[c][1:]).sum() >= 10, name


# ---- 2. the stage entry points alone
def test_stats_entry_point():
    pic, host = _host("odd_size")
    thr = torch.tensor(C.DECODE["odd_size"][3], dtype=torch.float32, device="cuda")
    pal = torch.from_numpy(_palette().copy()).cuda()
    n = torch.full((C.K,), 7, dtype=torch.int32, device="cuda")
    s = torch.full((C.K,), 7, dtype=torch.int64, device="cuda")
    img = torch.from_numpy(pic).cuda()
    assert lib.pa_inst_stats(img.data_ptr(), pal.data_ptr(), thr.data_ptr(), n.data_ptr(), s.data_ptr(), pic.shape[0], pic.shape[1], C.K, 1,
                             E._stream()) == 0
    assert np.array_equal(n.cpu().numpy(), host["n"]) and np.array_equal(s.cpu().numpy(), host["s"])


@pytest.mark.parametrize("rows,words,density", [(130, 36, 0.5), (300, 1060, 0.02), (200, 68, 0.0005), (64, 4, 1.0)])
def test_intersections_entry_point(rows, words, density):
    """Dense random words (every accumulator busy), sparse and very sparse ones (a wave skips the words at which its 16 rows or the 64
    columns hold no bit), all ones; rows that fill no tile, words that fill no panel and more than one split of the words."""
    rng = np.random.default_rng(rows)
    masks = rng.random((rows, words * 32)) < density
    packed = torch.from_numpy(H.pack_bits(masks).view(np.int32)).cuda()
    out = torch.full((rows, rows + 3), -1, dtype=torch.int32, device="cuda")
    assert lib.pa_inst_intersections(packed.data_ptr(), rows, words, out.data_ptr(), rows + 3, E._stream()) == 0
    got, ref = out.cpu().numpy(), H.intersections(masks)
    upper = np.triu(np.ones((rows, rows), bool), 1)
    assert np.array_equal(got[:, :rows][upper], ref[upper]) and not got[:, rows:].any()


# ---- 3. the unmodified reference
@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_decode_reproduces_the_reference(golden, name):
    pic, thr = golden[name + ".picture"], [float(t) for t in golden[name + ".thresholds"]]
    assert np.array_equal(golden["palette"], _palette()) and thr == C.FIXTURE[name][3] and pic.shape[:2] == C.FIXTURE[name][1:3]
    res = E.instances(pic, dist_thr=thr)
    ref_scores, ref_bits = golden[name + ".scores"], golden[name + ".masks"]
    assert len(res["scores"]) == len(ref_scores) == 100
    assert np.array_equal(H.pack_bits(res["masks"].reshape(100, -1)), ref_bits)          # the same 100 masks in the same order
    err, bar = float(np.abs(res["scores"].astype(np.float64) - ref_scores).max()), 4 * float(golden["deviation"])
    print("%s: max |device - reference| %.3e (bar %.3e)" % (name, err, bar))
    assert err <= bar


# ---- 4. the linear kernel, the empty result
def test_linear_kernel():
    for name in ("ties_two_thr", "odd_caps"):
        _, _, _, thr, nms_pre, max_num = C.DECODE[name]
        pic, host = _host(name)
        ref = H.decode(pic, _palette(), thr, nms_pre, max_num, kernel="linear", stages=host)
        assert not np.array_equal(ref["scores"], host["scores"])                        # the kernel matters
        _compare_result(_device(pic, thr, nms_pre, max_num, kernel="linear").result(with_f64=True, with_bits=True), ref, max_num)
    with pytest.raises(NotImplementedError):
        E.instances(_host("odd_caps")[0], kernel="cubic")


def test_a_picture_without_candidates_gives_the_single_zero_mask():
    pic = np.zeros((37, 53, 3), np.uint8)
    assert H.decode(pic, _palette(), [5.0])["empty"]
    res = E.instances(pic, dist_thr=5.0)
    assert res["scores"].tolist() == [0.0] and res["labels"].tolist() == [0.0] and res["scores"].dtype == np.float32
    assert res["masks"].shape == (1, 37, 53) and res["masks"].dtype == bool and not res["masks"].any()


# ---- 5. determinism, other streams
def test_two_runs_give_the_same_bytes_also_beside_a_busy_stream():
    name = "odd_caps"
    _, _, _, thr, nms_pre, max_num = C.DECODE[name]
    pic = _host(name)[0]
    first = _device(pic, thr, nms_pre, max_num)
    ref_out, ref_ws = first.out.clone(), first.workspace.clone()
    again = _device(pic, thr, nms_pre, max_num)
    assert torch.equal(again.out, ref_out)
    live = [lib.pa_inst_workspace_offset(*first.shape, s) for s in (0, 1, 2)]            # n, S, counts: fully written sections
    for off, size in zip(live, (4 * C.K, 8 * C.K, 8)):
        assert torch.equal(again.workspace[off:off + size], ref_ws[off:off + size])
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda", dtype=torch.bfloat16)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):
            a = (a @ a).clamp_(-1, 1)
    beside = _device(pic, thr, nms_pre, max_num)
    with torch.cuda.stream(side):                        # and on a stream of its own
        there = _device(pic, thr, nms_pre, max_num)
    torch.cuda.synchronize()
    assert torch.equal(beside.out, ref_out) and torch.equal(there.out, ref_out)


# ---- 6. the C ABI
def test_entry_points_refuse_bad_arguments():
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched."""
    ok = dict(h=8, w=8, k=10, t=1, pre=20, top=5, kernel=0)
    bad = [dict(h=0), dict(w=0), dict(h=16385), dict(h=8192, w=8192), dict(k=0), dict(t=0), dict(t=9), dict(k=65537), dict(k=40000, t=2),
           dict(pre=0), dict(pre=4097), dict(top=0), dict(top=21), dict(kernel=2), dict(kernel=-1)]
    p = 256                                            # a non-null, aligned, never dereferenced address
    for change in bad:
        a = dict(ok, **change)
        assert lib.pa_inst_decode(p, p, p, a["h"], a["w"], a["k"], a["t"], a["pre"], a["top"], 2.0, a["kernel"], p, p, p, 0, p, p, 0, 0) == 1, change
        if not {"top", "kernel"} & set(change):
            assert lib.pa_inst_workspace_bytes(a["h"], a["w"], a["k"], a["t"], a["pre"]) == -1, change
    args = (8, 8, 10, 1, 20, 5, 2.0, 0)
    for null in range(8):                              # every required pointer (the float64 scores and the byte masks are optional)
        pic, pal, thr, ws, cnt, sc, idx, masks = [0 if i == null else p for i in range(8)]
        assert lib.pa_inst_decode(pic, pal, thr, *args, ws, cnt, sc, 0, idx, masks, 0, 0) == 1, null
    assert lib.pa_inst_decode(p, p, p, *args, p + 4, p, p, 0, p, p, 0, 0) == 1              # misaligned workspace
    for change in (dict(h=0), dict(k=0), dict(t=9)):
        a = dict(ok, **change)
        assert lib.pa_inst_stats(p, p, p, p, p, a["h"], a["w"], a["k"], a["t"], 0) == 1
    assert lib.pa_inst_stats(0, p, p, p, p, 8, 8, 10, 1, 0) == 1
    for rows, words, ld, m in ((0, 4, 8, p), (4097, 4, 4097, p), (8, 0, 8, p), (8, 6, 8, p), (8, 4, 7, p), (8, 4, 8, 0), (8, 4, 8, p + 4)):
        assert lib.pa_inst_intersections(m, rows, words, p, ld, 0) == 1, (rows, words, ld, m)
    with pytest.raises(RuntimeError, match="pa_inst_decode"):
        E.instances(np.zeros((4, 4, 3), np.uint8), nms_pre=5000)
    with pytest.raises(RuntimeError, match="pa_inst_decode"):
        E.instances(np.zeros((4, 4, 3), np.uint8), nms_pre=10, max_num=11)


def test_workspace_stays_near_the_bit_mask_budget():
    for h, w, k, t, pre in ((480, 640, 6400, 1, 2000), (120, 160, 6400, 2, 2000), (61, 83, 6400, 1, 300), (480, 640, 6400, 8, 4096)):
        budget = pre * h * w / 8 + 8 * pre * pre + 32 * t * k
        got = lib.pa_inst_workspace_bytes(h, w, k, t, pre)
        print("%dx%d K %d T %d nms_pre %d: %d bytes, budget %d" % (h, w, k, t, pre, got, budget))
        assert budget / 2 <= got <= 2 * budget


# ---- 7. the engine
def test_run_instances_equals_instances_of_the_pictures_run_returns():
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70), PC.picture(83, 64, 48)]
    kw = dict(dist_thr=[30.0], nms_pre=150, max_num=20)

    def engine(task, bs):
        return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)
    painted = engine("coco_pano_inst", 8).run(pictures)
    got = engine("coco_pano_inst", 2).run_instances(pictures, **kw)
    assert len(got) == 3
    for g, pic in zip(got, painted):
        ref = E.instances(pic, **kw)
        assert len(ref["scores"]) > 1 and g["masks"].shape[1:] == pic.shape[:2]
        for k in ref:
            assert np.array_equal(g[k], ref[k]), k
    with pytest.raises(ValueError):
        engine("ade20k_semseg", 8).run_instances(pictures)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.instances(pictures[0], device="cpu")
