"""GPU parity of the boundary-IoU branch (csrc/painter_score.hip: pa_semseg_boundary_confusion, pa_label_boundary, through the C ABI and
painter_amd/painter_engine.py) against tests/painter_boundary_host.py -- the definition, restated from detectron2's published source and
unverified against detectron2 / cv2 -- and of its plain matrix against `SemsegScore` byte for byte.

Every comparison is of integers or bytes: no tolerances.  The shapes are the smallest that break each piece: d >= w and d >= h, 2d + 1
wider than the picture, d = 16 / 21 / 25 / 36 / 66 across the tiles of min(64, 2d + 1) columns and the strips of min(32, 2d + 1) rows,
5063 pixels (no multiple of 64), one-pixel rows and columns, K = 199 / 200 / 254 for LDS bins and direct adds."""
import functools

import numpy as np
import pytest
import torch

from tests import painter_boundary_host as B
from tests import painter_score_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

INVALID = 1                                            # hipErrorInvalidValue
# beyond B.SHAPES: windows of 73 and 133 columns INSIDE the picture -- full tiles of 64 outputs whose common columns are streamed
WIDE = [(80, 150, .212, 36), (200, 260, .2, 66)]
SEMSEG_CASES = [(name, d) for name, case in C.SEMSEG.items() for d in case[4]]


@functools.lru_cache(maxsize=None)
def reference(name, dist_type="abs", ratio=.02):
    pic, gt, pal = C.semseg_fixture_case(name)
    return B.boundary_confusion([pic], [gt], pal, dist_type, dilation_ratio=ratio)


def device_matrices(pictures, gts, palette, dist_type="abs", ratio=.02, bins=0):
    score = E.SemsegBoundaryScore(palette, dist_type, dilation_ratio=ratio)
    score.bins = bins
    score.add(pictures, gts)
    return score.matrix(), score.boundary_matrix()


def plain_matrix(pictures, gts, palette, dist_type="abs", bins=0):
    score = E.SemsegScore(palette, dist_type)
    score.bins = bins
    return score.add(pictures, gts).matrix()


def same(a, b):
    return a.dtype == b.dtype == np.int64 and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the erosion alone
@pytest.mark.parametrize("h,w,ratio,d", B.SHAPES + WIDE)
def test_label_boundary_equals_the_statement(h, w, ratio, d):
    assert B.dilation(h, w, ratio) == d
    _, _, _, pred, gtk = B.label_maps(h, w)
    for m in (pred, gtk, np.full((h, w), 7, np.uint8), np.zeros((h, w), np.uint8)):
        got = E.label_boundary(m, ratio)
        want = B.boundary(m, d)
        assert got.dtype == np.uint8 and got.shape == (h, w) and got.tobytes() == want.tobytes()
    if (h, w, ratio, d) in WIDE:
        assert 2 * d + 1 < min(h, w) and d >= 32 and (B.boundary(gtk, d) != gtk).any()          # the interior is there and differs
    assert E.label_boundary(torch.from_numpy(gtk).cuda(), ratio).tobytes() == B.boundary(gtk, d).tobytes()


# ---- 2. both matrices
@pytest.mark.parametrize("name,dist_type", SEMSEG_CASES)
def test_matrices_equal_the_statement_and_the_plain_scorer(name, dist_type):
    pic, gt, pal = C.semseg_fixture_case(name)
    conf, bconf, invalid = reference(name, dist_type)
    got, bgot = device_matrices([pic], [gt], pal, dist_type)
    assert invalid == 0 and same(bgot, bconf) and same(got, conf)
    assert same(got, plain_matrix([pic], [gt], pal, dist_type))
    assert bgot.sum() == gt.size and np.count_nonzero(bgot) > 300


def test_mixed_table_two_adds_reset_and_empty_list():
    pal = C.coco_palette()
    pairs = [C.semseg_case("coco", 20 + i, h, w)[:2] for i, (h, w) in enumerate(((1, 1), (1, 300), (300, 1), (61, 83), (96, 128)))]
    pics, gts = [p for p, _ in pairs], [g for _, g in pairs]
    assert [B.dilation(*g.shape) for g in gts] == [1, 6, 6, 2, 3]                # d differs per job
    conf, bconf, _ = B.boundary_confusion(pics, gts, pal)
    whole, bwhole = device_matrices(pics, gts, pal)
    assert same(whole, conf) and same(bwhole, bconf) and bwhole.sum() == 1 + 300 + 300 + 5063 + 12288
    assert same(whole, plain_matrix(pics, gts, pal))
    score = E.SemsegBoundaryScore(pal)
    score.add(pics[:2], gts[:2])
    score.add(pics[2:], gts[2:])                                                 # the second list is larger: the workspace grows
    assert same(score.matrix(), whole) and same(score.boundary_matrix(), bwhole)
    score.reset()
    assert not score.matrix().any() and not score.boundary_matrix().any() and score.add([], []) is score


@pytest.mark.parametrize("h,w,ratio,d", [(96, 128, .1, 16), (96, 128, .35, 56), (61, 83, .1, 10), (61, 83, .35, 36)])
def test_matrices_at_wider_dilations(h, w, ratio, d):
    assert B.dilation(h, w, ratio) == d
    pic, gt, pal = B.label_maps(h, w)[:3]
    conf, bconf, _ = B.boundary_confusion([pic], [gt], pal, dilation_ratio=ratio)
    got, bgot = device_matrices([pic], [gt], pal, ratio=ratio)
    assert same(got, conf) and same(bgot, bconf) and same(got, plain_matrix([pic], [gt], pal))


@pytest.mark.parametrize("k", [199, 200, 254])
def test_bins_in_lds_and_in_memory(k):
    assert lib.pa_semseg_lds_bins(k) == int(k <= 199)
    pal = C.synthetic_palette(k)
    pic, gt = C.noisy_case(k, 61, 83, pal)
    conf, bconf, invalid = B.boundary_confusion([pic], [gt], pal)
    assert invalid == 0 and np.count_nonzero(bconf) > 300
    for bins in (0, 1):
        got, bgot = device_matrices([pic], [gt], pal, bins=bins)
        assert same(got, conf) and same(bgot, bconf), bins
        assert same(got, plain_matrix([pic], [gt], pal, bins=bins))


# ---- 3. determinism, inputs, invalid labels
def test_two_runs_give_identical_bytes_and_tensors_equal_arrays():
    pic, gt, pal = C.semseg_fixture_case("ade_96x128")
    first, again = device_matrices([pic], [gt], pal), device_matrices([pic], [gt], pal)
    dev = device_matrices([torch.from_numpy(pic).cuda()], [torch.from_numpy(gt).cuda()], pal)
    for i in range(2):
        assert first[i].tobytes() == again[i].tobytes() == dev[i].tobytes()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.SemsegBoundaryScore(pal).add([torch.from_numpy(pic)], [gt])


def test_invalid_labels_make_both_matrices_raise():
    pal = C.coco_palette()
    pic, gt, _ = C.semseg_case("coco", 3, 61, 83)
    bad = gt.copy()
    bad[5, :7], bad[9, 3] = 133, 254
    score = E.SemsegBoundaryScore(pal).add([pic], [bad])
    with pytest.raises(ValueError, match=r"\b8 ground-truth pixels"):
        score.matrix()
    with pytest.raises(ValueError, match=r"\b8 ground-truth pixels"):
        score.boundary_matrix()
    with pytest.raises(ValueError, match=r"\b8 ground-truth pixels"):
        score.scores()


# ---- 4. the engine
def _engine(task, bs):
    from tests import painter_eval_cases as PC
    return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)


def test_run_semseg_score_equals_scoring_the_pictures_run_returns():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48), PC.picture(92, 60, 80), PC.picture(93, 45, 70)]
    sizes = [(24, 32), (40, 30), (35, 23)]                              # (width, height)
    pal = C.ade_palette()
    rng = np.random.default_rng(5)
    gts = [rng.integers(0, 150, (h, w)).astype(np.uint8) for w, h in sizes]
    gts[1][3] = C.IGNORE
    painted = _engine("ade20k_semseg", 8).run(queries, sizes)
    conf, bconf, _ = B.boundary_confusion(painted, gts, pal)
    ref, bref = device_matrices(painted, gts, pal)
    assert same(ref, conf) and same(bref, bconf) and bref.sum() == sum(w * h for w, h in sizes)
    for bs in (1, 2, 8):
        score = E.SemsegBoundaryScore(pal)
        assert _engine("ade20k_semseg", bs).run_semseg_score(queries, gts, score, sizes) is score
        assert same(score.matrix(), ref) and same(score.boundary_matrix(), bref), bs
    scores = E.SemsegBoundaryScore(pal).add(painted, gts).scores()
    assert set(scores) == {"mIoU", "fwIoU", "mACC", "pACC", "IoU", "ACC", "BoundaryIoU", "minIoU_BIoU"}
    want = B.boundary_scores(conf, bconf)
    assert all(np.array_equal(scores[key], want[key], equal_nan=True) for key in want)


# ---- 5. the C ABI: refusals, guard bands
def _table(pics, maps, ds):
    jobs = (E.BoundaryJob * len(pics))()
    for job, p, g, d in zip(jobs, pics, maps, ds):
        job.picture, job.gt, job.h, job.w, job.d = p.data_ptr(), g.data_ptr(), int(p.shape[0]), int(p.shape[1]), d
    return E._job_table(jobs, pics[0].device)


def test_entry_points_refuse_bad_arguments_and_touch_nothing():
    pal = C.coco_palette()
    pic, gt, _ = C.semseg_case("coco", 3, 61, 83)
    pics, maps = [torch.from_numpy(pic).cuda()], [torch.from_numpy(gt).cuda()]
    host, table = _table(pics, maps, [2])
    palette = torch.from_numpy(np.array(pal, np.float32)).cuda()
    n = 134 * 134
    conf, bconf, inv = (torch.full((c,), 0x5A5A, dtype=torch.int64, device="cuda") for c in (n, n, 1))
    ws = torch.full((lib.pa_semseg_boundary_workspace_bytes(5063),), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((5063,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = dict(jobs=table.data_ptr(), n_jobs=1, total=5063, pal=palette.data_ptr(), k=133, dist=0, bins=0, conf=conf.data_ptr(),
              bconf=bconf.data_ptr(), inv=inv.data_ptr(), ws=ws.data_ptr())

    def call(c):
        return lib.pa_semseg_boundary_confusion(c["jobs"], c["n_jobs"], c["total"], c["pal"], c["k"], c["dist"], 255, c["bins"], c["conf"],
                                                c["bconf"], c["inv"], c["ws"], 0)

    for change in (dict(k=0), dict(k=255), dict(k=256), dict(total=0), dict(total=(1 << 31) + 1), dict(bins=2), dict(bins=-1), dict(dist=-1),
                   dict(dist=3), dict(n_jobs=0), dict(jobs=0), dict(pal=0), dict(conf=0), dict(bconf=0), dict(inv=0), dict(ws=0),
                   dict(bconf=bconf.data_ptr() + 4)):
        assert call(dict(ok, **change)) == INVALID, change
    m = maps[0]
    for h, w, d, ptrs in ((0, 83, 2, None), (61, 0, 2, None), (61, 83, 0, None), (61, 83, -3, None), (1 << 16, 1 << 16, 2, None),
                          (61, 83, 2, (0, 1, 1)), (61, 83, 2, (1, 0, 1)), (61, 83, 2, (1, 1, 0))):
        a, b, c = ptrs or (1, 1, 1)
        assert lib.pa_label_boundary(m.data_ptr() * a, h, w, d, out.data_ptr() * b, ws.data_ptr() * c, 0) == INVALID, (h, w, d, ptrs)
    torch.cuda.synchronize()
    assert (conf == 0x5A5A).all() and (bconf == 0x5A5A).all() and (inv == 0x5A5A).all() and (ws == 0x5A).all() and (out == 0x5A).all()
    del host


@pytest.mark.parametrize("h,w,d", [(61, 83, 21), (1, 300, 6)])
def test_guard_bands_of_both_entry_points(h, w, d):
    """conf, bconf, invalid, the boundary map and the workspace at exactly pa_semseg_boundary_workspace_bytes, each between poisoned guard
    bands: nothing outside them is written, and the results are those of the ordinary run."""
    from tests.guard_bands import Arena
    pal = C.coco_palette()
    k = len(pal)
    pic, gt, _ = C.semseg_case("coco", 3, h, w)
    ratio = {21: .2, 6: .02}[d]
    assert B.dilation(h, w, ratio) == d
    ordinary = device_matrices([pic], [gt], pal, ratio=ratio)
    gtk = np.where(gt == C.IGNORE, k, gt).astype(np.uint8)
    ordinary_map = E.label_boundary(gtk, ratio)
    arena = Arena("cuda")
    pics, maps = [torch.from_numpy(pic).cuda()], [torch.from_numpy(gt).cuda()]
    host, table = _table(pics, maps, [d])
    palette = torch.from_numpy(np.array(pal, np.float32)).cuda()
    nbytes = lib.pa_semseg_boundary_workspace_bytes(h * w)
    assert nbytes == 4 * ((h * w + 15) // 16 * 16)
    conf, bconf, inv = (arena.empty((c,), torch.int64, name=name) for c, name in (((k + 1) ** 2, "conf"), ((k + 1) ** 2, "bconf"), (1, "invalid")))
    for t in (conf, bconf, inv):
        t.zero_()                                                      # accumulated in place
    ws = arena.empty((nbytes,), torch.uint8, name="workspace")
    assert lib.pa_semseg_boundary_confusion(table.data_ptr(), 1, h * w, palette.data_ptr(), k, 0, 255, 0, conf.data_ptr(), bconf.data_ptr(),
                                            inv.data_ptr(), ws.data_ptr(), E._stream()) == 0
    arena.check()
    assert int(inv[0]) == 0
    assert conf.cpu().numpy().reshape(k + 1, k + 1).tobytes() == ordinary[0].tobytes()
    assert bconf.cpu().numpy().reshape(k + 1, k + 1).tobytes() == ordinary[1].tobytes()
    ws2 = arena.empty((nbytes,), torch.uint8, name="workspace of pa_label_boundary")
    out = arena.empty((h, w), torch.uint8, name="boundary map")
    src = torch.from_numpy(gtk).cuda()
    assert lib.pa_label_boundary(src.data_ptr(), h, w, d, out.data_ptr(), ws2.data_ptr(), E._stream()) == 0
    arena.check()
    assert out.cpu().numpy().tobytes() == ordinary_map.tobytes() == B.boundary(gtk, d).tobytes()
    del host
