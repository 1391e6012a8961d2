"""The restoration-scoring definition (tests/painter_restore_host.py) against the one number of the unmodified reference that can be
produced here (myPSNR of painter_inference_lol.py, tests/golden/painter_restore.npz), against itself (two window orderings), the Y formula
on all 2^24 colours, hand-checked values, and what can be said about the entry points without a GPU."""
import inspect
import os
import types

import numpy as np
import pytest

from tests import painter_restore_cases as C
from tests import painter_restore_host as H

CASES = [(name, metric) for name, case in C.FIXTURE.items() for metric in case[4]]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_restore.npz"))


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name, n_args in (("pa_restore_scores", 11), ("pa_restore_workspace_bytes", 2), ("pa_restore_tile", 0)):
        assert name in protos and len(protos[name][1]) == n_args
        assert getattr(lib, name) is not None
    assert lib.pa_abi_version() == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "painter_hip.h")).read()
    assert "pa_restore_job" in header and "#define PA_RESTORE_RGB_F64 0" in header and "#define PA_RESTORE_Y_U8 1" in header
    tile = lib.pa_restore_tile()
    assert tile >= 8
    # 16 bytes per tile and the 24-byte records of the table
    assert lib.pa_restore_workspace_bytes(8, 1000) == 16 * 1000 + 24 * 8
    assert lib.pa_restore_workspace_bytes(0, 10) == lib.pa_restore_workspace_bytes(1, -1) == lib.pa_restore_workspace_bytes(1, 0) == -1
    assert lib.pa_restore_workspace_bytes(1025, 10) == lib.pa_restore_workspace_bytes(1, (1 << 24) + 1) == -1
    # the LDS budget the tile was sized for: two halo planes and five moment planes of doubles, three workgroups per 160 KB CU
    edge = tile + 10
    assert 3 * (8 * (2 * edge * edge + 5 * edge * tile) + 8 * 11 + 64) <= 160 * 1024


def test_entry_point_refuses_bad_arguments_on_the_host():
    """The job table is a host array: hipErrorInvalidValue (1) for a picture below the window, before any pointer is handed to the device."""
    import ctypes
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib
    # a non-null, aligned, never dereferenced address: every call below is refused by a host-side check before the table copy is enqueued.
    # Were such a check to regress on a machine WITH a device, the call would enqueue a copy to this address -- keep one bad argument per call.
    a = 256
    w7 = (ctypes.c_double * 7)(*([1 / 7] * 7))

    def call(h=7, w=7, n_jobs=1, mode=0, win=7, weights=w7, cov=1.0, c1=1e-4, c2=9e-4, pred=a, gt=a, out=a, ws=a, table=True):
        jobs = (E.RestoreJob * 1)()
        jobs[0].pred, jobs[0].gt, jobs[0].h, jobs[0].w = pred, gt, h, w
        return lib.pa_restore_scores(ctypes.addressof(jobs) if table else None, n_jobs, mode, win, ctypes.addressof(weights) if weights else None,
                                     cov, c1, c2, out, ws, 0)

    for kw in (dict(h=6), dict(w=6), dict(h=0), dict(n_jobs=0), dict(n_jobs=1025), dict(mode=2), dict(mode=-1), dict(win=0), dict(win=12),
               dict(weights=None), dict(cov=0.0), dict(cov=float("nan")), dict(c1=0.0), dict(c2=float("inf")), dict(pred=0), dict(gt=0),
               dict(out=0), dict(ws=0), dict(out=a + 4), dict(ws=a + 4), dict(pred=a + 4), dict(table=False)):
        assert call(**kw) == 1, kw
    w11 = (ctypes.c_double * 11)(*([1 / 11] * 11))
    assert call(h=10, w=40, mode=1, win=11, weights=w11) == 1 and call(h=40, w=10, mode=1, win=11, weights=w11) == 1
    bad = (ctypes.c_double * 7)(*([1 / 7] * 6 + [float("nan")]))
    assert call(weights=bad) == 1
    assert E.ctypes.sizeof(E.RestoreJob) == 24


@pytest.mark.parametrize("name,metric", CASES)
def test_statement_reproduces_the_fixture_and_mypsnr(golden, name, metric):
    """The statement's record is what the fixture stores; its PSNR is myPSNR's (the reference's) within 1e-12 relative."""
    pred, gt = C.inputs(*C.fixture_case(name), metric)
    sums = H.sums(pred, gt, metric)
    key = "%s.%s." % (name, metric)
    assert np.array_equal(sums, golden[key + "sums"])
    psnr, ssim = H.scores(pred, gt, metric)
    assert psnr == golden[key + "psnr"] and ssim == golden[key + "ssim"]
    if metric == "skimage":
        ref = float(golden[name + ".myPSNR"])
        assert psnr == ref if np.isinf(ref) else abs(psnr - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("name,metric", CASES)
def test_the_two_window_orderings_agree(golden, name, metric):
    pred, gt = C.inputs(*C.fixture_case(name), metric)
    direct, scipy_route = H.scores(pred, gt, metric, route="direct")[1], H.scores(pred, gt, metric, route="scipy")[1]
    print(name, metric, "direct - scipy", direct - scipy_route)
    assert abs(direct - scipy_route) <= 1e-12 and scipy_route == golden["%s.%s.ssim_scipy" % (name, metric)]
    pairs, _ = H.planes(pred, gt, metric)
    w = H.weights(metric)
    for x, y in pairs:
        for a, b in zip(H.moments(x, y, w, "direct"), H.moments(x, y, w, "scipy")):
            assert a.shape == b.shape == (x.shape[0] - len(w) + 1, x.shape[1] - len(w) + 1)
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def test_y_formula_on_every_colour():
    """Y = 16 + floor((65481 R + 128553 G + 24966 B + 127500) / 255000) is the exact rational 16 + (65.481 R + 128.553 G + 24.966 B) / 255
    rounded half up, on all 2^24 colours; 194 colours tie exactly at one half and round up; Y stays in [16, 235]."""
    c = np.arange(1 << 24, dtype=np.int64)
    rgb = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1)
    y = H.y_channel(rgb.astype(np.uint8))
    num = 65481 * rgb[:, 0] + 128553 * rgb[:, 1] + 24966 * rgb[:, 2]                # exact: (Y - 16) * 255000
    low, rem = num // 255000, num % 255000
    assert np.array_equal(y - 16, np.where(2 * rem >= 255000, low + 1, low))        # nearest, ties up
    tie = 2 * rem == 255000
    assert int(tie.sum()) == 194 and np.array_equal((y - 16)[tie], low[tie] + 1)
    assert y.min() == 16 and y.max() == 235 and y[0] == 16 and y[-1] == 235
    for colour in C.TIE_COLOURS:
        assert tie[(colour[0] << 16) | (colour[1] << 8) | colour[2]]


def test_fixture_covers_what_it_is_there_for(golden):
    clipped = golden["natural_61x83.clipped"]
    assert clipped[0] > 0 and clipped[1] > 0                                          # a prediction clipped at both ends
    pred, gt = C.fixture_case("natural_61x83")
    assert H.scores(pred, gt, "skimage") != H.scores(np.clip(pred, 0.01, 0.99), gt, "skimage")
    assert np.isinf(golden["perfect_40x52.skimage.psnr"]) and golden["perfect_40x52.skimage.ssim"] == 1.0          # a perfect prediction
    assert np.isinf(golden["perfect_40x52.matlab_y.psnr"]) and golden["perfect_40x52.matlab_y.ssim"] == 1.0
    assert np.isinf(golden["perfect_40x52.myPSNR"])
    pred, gt = C.fixture_case("near_constant_61x83")                                  # the cancellation-heavy pair
    assert gt.min() == 127 and gt.max() == 128 and np.abs(pred - gt / 255.).max() < 1e-5
    x = np.clip(pred, 0, 1)[..., 0]
    ux, _, uxx, _, _ = H.moments(x, x, H.weights("skimage"), "direct")
    assert ((uxx - ux * ux) / uxx).max() < 1e-4                                       # the variance is the last digits of two equal numbers
    pred, gt = C.fixture_case("ties_33x47")                                           # a Y case with tie colours
    code = (gt[..., 0].astype(np.int64) << 16) | (gt[..., 1].astype(np.int64) << 8) | gt[..., 2]
    ties = {(r << 16) | (g << 8) | b for r, g, b in C.TIE_COLOURS}
    assert np.isin(code, list(ties)).mean() > 0.3
    assert {m for _, m in CASES} == set(H.METRICS)


def test_hand_checked_values():
    """A 7 x 7 picture has exactly one window per channel; identical pictures give 1.0 and inf; S of one window by hand."""
    pred, gt = C.fixture_case("one_window_7x7")
    s = H.sums(pred, gt, "skimage")
    assert s[0] == 147 and list(s[3::2]) == [1, 1, 1]
    x, y = np.clip(pred, 0, 1)[..., 1], gt[..., 1] / 255.
    ux, uy = x.mean(), y.mean()
    vx, vy, vxy = x.var(ddof=1), y.var(ddof=1), ((x - ux) * (y - uy)).sum() / 48
    c1, c2 = 0.02 ** 2, 0.06 ** 2
    assert abs(s[4] - (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))) <= 1e-12
    assert abs(H.metrics(s, "skimage")[0] - 10 * np.log10(1 / ((np.clip(pred, 0, 1) - gt / 255.) ** 2).mean())) <= 1e-12
    assert H.constants("skimage") == (49 / 48, 0.02 ** 2, 0.06 ** 2) and H.constants("skimage", 1.0)[1:] == (0.01 ** 2, 0.03 ** 2)
    assert H.constants("matlab_y") == (1.0, (0.01 * 255) ** 2, (0.03 * 255) ** 2)          # (K * L)^2 as SSIM_index writes it: 2.55^2, 7.65^2
    w = H.weights("matlab_y")
    assert len(w) == 11 and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and abs(w[5] / w[4] - np.exp(1 / 4.5)) < 1e-15
    for metric in H.METRICS:
        p, g = C.inputs(*C.case("perfect", 9, 23, 31), metric)
        for route in ("direct", "scipy"):
            psnr, ssim = H.scores(p, g, metric, route=route)
            assert psnr == float("inf") and ssim == 1.0
    # a 11 x 11 picture has one Gaussian window; its Y squared sum is an integer
    p, g = C.inputs(*C.case("natural", 10, 11, 11), "matlab_y")
    s = H.sums(p, g, "matlab_y")
    assert s[0] == 121 and s[3] == 1 and s[1] == ((H.y_channel(p) - H.y_channel(g)) ** 2).sum() and list(s[4:]) == [0, 0, 0, 0]


def test_a_picture_below_the_window_is_an_error():
    from painter_amd import painter_engine as E
    for metric, (h, w) in (("skimage", (6, 40)), ("skimage", (40, 6)), ("matlab_y", (10, 40)), ("matlab_y", (40, 10))):
        p, g = C.inputs(*C.case("natural", 1, h, w), metric)
        with pytest.raises(ValueError, match="window"):
            H.sums(p, g, metric)
        with pytest.raises(ValueError, match="window"):
            E._restore_sizes("t", [(h, w)], [g], len(H.weights(metric)))
    with pytest.raises(ValueError):
        H.sums(np.zeros((8, 8, 3)), np.zeros((8, 9, 3), np.uint8), "skimage")


def test_engine_constants_are_the_statements():
    from painter_amd import painter_engine as E
    for metric in H.METRICS:
        mode, w, cov_norm, c1, c2 = E._restore_setup(metric)
        assert mode == H.METRICS.index(metric) and np.array_equal(w, H.weights(metric)) and (cov_norm, c1, c2) == H.constants(metric)
    assert E._restore_setup("skimage", 1.0)[3:] == H.constants("skimage", 1.0)[1:]
    assert E.RESTORE_METRICS == H.METRICS and E.RESTORE_OUT == H.OUT
    assert E.RESTORE_DEFAULT_METRIC == dict(lol="skimage", derain="matlab_y", sidd=None)
    d = {k: v.default for k, v in inspect.signature(E.restoration_scores).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(metric="skimage", data_range=2.0, device="cuda")
    for name in C.FIXTURE:
        for metric in C.FIXTURE[name][4]:
            s = H.sums(*C.inputs(*C.fixture_case(name), metric), metric)
            got, ref = E.restoration_metrics(s[None], metric), H.metrics(s, metric)
            assert got["psnr"][0] == ref[0] and got["ssim"][0] == ref[1]
    for text in (H.__doc__, E.restoration_scores.__doc__):
        assert "unverified against skimage / MATLAB" in " ".join(text.split())


def test_arguments_are_refused_before_anything_is_enqueued():
    """Task, metric, sizes and window are checked before the first forward: an engine that would fail on any use proves nothing ran."""
    from painter_amd import painter_engine as E
    pictures, gts = [np.zeros((16, 12, 3), np.uint8)], [np.zeros((16, 12, 3), np.uint8)]
    lol, sidd = types.SimpleNamespace(task="lol"), types.SimpleNamespace(task="sidd")
    with pytest.raises(ValueError, match="derain / lol / sidd"):
        E.PainterEngine.run_restoration_scores(types.SimpleNamespace(task="ade20k_semseg"), pictures, gts)
    with pytest.raises(ValueError, match="no default metric"):
        E.PainterEngine.run_restoration_scores(sidd, pictures, gts)
    with pytest.raises(ValueError, match="metric is one of"):
        E.PainterEngine.run_restoration_scores(lol, pictures, gts, metric="lpips")
    with pytest.raises(ValueError, match="ground truth"):
        E.PainterEngine.run_restoration_scores(lol, pictures, [np.zeros((12, 16, 3), np.uint8)])
    with pytest.raises(ValueError, match="ground-truth pictures"):
        E.PainterEngine.run_restoration_scores(lol, pictures, gts + gts)
    with pytest.raises(ValueError, match="window"):
        E.PainterEngine.run_restoration_scores(lol, pictures, [np.zeros((6, 12, 3), np.uint8)], sizes=[(12, 6)])
    with pytest.raises(ValueError, match="window"):
        E.PainterEngine.run_restoration_scores(types.SimpleNamespace(task="derain"), pictures, [np.zeros((16, 10, 3), np.uint8)], sizes=[(10, 16)])
    with pytest.raises(ValueError, match="data_range"):
        E.PainterEngine.run_restoration_scores(sidd, pictures, gts, metric="skimage", data_range=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.restoration_scores([np.zeros((16, 12, 3))], gts, device="cpu")
