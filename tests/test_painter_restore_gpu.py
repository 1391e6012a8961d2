"""GPU parity of restoration scoring (csrc/painter_restore.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_restore_host.py, the definition.

The bars.  Element and window counts are equal.  The Y-mode squared sum is an integer and equal.  The float64 squared sum is within
1e-12 * sum of the exactly rounded sum (math.fsum) of the statement's terms: the device adds at most a few thousand non-negative terms per
partial and a few dozen partials here, each addition within 2^-53 relative of the running sum.  Each picture's SSIM is within 1e-10
absolute of the statement's.  That bar is derived, not tuned: the cancellation in uxx - ux ux costs at most win^2 * 2^-53 * max^2 -- 8.7e-10
for the Gaussian at L = 255 against C2 = 58.5, so <= 1.5e-11 per pixel of S, and <= 1.5e-12 for the uniform window at L = 2; the statement's
own two orderings differ by <= 2.7e-13 in practice; 1e-10 is about 7 x the worst-case bound.  The largest deviation seen is printed.

The shapes are the smallest that can break the kernel: one window, one window and a column, the halo of one full tile and one pixel less /
more each way, two tile rows by three tile columns with one-window remainders, a one-window-wide strip 300 long both ways, 61 x 83, and all
of them in one launch."""
import math

import numpy as np
import pytest
import torch

from tests import painter_restore_cases as C
from tests import painter_restore_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

INVALID = 1                                            # hipErrorInvalidValue
SSIM_BAR = 1e-10
SSD_BAR = 1e-12


def shapes(metric):
    win, tile = len(H.weights(metric)), lib.pa_restore_tile()
    e = tile + win - 1
    return [(win, win), (win, win + 1), (e, e), (e - 1, e), (e + 1, e), (e, e - 1), (e, e + 1), (e + 1, e + tile + 1),
            (win, 300 + win - 1), (300 + win - 1, win), (61, 83)]


_REFERENCE = {}


def reference(metric):
    """The seeded pictures of `shapes(metric)` and the statement's records, computed once per metric and left unchanged."""
    if metric not in _REFERENCE:
        pairs = [C.inputs(*C.case("natural", 40 + i, h, w), metric) for i, (h, w) in enumerate(shapes(metric))]
        records = np.stack([H.sums(p, g, metric) for p, g in pairs])
        records.setflags(write=False)
        _REFERENCE[metric] = (pairs, records)
    return _REFERENCE[metric]


def device_sums(pairs, metric, **kw):
    dev = torch.device("cuda", torch.cuda.current_device())
    preds = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p, _ in pairs]
    gts = [torch.from_numpy(np.ascontiguousarray(g)).to(dev) for _, g in pairs]
    return E.RestorationScores(preds, gts, metric, **kw).sums()


def check_record(got, ref, metric, what):
    """One picture's device record against the statement's -> |SSIM difference|."""
    assert got.shape == ref.shape == (8,)
    assert got[0] == ref[0] and np.array_equal(got[3::2], ref[3::2]), (what, got, ref)             # element and window counts
    if metric == "matlab_y":
        assert got[1] == ref[1] and got[1] == int(got[1]) and np.array_equal(got[4:], np.zeros(4)), (what, got, ref)
    else:
        assert abs(got[1] - ref[1]) <= SSD_BAR * ref[1], (what, got[1], ref[1])
    dev = abs(float(H.metrics(got, metric)[1]) - float(H.metrics(ref, metric)[1]))
    assert dev <= SSIM_BAR, (what, dev)
    return dev


# ---- 1. the definition, on the smallest shapes that can break the kernel
@pytest.mark.parametrize("metric", H.METRICS)
def test_sums_equal_the_statement_alone_and_in_a_mixed_list(metric):
    pairs, records = reference(metric)
    mixed = device_sums(pairs, metric)
    assert mixed.shape == (len(pairs), 8) and mixed.dtype == np.float64
    worst = 0.0
    for i, (pair, shape) in enumerate(zip(pairs, shapes(metric))):
        alone = device_sums([pair], metric)
        worst = max(worst, check_record(alone[0], records[i], metric, shape))
        assert alone[0].tobytes() == mixed[i].tobytes(), shape                         # the company in the launch changes no bit
    print("restoration scores, %s: largest |SSIM(device) - SSIM(statement)| over %d shapes: %.3e (bar %.0e)" % (metric, len(pairs), worst, SSIM_BAR))
    assert device_sums(pairs, metric).tobytes() == mixed.tobytes()                      # two runs, the same bits
    assert device_sums(pairs[::-1], metric)[::-1].tobytes() == mixed.tobytes()          # nor does the order of the list
    windows = [(h - len(H.weights(metric)) + 1) * (w - len(H.weights(metric)) + 1) for h, w in shapes(metric)]
    assert list(mixed[:, 3]) == windows and windows[0] == 1 and windows[1] == 2 and windows[8] == windows[9] == 300


def test_public_function_takes_arrays_and_tensors_and_returns_the_statements_scores():
    for metric in H.METRICS:
        pairs, records = reference(metric)
        pairs, records = pairs[-3:], records[-3:]
        got = E.restoration_scores([p for p, _ in pairs], [g for _, g in pairs], metric=metric)
        assert set(got) == {"psnr", "ssim"} and got["psnr"].shape == got["ssim"].shape == (3,) and got["psnr"].dtype == np.float64
        psnr, ssim = H.metrics(records, metric)
        assert np.abs(got["ssim"] - ssim).max() <= SSIM_BAR and np.allclose(got["psnr"], psnr, rtol=1e-12, atol=0)
        tensors = E.restoration_scores([torch.from_numpy(p).cuda() for p, _ in pairs], [torch.from_numpy(g).cuda() for _, g in pairs], metric)
        assert tensors["psnr"].tobytes() == got["psnr"].tobytes() and tensors["ssim"].tobytes() == got["ssim"].tobytes()
    empty = E.restoration_scores([], [])
    assert empty["psnr"].shape == empty["ssim"].shape == (0,)
    # data_range is skimage's: 1.0 gives other constants, and the statement's numbers for them
    p, g = reference("skimage")[0][-1]
    one = E.restoration_scores([p], [g], data_range=1.0)["ssim"][0]
    assert abs(one - H.scores(p, g, "skimage", data_range=1.0)[1]) <= SSIM_BAR and one != E.restoration_scores([p], [g])["ssim"][0]


# ---- 2. the properties
def test_predictions_outside_the_range_are_clipped():
    pred, gt = C.fixture_case("natural_61x83")
    assert (pred < 0).sum() > 0 and (pred > 1).sum() > 0
    a = device_sums([(pred, gt)], "skimage")
    b = device_sums([(np.clip(pred, 0, 1), gt)], "skimage")
    assert a.tobytes() == b.tobytes()
    check_record(a[0], H.sums(pred, gt, "skimage"), "skimage", "clipped")
    d = pred - gt / 255.
    assert abs(a[0, 1] - math.fsum((d * d).ravel().tolist())) > 1e-6 * a[0, 1]               # the unclipped squared sum is another number


def test_a_perfect_prediction_gives_one_and_infinity():
    for metric in H.METRICS:
        pairs = [C.inputs(*C.case("perfect", 3, h, w), metric) for h, w in ((40, 52), (61, 83))]
        got = E.restoration_scores([p for p, _ in pairs], [g for _, g in pairs], metric)
        assert list(got["ssim"]) == [1.0, 1.0] and np.isinf(got["psnr"]).all() and (got["psnr"] > 0).all(), (metric, got)
        sums = device_sums(pairs, metric)
        assert (sums[:, 1] == 0).all() and np.array_equal(sums[:, 2], sums[:, 3])


def test_the_near_constant_pair_stays_within_the_bar():
    pred, gt = C.fixture_case("near_constant_61x83")
    for metric in H.METRICS:
        p, g = C.inputs(pred, gt, metric)
        dev = check_record(device_sums([(p, g)], metric)[0], H.sums(p, g, metric), metric, "near constant")
        print("restoration scores, %s, near-constant pair: |SSIM(device) - SSIM(statement)| = %.3e (bar %.0e)" % (metric, dev, SSIM_BAR))


def test_tie_colours_in_y_mode_equal_the_statement():
    pred, gt = C.fixture_case("ties_33x47")
    p, g = C.inputs(pred, gt, "matlab_y")
    got, ref = device_sums([(p, g)], "matlab_y")[0], H.sums(p, g, "matlab_y")
    check_record(got, ref, "matlab_y", "ties")
    # a picture of tie colours alone against itself shifted by one colour: every Y on both sides is a tie
    ties = np.array(C.TIE_COLOURS, np.uint8)
    a = ties[np.arange(11 * 13).reshape(11, 13) % len(ties)]
    b = ties[(np.arange(11 * 13).reshape(11, 13) + 1) % len(ties)]
    got = device_sums([(a, b)], "matlab_y")[0]
    assert got[1] == ((H.y_channel(a) - H.y_channel(b)) ** 2).sum() > 0
    check_record(got, H.sums(a, b, "matlab_y"), "matlab_y", "ties only")


# ---- 3. refusals
def test_errors():
    dev = torch.device("cuda", torch.cuda.current_device())
    for metric, (h, w) in (("skimage", (6, 40)), ("skimage", (40, 6)), ("matlab_y", (10, 40)), ("matlab_y", (40, 10))):
        p, g = C.inputs(*C.case("natural", 1, h, w), metric)
        with pytest.raises(ValueError, match="window"):
            E.restoration_scores([p], [g], metric)
        # the C entry point: hipErrorInvalidValue from the host table, nothing is launched (the output keeps its bytes)
        mode, weights, cov_norm, c1, c2 = E._restore_setup(metric)
        tp, tg = torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)
        jobs = (E.RestoreJob * 1)()
        jobs[0].pred, jobs[0].gt, jobs[0].h, jobs[0].w = tp.data_ptr(), tg.data_ptr(), h, w
        out = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
        ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
        err = lib.pa_restore_scores(E.ctypes.addressof(jobs), 1, mode, len(weights), weights.ctypes.data, cov_norm, c1, c2, out.data_ptr(),
                                    ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert err == INVALID and (out.cpu().numpy() == 7.0).all() and not ws.cpu().numpy().any()
    pred, gt = C.case("natural", 1, 16, 12)
    with pytest.raises(ValueError, match="ground truth"):
        E.restoration_scores([pred], [gt[:, :11].copy()])
    with pytest.raises(ValueError, match="ground-truth pictures"):
        E.restoration_scores([pred], [gt, gt])
    with pytest.raises(ValueError, match="metric is one of"):
        E.restoration_scores([pred], [gt], metric="lpips")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.restoration_scores([torch.from_numpy(pred)], [gt])


# ---- 4. the engine
def _engine(task, bs, model=None):
    from tests import painter_eval_cases as PC
    return E.PainterEngine(model or PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)


def test_engine_refusals():
    from tests import painter_eval_cases as PC
    queries = PC.query_pictures("derain")[1:]
    sizes = [(52, 40)]
    gt = C.ground_truth(8, 40, 52)
    with pytest.raises(ValueError, match="derain / lol / sidd"):                        # wrong task
        _engine("ade20k_semseg", 2).run_restoration_scores(queries, [gt], sizes)
    model = PC.StandInModel()
    with pytest.raises(ValueError, match="no default metric"):                          # sidd without a metric
        _engine("sidd", 2, model).run_restoration_scores(queries, [gt], sizes)
    with pytest.raises(ValueError, match="ground truth"):                               # mismatched sizes
        _engine("lol", 2, model).run_restoration_scores(queries, [gt[:39].copy()], sizes)
    with pytest.raises(ValueError, match="window"):
        _engine("derain", 2, model).run_restoration_scores(queries, [gt[:10].copy()], [(52, 10)])
    assert model.calls == []                                                            # all of it before the first forward
    got = _engine("sidd", 2, model).run_restoration_scores(queries, [gt], sizes, metric="skimage")
    assert got["ssim"].shape == (1,) and len(model.calls) == 1


def test_run_restoration_scores_equals_scoring_what_run_restoration_returns():
    """The configuration of tests/test_painter_eval_gpu.py's run_restoration test (the stand-in model, derain's queries), at small output
    sizes: both metrics, bit for bit against `restoration_scores` of the returned pictures, and within the bars of the statement."""
    from tests import painter_eval_cases as PC
    queries = PC.query_pictures("derain") + PC.query_pictures("lol")[1:]
    sizes = [(83, 61), (52, 40), (35, 36)]                                              # (width, height)
    gts = [C.ground_truth(20 + i, h, w) for i, (w, h) in enumerate(sizes)]
    restored, saved = _engine("derain", 8).run_restoration(queries, sizes)
    for metric, preds in (("skimage", restored), ("matlab_y", saved)):
        ref = E.restoration_scores(preds, gts, metric)
        for bs in (1, 2, 8):
            got = _engine("derain", bs).run_restoration_scores(queries, gts, sizes, metric=metric)
            assert got["psnr"].tobytes() == ref["psnr"].tobytes() and got["ssim"].tobytes() == ref["ssim"].tobytes(), (metric, bs)
        host = [H.scores(p, g, metric) for p, g in zip(preds, gts)]
        assert np.abs(ref["ssim"] - [s for _, s in host]).max() <= SSIM_BAR
        assert np.allclose(ref["psnr"], [p for p, _ in host], rtol=1e-12, atol=0)
    # the defaults by task: derain -> matlab_y, lol -> skimage
    assert _engine("derain", 8).run_restoration_scores(queries, gts, sizes)["ssim"].tobytes() == \
        E.restoration_scores(saved, gts, "matlab_y")["ssim"].tobytes()
    lol = _engine("lol", 8).run_restoration_scores(queries, gts, sizes)
    assert lol["ssim"].tobytes() == E.restoration_scores(_engine("lol", 8).run(queries, sizes), gts, "skimage")["ssim"].tobytes()
