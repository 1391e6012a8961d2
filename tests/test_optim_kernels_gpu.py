"""Kernel-level tests of the fused optimizer step (csrc/optim.hip: pa_grad_sumsq, pa_adamw_step) against torch.optim.AdamW +
clip_grad_norm_ in float64 on the CPU, gated by what torch's own fp32 AdamW loses against float64 on the same inputs
(tests/optim_cases.py: error measure, gate and floor).  Tests 1, 2, 3 and 5 drive the C ABI with hand-built PaOptTensor tables, so
that every pointer is under the test's control; the others go through painter_amd.optim.AdamW.

What the suite did not see before: step counts per parameter (a parameter without gradient next to a live one in its group), the
scalar branch both kernels take when a pointer of a chunk is not 16-byte aligned (the gradients of a flattened all-reduce bucket
are not), the bf16 operand copies by value, the reference's 52-group shape, step counts far from 1, and edge values.

Every test prints the device error next to the yardstick (pytest -s shows them).  MI355X, first runs (error = max|a - b| / max|b|
against float64; device / torch-fp32 yardstick / gate):

    case                      p                            exp_avg                      exp_avg_sq
    alignment[none]           2.32e-7 / 1.79e-7 / 3.58e-7  2.14e-7 / 3.51e-7 / 7.02e-7  2.43e-7 / 3.51e-7 / 7.02e-7
    alignment[g|p|mv|all]     1.79e-7 / 1.79e-7 / 3.58e-7  2.14e-7 / 3.51e-7 / 7.02e-7  2.58e-7 / 3.51e-7 / 7.02e-7
    decoder_pred bucket       1.25e-7 / 1.25e-7 / 2.51e-7  9.45e-8 / 2.29e-7 / 4.57e-7  1.13e-7 / 4.88e-7 / 9.77e-7
    partial (a) late, never   2.21e-7 / 2.69e-7 / 5.39e-7  8.96e-8 / 1.31e-7 / 2.61e-7  1.63e-7 / 2.70e-7 / 5.40e-7
    partial (b) switched on   1.65e-7 / 2.52e-7 / 5.04e-7  9.59e-8 / 1.95e-7 / 3.90e-7  1.09e-7 / 3.04e-7 / 6.08e-7
    partial (c) skipped step  1.08e-7 / 1.33e-7 / 2.65e-7  6.21e-8 / 2.29e-7 / 4.59e-7  1.14e-7 / 4.46e-7 / 8.93e-7
    checkpoint torch -> fused 3.17e-7 / 3.50e-7 / 7.00e-7  1.18e-7 / 1.18e-7 / 2.38e-7  1.22e-7 / 1.93e-7 / 3.86e-7
    checkpoint fused -> torch 3.23e-7 / 3.50e-7 / 7.00e-7  1.18e-7 / 1.18e-7 / 2.38e-7  1.34e-7 / 1.93e-7 / 3.86e-7
    state_dict between steps  2.21e-7 / 2.51e-7 / 5.01e-7  8.76e-8 / 8.76e-8 / 2.38e-7  1.07e-7 / 9.71e-8 / 2.38e-7
    step array grows 64->128  1.98e-7 / 3.48e-7 / 6.96e-7  1.38e-7 / 2.11e-7 / 4.22e-7  2.38e-7 / 3.85e-7 / 7.69e-7
    released, second group    2.01e-7 / 2.39e-7 / 4.77e-7  1.56e-7 / 1.84e-7 / 3.68e-7  3.30e-7 / 3.30e-7 / 6.60e-7
    52 groups, 352 tensors    1.08e-7 / 1.66e-7 / 3.31e-7  1.69e-7 / 2.18e-7 / 4.37e-7  2.55e-7 / 3.44e-7 / 6.88e-7
    300 steps                 3.43e-6 / 3.35e-6 / 6.69e-6  1.43e-7 / 1.89e-7 / 3.78e-7  2.57e-6 / 2.86e-6 / 5.73e-6
    edge zero gradients       1.11e-7 / 1.57e-7 / 3.14e-7  7.42e-8 / 7.42e-8 / 2.38e-7  9.82e-8 / 9.82e-8 / 2.38e-7
    edge +-1e-20              9.30e-8 / 9.30e-8 / 2.38e-7  9.97e-9 / 9.97e-9 / 2.38e-7  2.41e-5 / 2.41e-5 / 4.83e-5
    edge lr 0 | wd 0          6.36e-8 / 3.43e-8 / 2.38e-7  8.11e-8 / 8.11e-8 / 2.38e-7  8.28e-8 / 8.28e-8 / 2.38e-7
    edge eps 1e-3             8.17e-8 / 1.19e-7 / 2.38e-7  8.11e-8 / 8.11e-8 / 2.38e-7  8.28e-8 / 8.28e-8 / 2.38e-7
    edge frozen group         7.62e-8 / 1.50e-7 / 3.00e-7  6.28e-8 / 6.28e-8 / 2.38e-7  7.83e-8 / 7.83e-8 / 2.38e-7
    pa_grad_sumsq norm        1.1e-8 .. 2.3e-8 over the six layouts (gate 2e-6)

What these tests found when they were written.  With one step count per group, partial (a) ended with steps [6, 6, 6, 6] for torch's
[6, 6, 2, 0] and the late parameter off by 5.76e-3; (b) with [5, 5, 5, 5] for [5, 2, 5, 0] and 1.87e-3.  With 1 - beta formed in fp32
from the fp32-rounded beta (1.f - 0.999f is 1.3e-5 away from 0.001), the 300 steps left exp_avg_sq off by 1.16e-5 (gate 5.73e-6) and
the edge cases left exp_avg at 2.65e-7 and exp_avg_sq at 2.98e-7 (gate 2.38e-7); the betas now reach the kernel as doubles.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import optim_oracle as OO
from tests import optim_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd import optim as PO
    from painter_amd._lib import check, lib

BETAS, EPS = (0.9, 0.95), 1e-8
CHUNK = 8192


# ---------------------------------------------------------------------------------------------------------------- C ABI driver
class Table:
    """A PaOptTensor table over tensors the test placed itself.  recs: dicts p, g (or None), m, v, w16 (or None), group."""

    def __init__(self, recs):
        assert int(lib.pa_opt_chunk_elems()) == CHUNK
        rows, self.nchunks = [], 0
        for r in recs:
            n = r["p"].numel()
            for k in ("p", "g", "m", "v"):
                t = r.get(k)
                assert t is None and k == "g" or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
            w = r.get("w16")
            assert w is None or (w.is_cuda and w.dtype == torch.bfloat16 and w.is_contiguous() and w.numel() == n)
            ptr = lambda t: 0 if t is None else t.data_ptr()
            rows.append((ptr(r["p"]), ptr(r.get("g")), ptr(r["m"]), ptr(r["v"]), ptr(w), n, r["group"], self.nchunks))
            self.nchunks += (n + CHUNK - 1) // CHUNK
        self.recs, self.nt = recs, len(recs)
        self.dev = torch.from_numpy(np.array(rows, dtype=PO._REC).view(np.uint8).reshape(-1).copy()).cuda()
        self.steps = torch.zeros(self.nt, dtype=torch.float32, device="cuda")         # one count per record
        self.info = torch.zeros(2, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(max(int(lib.pa_grad_sumsq_workspace_bytes(self.nchunks)), 16), dtype=torch.uint8, device="cuda")

    def sumsq(self):
        check(lib.pa_grad_sumsq(self.dev.data_ptr(), self.nt, self.nchunks, self.info.data_ptr(), self.ws.data_ptr(), ops.stream()), "pa_grad_sumsq")
        return self.info

    def step(self, groups, scale=None, found_inf=None, max_norm=0.0, norm_info=True, betas=BETAS, eps=EPS):
        gs = PO._Groups()
        for gi, (lr, wd) in enumerate(groups):
            gs.lr[gi], gs.wd[gi] = lr, wd
        keep = [None if x is None else torch.tensor([float(x)], dtype=torch.float32, device="cuda") for x in (scale, found_inf)]
        check(lib.pa_adamw_step(self.dev.data_ptr(), self.nt, self.nchunks, ctypes.byref(gs), betas[0], betas[1], eps, self.steps.data_ptr(),
                                self.info.data_ptr() if norm_info else 0, ops.p(keep[0]), ops.p(keep[1]), float(max_norm), ops.stream()),
              "pa_adamw_step")
        torch.cuda.synchronize()

    def result(self):
        return {"p": [r["p"].cpu() for r in self.recs], "exp_avg": [r["m"].cpu() for r in self.recs],
                "exp_avg_sq": [r["v"].cpu() for r in self.recs], "step": self.steps.cpu().tolist()}


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _inputs(lengths, seed, nsteps, scale):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in lengths]
    grads = [[torch.randn(n, generator=g) * (5.0 if k == 1 else 0.2) * scale for n in lengths] for k in range(nsteps)]
    return params, grads


class Placed:
    """p, g, m, v of a list of tensors as views of four guarded flat device buffers at the element residues of an alignment class."""

    def __init__(self, lengths, cls, params, w16=False):
        self.bufs, self.views, self.guards = {}, {}, {}
        for q in "pgmv":
            self.bufs[q], self.views[q], self.guards[q] = C.guarded_views(lengths, cls[q], device="cuda")
            assert self.bufs[q].data_ptr() % 16 == 0
        for i, p in enumerate(params):
            self.views["p"][i].copy_(p)
            self.views["m"][i].zero_()
            self.views["v"][i].zero_()
        self.w16 = None
        if w16:                      # the bf16 copies sit at the same element residues as p: element offset r -> 2 r bytes past a 16-byte line
            self.w16buf = torch.full((self.bufs["p"].numel(),), 7.0, dtype=torch.bfloat16, device="cuda")
            offs, _ = C.flat_layout(lengths, cls["p"])
            self.w16 = [self.w16buf[o:o + n] for o, n in zip(offs, lengths)]
        self.before_w16 = None if not w16 else _bits(self.w16buf)

    def set_grads(self, grads):
        for v, g in zip(self.views["g"], grads):
            v.copy_(g)

    def records(self, group_of):
        return [dict(p=self.views["p"][i], g=self.views["g"][i], m=self.views["m"][i], v=self.views["v"][i],
                     w16=None if self.w16 is None else self.w16[i], group=group_of[i]) for i in range(len(group_of))]

    def assert_guards_untouched(self):
        want = _bits(torch.tensor([C.GUARD]))[0]
        for q in "pgmv":
            got = _bits(self.bufs[q])[self.guards[q].cpu()]
            assert bool((got == want).all()), "guard elements of the %s buffer were written" % q


def _run_table_case(label, lengths, placed, group_of, groups, params, grads, scale, max_norm):
    tab = Table(placed.records(group_of))
    for k, gk in enumerate(grads):
        placed.set_grads(gk)
        info = tab.sumsq()
        tab.step(groups, scale=scale, max_norm=max_norm)
        assert float(info[1]) == 0.0
    steps = [dict(grads=gk) for gk in grads]
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=BETAS, eps=EPS, scale=scale, max_norm=max_norm)
    C.check_against(label, tab.result(), ref, gates, yard)
    placed.assert_guards_untouched()
    return tab


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("cls", list(C.ALIGN_CLASSES))
def test_alignment_classes_match_float64_adamw(cls):
    """1. Views at element offsets 0..3 mod 4, lengths around the chunk size, three steps with loss scale 128 and max_norm 0.05
    (unscale and clip both live)."""
    params, grads = _inputs(C.LENGTHS, 11, 3, 128.0)
    placed = Placed(C.LENGTHS, C.ALIGN_CLASSES[cls], params)
    for q in "pgmv":
        res = {v.data_ptr() % 16 for v in placed.views[q]}
        assert (res == {0}) == (set(C.ALIGN_CLASSES[cls][q]) == {0}), (cls, q, res)
    group_of = [i % 3 for i in range(len(C.LENGTHS))]
    groups = [(1e-3, 0.05), (7.5e-4, 0.0), (5e-4, 0.05)]
    _run_table_case("alignment[%s]" % cls, C.LENGTHS, placed, group_of, groups, params, grads, 128.0, 0.05)


def test_decoder_pred_bucket_as_the_gradient_all_reduce_flattens_it():
    """2. Gradients are views of one torch.cat message in the engine's order (64, 64, 192, 3, 36864, 64 elements): those of
    decoder_pred.0.weight / .0.bias begin 12 bytes past a 16-byte boundary while parameters and moments are fresh allocations."""
    names = [n for n, _ in C.DECODER_PRED_BUCKET]
    lengths = [n for _, n in C.DECODER_PRED_BUCKET]
    params, grads = _inputs(lengths, 12, 3, 128.0)
    dev_p = [p.clone().cuda() for p in params]
    dev_m, dev_v = [torch.zeros_like(p) for p in dev_p], [torch.zeros_like(p) for p in dev_p]
    group_of = [1, 1, 0, 1, 0, 1]                                       # matrices decayed, one-dimensional tensors not
    groups = [(1e-3, 0.05), (1e-3, 0.0)]
    steps_dev = torch.zeros(len(lengths), dtype=torch.float32, device="cuda")
    for k in range(3):
        flat, views = C.bucket_views([g.cuda() for g in grads[k]])
        for n, v in zip(names, views):
            assert (v.data_ptr() % 16 != 0) == (n in ("decoder_pred.0.weight", "decoder_pred.0.bias")), n
        assert all(t.data_ptr() % 16 == 0 for t in dev_p + dev_m + dev_v)
        tab = Table([dict(p=dev_p[i], g=views[i], m=dev_m[i], v=dev_v[i], group=group_of[i]) for i in range(len(lengths))])
        tab.steps.copy_(steps_dev)
        info = tab.sumsq()
        tab.step(groups, scale=128.0, max_norm=0.05)
        assert float(info[1]) == 0.0
        steps_dev.copy_(tab.steps)
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, [dict(grads=gk) for gk in grads], betas=BETAS, eps=EPS, scale=128.0, max_norm=0.05)
    C.check_against("decoder_pred bucket", tab.result(), ref, gates, yard)


# ---------------------------------------------------------------------------------------------------------------- 3
def _sumsq_layouts():
    """(label, [gradient views]) for the layouts of tests 1 and 2; gradients are N(0, 1) pushed away from zero (|g| >= 0.5), so that
    every element's 3 g^2 stands clear of the fp32 rounding of the total."""
    g = torch.Generator().manual_seed(13)
    away = lambda x: torch.where(x < 0, -1.0, 1.0) * x.abs().clamp_min(0.5)
    out = []
    for name, cls in C.ALIGN_CLASSES.items():
        buf, views, guard = C.guarded_views(C.LENGTHS, cls["g"], device="cuda")
        for v in views:
            v.copy_(away(torch.randn(v.numel(), generator=g)))
        out.append((name, views))
    flat, views = C.bucket_views([away(torch.randn(n, generator=g)).cuda() for _, n in C.DECODER_PRED_BUCKET])
    out.append(("bucket", views))
    return out


def _sumsq_table(views):
    scratch = [torch.zeros(v.numel(), device="cuda") for v in views]          # p, m, v are not read by pa_grad_sumsq
    return Table([dict(p=s, g=v, m=s, v=s, group=0) for s, v in zip(scratch, views)])


def _probe_positions(n):
    """First element, elements 3 and 4, the last of a chunk and the first of the next, the last two -- those that exist."""
    return sorted({i for i in (0, 3, 4, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, n - 2, n - 1) if 0 <= i < n})


def test_grad_sumsq_reads_every_element_exactly_once():
    """3. Part A: a NaN or an inf planted at any probed position is seen.  Part B: the norm is the float64 norm within 2e-6, and doubling
    one element changes the sum by that element's 3 g^2 -- an element read twice, or skipped, shows.  The guard elements around the
    views hold 1e30: one of them read would overflow the sum."""
    for label, views in _sumsq_layouts():
        tab = _sumsq_table(views)
        info = tab.sumsq()
        torch.cuda.synchronize()
        base = float(info[0])
        exact = sum(float((v.double() ** 2).sum()) for v in views)
        assert float(info[1]) == 0.0 and np.isfinite(base), label
        err = abs(base ** 0.5 - exact ** 0.5) / exact ** 0.5
        print("sumsq[%s]: norm rel err %.3e (gate 2e-6)" % (label, err))
        assert err <= 2e-6, (label, base, exact)
        for ti, v in enumerate(views):
            pos = _probe_positions(v.numel())
            keep = v[pos].clone()
            # Part A, batched: the flags of all probes of this tensor are collected on the device and read once
            flags = []
            for bad in (float("nan"), float("inf")):
                for i in pos:
                    old = v[i].clone()
                    v[i] = bad
                    flags.append(tab.sumsq()[1].clone())
                    v[i] = old
            flags = torch.stack(flags).cpu()
            assert bool((flags != 0).all()), (label, ti, pos, flags.tolist())
            # Part B
            sums = []
            for i in pos:
                old = v[i].clone()
                v[i] = old * 2
                sums.append(tab.sumsq()[0].clone())
                v[i] = old
            sums = torch.stack(sums).cpu().double()
            assert torch.equal(v[pos], keep)
            for i, s, gi in zip(pos, sums.tolist(), keep.cpu().double().tolist()):
                # fp32 rounding of the total: per-chunk fp32 partial sums, float64 across chunks, one rounding of the result -- a few
                # ulps of `base` cover the changed partial sum and the two final roundings
                assert abs((s - base) - 3.0 * gi * gi) <= 8 * 2.0 ** -24 * max(base, s), (label, ti, i, s - base, 3.0 * gi * gi)
        info = tab.sumsq()
        assert float(info[0]) == base and float(info[1]) == 0.0, label         # everything was put back


# ---------------------------------------------------------------------------------------------------------------- 4
def _optim_result(opt, dev_p):
    sd = opt.state_dict()["state"]
    out = {"p": [p.detach().cpu() for p in dev_p], "exp_avg": [], "exp_avg_sq": [], "step": []}
    for i, p in enumerate(dev_p):
        st = sd.get(i)
        out["exp_avg"].append(st["exp_avg"].cpu() if st else torch.zeros(p.shape))
        out["exp_avg_sq"].append(st["exp_avg_sq"].cpu() if st else torch.zeros(p.shape))
        out["step"].append(float(st["step"]) if st else 0.0)
    return out


def _oracle_result(params, steps, cfg, scale, max_norm):
    ora_p = [p.clone() for p in params]
    state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in params]
    for st in steps:
        if st.get("skip"):
            continue
        OO.scaled_clipped_step(ora_p, st["grads"], state, cfg, scale, max_norm, BETAS[0], BETAS[1], EPS)
    return {"p": ora_p, "exp_avg": [s["exp_avg"] for s in state], "exp_avg_sq": [s["exp_avg_sq"] for s in state],
            "step": [float(s["step"]) for s in state]}


PARTIAL_SHAPES = [(33, 65), (8193,), (5,), (4097,)]


def _partial_case(which):
    g = torch.Generator().manual_seed(14)
    params = [torch.randn(s, generator=g) for s in PARTIAL_SHAPES]
    grad = lambda: [torch.randn(s, generator=g) * 0.3 * 128.0 for s in PARTIAL_SHAPES]
    steps = []
    if which == "late_and_never":               # (a) parameter 2: None in steps 1-4, live from step 5; parameter 3: never
        for k in range(6):
            gs = grad()
            steps.append(dict(grads=[gs[0], gs[1], gs[2] if k >= 4 else None, None]))
    elif which == "requires_grad_switched_on":  # (b) parameter 1 is frozen for three steps; parameter 3: never
        for k in range(5):
            gs = grad()
            steps.append(dict(grads=[gs[0], gs[1] if k >= 3 else None, gs[2], None], frozen=[1] if k < 3 else []))
    else:                                       # (c) a step skipped by found_inf between two live steps; parameter 3: never
        for k in range(3):
            gs = grad()
            steps.append(dict(grads=[gs[0], gs[1], gs[2], None], skip=(k == 1)))
    return params, steps


@pytest.mark.parametrize("which", ["late_and_never", "requires_grad_switched_on", "skipped_between_live_steps"])
def test_partial_gradients_keep_torchs_per_parameter_steps(which):
    """4. One group of four parameters; torch.optim.AdamW advances a parameter's own step only when it has a gradient.  Before the
    step counts became per parameter, (a) and (b) failed here: the late parameter took the group's count (steps [6, 6, 6, 6] for
    torch's [6, 6, 2, 0]) and about half of its first update."""
    params, steps = _partial_case(which)
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    opt = PO.AdamW([{"params": dev_p, "lr": 1e-2, "weight_decay": 0.05}], lr=1e-2, betas=BETAS, eps=EPS)
    scale_t = torch.tensor(128.0, device="cuda")
    for st in steps:
        for i, (p, gr) in enumerate(zip(dev_p, st["grads"])):
            p.requires_grad_(i not in st.get("frozen", []))
            p.grad = None if gr is None else gr.clone().cuda()
        opt.grad_sumsq()
        opt.step(grad_scale=scale_t, max_norm=0.05, found_inf=torch.tensor(1.0 if st.get("skip") else 0.0, device="cuda"))
    got = _optim_result(opt, dev_p)
    group_of, groups = [0] * 4, [(1e-2, 0.05)]
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=BETAS, eps=EPS, scale=128.0, max_norm=0.05)
    print("partial[%s]: steps device %s torch %s" % (which, got["step"], ref["step"]))
    C.check_against("partial[%s]" % which, got, ref, gates, yard)
    ora = _oracle_result(params, steps, [groups[0]] * 4, 128.0, 0.05)
    assert ora["step"] == ref["step"]
    for q in C.QUANTITIES:
        for a, b in zip(got[q], ora[q]):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7 if q != "exp_avg_sq" else 1e-9), (which, q)
    # the parameter that never had a gradient: bit-identical, and no moments moved
    assert torch.equal(_bits(dev_p[3]), _bits(params[3])) and got["step"][3] == 0.0
    st3 = opt.state.get(dev_p[3], {})
    assert not st3 or (not st3["exp_avg"].any() and not st3["exp_avg_sq"].any())


def test_checkpoints_with_unequal_steps_in_a_group_interchange_with_torch_adamw():
    """A torch.optim.AdamW checkpoint whose parameters of one group carry different steps loads into painter_amd.optim.AdamW, and
    the reverse; both continue to the same parameters at the gate."""
    import copy
    params, steps = _partial_case("late_and_never")
    more = _partial_case("skipped_between_live_steps")[1]
    more = [dict(grads=[gs["grads"][0], gs["grads"][1], gs["grads"][2], None]) for gs in more]
    mk = lambda: [torch.nn.Parameter(p.clone().cuda()) for p in params]
    group_of, groups = [0] * 4, [(1e-2, 0.05)]

    def drive(opt, ps, sts):
        for st in sts:
            for p, gr in zip(ps, st["grads"]):
                p.grad = None if gr is None else (gr / 128.0).cuda()
            opt.step()

    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps + more, betas=BETAS, eps=EPS, scale=128.0)
    # torch -> ours
    tp, op = mk(), mk()
    topt = torch.optim.AdamW([{"params": tp}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)
    drive(topt, tp, steps)
    sd = copy.deepcopy(topt.state_dict())
    assert sorted(float(s["step"]) for s in sd["state"].values()) == [2.0, 6.0, 6.0]
    ours = PO.AdamW([{"params": op}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)
    with torch.no_grad():
        for a, b in zip(op, tp):
            a.copy_(b)
    ours.load_state_dict(sd)
    assert [float(ours.state[p]["step"]) for p in op[:3]] == [6.0, 6.0, 2.0]
    drive(ours, op, more)
    got = _optim_result(ours, op)
    C.check_against("checkpoint torch -> fused", got, ref, gates, yard)
    # ours -> torch
    op2, tp2 = mk(), mk()
    ours2 = PO.AdamW([{"params": op2}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)
    drive(ours2, op2, steps)
    sd2 = copy.deepcopy(ours2.state_dict())
    st = [sd2["state"][i]["step"] for i in sorted(sd2["state"])]
    assert [float(s) for s in st] == [6.0, 6.0, 2.0] + [0.0] * (len(st) - 3) and all(s.dim() == 0 for s in st)
    assert len({s.untyped_storage().data_ptr() for s in st}) == len(st)                    # independent tensors
    topt2 = torch.optim.AdamW([{"params": tp2}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)
    with torch.no_grad():
        for a, b in zip(tp2, op2):
            a.copy_(b)
    topt2.load_state_dict(sd2)
    drive(topt2, tp2, more)
    got2 = {"p": [p.detach().cpu() for p in tp2]}
    for q in ("exp_avg", "exp_avg_sq"):
        got2[q] = [topt2.state[p][q].cpu() if p in topt2.state else torch.zeros(p.shape) for p in tp2]
    got2["step"] = [float(topt2.state[p]["step"]) if p in topt2.state else 0.0 for p in tp2]
    C.check_against("checkpoint fused -> torch", got2, ref, gates, yard)


def _result_in_param_order(opt, dev_p, group_of, ngroups):
    """_optim_result for parameters spread over several groups: state_dict() numbers them in group order."""
    order = [i for gi in range(ngroups) for i in range(len(dev_p)) if group_of[i] == gi]
    got = _optim_result(opt, [dev_p[i] for i in order])
    back = {j: k for k, j in enumerate(order)}
    return {q: [got[q][back[i]] for i in range(len(dev_p))] for q in got}


def test_state_dict_between_steps_leaves_the_live_step_views_in_place():
    """state_dict() hands out independent step tensors and must not swap them into the optimizer's own state: a run that
    checkpoints every epoch would write the counts of its first checkpoint for ever.  Step, state_dict(), step again: the second
    state_dict() and opt.state[p]["step"] show the advanced counts, and the second checkpoint continues under torch.optim.AdamW."""
    import copy
    params, steps = _partial_case("late_and_never")
    mk = lambda: [torch.nn.Parameter(p.clone().cuda()) for p in params]
    op = mk()
    ours = PO.AdamW([{"params": op}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)

    def drive(opt, ps, sts):
        for st in sts:
            for p, gr in zip(ps, st["grads"]):
                p.grad = None if gr is None else (gr / 128.0).cuda()
            opt.step()

    drive(ours, op, steps[:2])
    sd1 = ours.state_dict()
    assert [float(sd1["state"][i]["step"]) for i in range(4)] == [2.0, 2.0, 0.0, 0.0]
    drive(ours, op, steps[2:5])
    sd2 = ours.state_dict()
    assert [float(sd1["state"][i]["step"]) for i in range(4)] == [2.0, 2.0, 0.0, 0.0]          # the first checkpoint is a snapshot
    assert [float(sd2["state"][i]["step"]) for i in range(4)] == [5.0, 5.0, 1.0, 0.0]
    assert [float(ours.state[p]["step"]) for p in op] == [5.0, 5.0, 1.0, 0.0]
    base = ours._steps.untyped_storage().data_ptr()
    assert all(ours.state[p]["step"].untyped_storage().data_ptr() == base for p in op)          # still views of the one array
    assert all(sd2["state"][i]["step"].untyped_storage().data_ptr() != base for i in range(4))
    tp = mk()
    with torch.no_grad():
        for a, b in zip(tp, op):
            a.copy_(b)
    topt = torch.optim.AdamW([{"params": tp}], lr=1e-2, weight_decay=0.05, betas=BETAS, eps=EPS)
    topt.load_state_dict(copy.deepcopy(sd2))
    drive(topt, tp, steps[5:])
    drive(ours, op, steps[5:])
    ref, gates, yard = C.reference_and_gates(params, [0] * 4, [(1e-2, 0.05)], steps, betas=BETAS, eps=EPS, scale=128.0)
    C.check_against("state_dict between steps, fused", _optim_result(ours, op), ref, gates, yard)
    got = {"p": [p.detach().cpu() for p in tp], "step": [float(topt.state[p]["step"]) for p in tp]}
    for q in ("exp_avg", "exp_avg_sq"):
        got[q] = [topt.state[p][q].cpu() for p in tp]
    C.check_against("state_dict between steps, torch continues", got, ref, gates, yard)


def test_step_array_grows_past_64_with_unequal_counts_in_place():
    """60 parameters in two groups take unequal numbers of steps (the step array holds 64 elements), then add_param_group brings
    ten more: the array is reallocated, the old counts are copied and every view re-pointed.  Two more steps, against float64."""
    g = torch.Generator().manual_seed(19)
    sizes = [5 + (i * 37) % 300 for i in range(70)]
    params = [torch.randn(n, generator=g) for n in sizes]
    group_of = [i % 2 for i in range(60)] + [2] * 10
    groups = [(1e-2, 0.05), (5e-3, 0.0), (2e-3, 0.05)]
    steps = []
    for k in range(5):
        gs = [torch.randn(n, generator=g) * 0.3 * 128.0 for n in sizes]
        live = lambda i: (i >= 60 and k >= 3) or (i < 60 and (i % 3 != k % 3 or k >= 3))       # before the growth each sits out one step
        steps.append(dict(grads=[gs[i] if live(i) else None for i in range(70)]))
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    opt = PO.AdamW([{"params": [dev_p[i] for i in range(60) if group_of[i] == gi], "lr": groups[gi][0], "weight_decay": groups[gi][1]} for gi in range(2)],
                   lr=1e-3, betas=BETAS, eps=EPS)
    scale_t = torch.tensor(128.0, device="cuda")
    for k, st in enumerate(steps):
        if k == 3:
            assert opt._steps.numel() == 64 and sorted(set(opt._steps[:60].cpu().tolist())) == [2.0]
            held = opt.state[dev_p[7]]["step"]
            opt.add_param_group({"params": dev_p[60:], "lr": groups[2][0], "weight_decay": groups[2][1]})
        for p, gr in zip(dev_p, st["grads"]):
            p.grad = None if gr is None else gr.clone().cuda()
        opt.grad_sumsq()
        opt.step(grad_scale=scale_t, max_norm=0.05)
    assert opt._steps.numel() == 128 and float(held) == 2.0                       # the old array was left behind, not advanced
    base = opt._steps.untyped_storage().data_ptr()
    assert all(opt.state[p]["step"].untyped_storage().data_ptr() == base for p in dev_p)
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=BETAS, eps=EPS, scale=128.0, max_norm=0.05)
    assert ref["step"] == [4.0] * 60 + [2.0] * 10
    C.check_against("step array grows", _result_in_param_order(opt, dev_p, group_of, 3), ref, gates, yard)


def test_replaced_parameter_or_moment_storage_is_checked_before_the_launch():
    """The kernel gets raw pointers.  A moment or a parameter whose storage was replaced after its first step (a hand-edited state,
    `p.data = ...`) is checked again on the host and refused there; nothing is launched with it."""
    p = torch.nn.Parameter(torch.ones(300, device="cuda"))
    opt = PO.AdamW([p], lr=1e-2)
    p.grad = torch.full_like(p, 0.5)
    opt.step()
    after = p.detach().clone()
    opt.state[p]["exp_avg"] = torch.zeros(600, device="cuda")[::2]                   # right size, not contiguous
    with pytest.raises(RuntimeError, match="exp_avg"):
        opt.step()
    opt.state[p]["exp_avg"] = torch.zeros(300, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="exp_avg"):
        opt.step()
    opt.state[p]["exp_avg"] = torch.zeros(300, device="cuda")
    p.grad = None
    p.data = torch.ones(300)                                                         # moved to the host
    with pytest.raises(RuntimeError, match="parameters must be"):
        opt.step()
    p.data = after.clone()
    p.grad = torch.full_like(p, 0.5)
    opt.step()                                                                       # valid again: runs
    assert float(opt.state[p]["step"]) == 2.0 and not torch.equal(p.detach(), after)


def test_released_parameter_with_a_stale_gradient_in_a_second_group():
    """Case (b) over two groups with different lr / weight decay: parameter 1 (group 1) is frozen for three steps while it still
    holds a gradient from earlier -- torch.optim.AdamW and this class both leave a frozen parameter alone -- and is then released.
    It gets the last step slot, so the table's order differs from the group order and its group index has to be looked up."""
    g = torch.Generator().manual_seed(20)
    shapes = [(33, 65), (8193,), (5,), (4097,)]
    params = [torch.randn(s, generator=g) for s in shapes]
    group_of, groups = [0, 1, 1, 0], [(1e-2, 0.05), (2e-3, 0.0)]
    steps, stale = [], torch.randn(shapes[1], generator=g) * 1e3
    for k in range(5):
        gs = [torch.randn(s, generator=g) * 0.3 * 128.0 for s in shapes]
        steps.append(dict(grads=[gs[0], gs[1] if k >= 3 else None, gs[2], gs[3]]))
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    opt = PO.AdamW([{"params": [dev_p[0], dev_p[3]], "lr": 1e-2, "weight_decay": 0.05}, {"params": [dev_p[1], dev_p[2]], "lr": 2e-3, "weight_decay": 0.0}],
                   lr=1e-3, betas=BETAS, eps=EPS)
    scale_t = torch.tensor(128.0, device="cuda")
    for k, st in enumerate(steps):
        for i, (p, gr) in enumerate(zip(dev_p, st["grads"])):
            p.grad = gr.clone().cuda() if gr is not None else stale.clone().cuda()
        dev_p[1].requires_grad_(k >= 3)
        opt.grad_sumsq()
        opt.step(grad_scale=scale_t, max_norm=0.05)
        if k == 2:
            assert torch.equal(_bits(dev_p[1]), _bits(params[1]))                  # the stale gradient was not applied
    assert [id(p) for p in opt._slot] == [id(dev_p[i]) for i in (0, 3, 2, 1)]
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=BETAS, eps=EPS, scale=128.0, max_norm=0.05)
    assert ref["step"] == [5.0, 2.0, 5.0, 5.0]
    C.check_against("released into a second group", _result_in_param_order(opt, dev_p, group_of, 2), ref, gates, yard)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("cls", ["none", "p", "all"])
def test_bf16_copies_are_the_cast_of_the_new_parameter_and_survive_a_skip(cls):
    """5. With w16 set the update pass writes the GEMM operand copy itself: bit for bit ops.cast_bf16 of the updated parameter, tails
    of the last chunk included; a skipped step (found_inf, NaN gradient, overflowed sum of squares) leaves copy, p, m, v and the step
    counts bit-identical."""
    params, grads = _inputs(C.LENGTHS, 15, 2, 128.0)
    placed = Placed(C.LENGTHS, C.ALIGN_CLASSES[cls], params, w16=True)
    group_of, groups = [i % 2 for i in range(len(C.LENGTHS))], [(1e-2, 0.05), (5e-3, 0.0)]
    tab = Table(placed.records(group_of))
    placed.set_grads(grads[0])
    tab.sumsq()
    tab.step(groups, scale=128.0, max_norm=0.05)
    for i, n in enumerate(C.LENGTHS):
        want = ops.cast_bf16(placed.views["p"][i].clone())
        assert torch.equal(_bits(placed.w16[i]), _bits(want)), (cls, n)
        assert not torch.equal(placed.views["p"][i].cpu(), params[i])
    inside = torch.zeros(placed.w16buf.numel(), dtype=torch.bool)
    for o, n in zip(C.flat_layout(C.LENGTHS, C.ALIGN_CLASSES[cls]["p"])[0], C.LENGTHS):
        inside[o:o + n] = True
    assert torch.equal(_bits(placed.w16buf)[~inside], placed.before_w16[~inside])          # nothing outside the copies was written
    snap = lambda: [_bits(placed.bufs[q]) for q in "pmv"] + [_bits(placed.w16buf), _bits(tab.steps)]
    before = snap()
    assert tab.steps.cpu().tolist() == [1.0] * len(C.LENGTHS)
    # skipped: found_inf set by the scaler
    placed.set_grads(grads[1])
    tab.sumsq()
    tab.step(groups, scale=128.0, found_inf=1.0, max_norm=0.05)
    assert all(torch.equal(a, b) for a, b in zip(before, snap())), "found_inf"
    # skipped: a NaN in the last element of the tensor with the odd tail
    bad = [g.clone() for g in grads[1]]
    bad[C.LENGTHS.index(8193)][-1] = float("nan")
    placed.set_grads(bad)
    assert float(tab.sumsq()[1]) != 0.0
    tab.step(groups, scale=128.0, max_norm=0.05)
    assert all(torch.equal(a, b) for a, b in zip(before, snap())), "NaN gradient"
    # skipped: finite gradients whose sum of squares overflows fp32 although no square and no thread's share of 32 squares does
    # (9e36 each, 2.9e38 per thread, inf per chunk): the non-finite count stays 0, the sum itself is the signal
    placed.set_grads([torch.full((n,), 3e18) for n in C.LENGTHS])
    info = tab.sumsq()
    assert float(info[1]) == 0.0 and not np.isfinite(float(info[0]))
    tab.step(groups, scale=128.0, max_norm=0.05)
    assert all(torch.equal(a, b) for a, b in zip(before, snap())), "overflowed sum of squares"
    # and a live step afterwards moves everything again
    placed.set_grads(grads[1])
    tab.sumsq()
    tab.step(groups, scale=128.0, max_norm=0.05)
    assert tab.steps.cpu().tolist() == [2.0] * len(C.LENGTHS)
    for i in range(len(C.LENGTHS)):
        assert torch.equal(_bits(placed.w16[i]), _bits(ops.cast_bf16(placed.views["p"][i].clone())))
    placed.assert_guards_untouched()


def test_bound_models_bf16_operand_copies_equal_the_cast_of_their_parameters():
    """5, through bind_model on the small bf16 model: after two steps every buffer of _hot.shadow_buffers() is ops.cast_bf16 of its
    parameter, bit for bit."""
    from functools import partial

    import torch.nn as nn

    from oracle import painter_oracle as O
    from painter_amd import models_painter
    cfg = O.small_config()
    m = models_painter.Painter(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                               drop_path_rate=0.0, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), use_rel_pos=True,
                               decoder_embed_dim=cfg.decoder_embed_dim, compute_dtype="bf16")
    m.load_state_dict(O.random_params(cfg, 7), strict=True)
    m = m.cuda().eval()
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, 2, 8, "random")
    opt = PO.AdamW(m.parameters(), lr=1e-2, weight_decay=0.05).bind_model(m)
    for _ in range(2):
        opt.zero_grad()
        loss, _, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.cuda(), valid=valid.clone().cuda())
        loss.backward()
        opt.step(max_norm=3.0)
    by_ptr = {p.data_ptr(): (n, p) for n, p in m.named_parameters()}
    shadows = m._hot.shadow_buffers()
    assert len(shadows) >= 4 * cfg.depth
    for ptr, buf in shadows.items():
        name, p = by_ptr[ptr]
        assert buf.numel() == p.numel(), name
        assert torch.equal(_bits(buf.reshape(-1)), _bits(ops.cast_bf16(p.detach().reshape(-1).clone()))), name


# ---------------------------------------------------------------------------------------------------------------- 6
def test_reference_group_shape_52_groups_over_352_tensors():
    """6. 26 layer ids x {decay, no decay} over the small configuration's parameter list at depth 24, two steps with the learning
    rate changed in between (as adjust_learning_rate does): find_tensor over hundreds of records, the group tables near their limit."""
    names, sizes, gidx, groups = C.painter_shaped_groups()
    g = torch.Generator().manual_seed(16)
    params = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * 0.2 * 128.0 for n in sizes] for _ in range(2)]
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    pg = [{"params": [dev_p[i] for i in range(len(sizes)) if gidx[i] == gi], "lr": lr, "weight_decay": wd, "lr_scale": lr / 1e-3}
          for gi, (lr, wd) in enumerate(groups)]
    opt = PO.AdamW(pg, lr=1e-3, betas=BETAS, eps=EPS)
    assert len(opt.param_groups) == 52
    scale_t = torch.tensor(128.0, device="cuda")
    steps = []
    for k, sched in enumerate((1.0, 0.37)):
        for grp in opt.param_groups:
            grp["lr"] = 1e-3 * sched * grp["lr_scale"]
        steps.append(dict(grads=grads[k], lrs=[1e-3 * sched * (lr / 1e-3) for lr, _ in groups]))
        for p, gr in zip(dev_p, grads[k]):
            p.grad = gr.clone().cuda()
        opt.grad_sumsq()
        opt.step(grad_scale=scale_t, max_norm=0.05)
    # state_dict() numbers the parameters in group order
    order = [i for gi in range(len(groups)) for i in range(len(sizes)) if gidx[i] == gi]
    got = _optim_result(opt, [dev_p[i] for i in order])
    back = {j: k for k, j in enumerate(order)}
    got = {q: [got[q][back[i]] for i in range(len(sizes))] for q in got}
    ref, gates, yard = C.reference_and_gates(params, gidx, groups, steps, betas=BETAS, eps=EPS, scale=128.0, max_norm=0.05)
    C.check_against("52 groups", got, ref, gates, yard)


def test_64_groups_are_accepted_and_65_raise():
    ps = [torch.nn.Parameter(torch.full((5,), 1.0, device="cuda")) for _ in range(65)]
    with pytest.raises(NotImplementedError):
        PO.AdamW([{"params": [p]} for p in ps], lr=1e-3)
    opt = PO.AdamW([{"params": [p], "lr": 1e-3 * (i + 1), "weight_decay": 0.0} for i, p in enumerate(ps[:64])], lr=1e-3, betas=BETAS)
    for p in ps[:64]:
        p.grad = torch.full_like(p, 0.5)
    opt.step()
    # a constant gradient's first update is lr (eps aside): the last group's learning rate reached its parameters
    got = torch.stack([p.detach() for p in ps[:64]]).cpu().double()
    want = 1.0 - 1e-3 * torch.arange(1, 65, dtype=torch.float64)[:, None].expand(64, 5)
    assert float((got - want).abs().max()) <= 2.0 ** -22
    with pytest.raises(NotImplementedError):
        PO.AdamW([{"params": [p]} for p in ps[:64]], lr=1e-3).add_param_group({"params": [ps[64]]})


# ---------------------------------------------------------------------------------------------------------------- 7
def test_three_hundred_steps_stay_within_torchs_own_fp32_drift():
    """7. 300 steps with constant hyper-parameters: the fp32 step counter and the double-precision pow of the bias corrections far
    from step 1.  The gate comes from the fp32 yardstick run of the same 300 steps."""
    shapes = [(257,), (31, 33), (8193,), (4,)]
    g = torch.Generator().manual_seed(17)
    params = [torch.randn(s, generator=g) for s in shapes]
    steps = [dict(grads=[torch.randn(s, generator=g) * 0.2 for s in shapes]) for _ in range(300)]
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    group_of, groups = [0, 0, 1, 1], [(1e-3, 0.05), (5e-4, 0.0)]
    opt = PO.AdamW([{"params": dev_p[:2], "lr": 1e-3, "weight_decay": 0.05}, {"params": dev_p[2:], "lr": 5e-4, "weight_decay": 0.0}],
                   lr=1e-3, betas=(0.9, 0.999), eps=EPS)
    dev_g = [torch.stack([st["grads"][i] for st in steps]).cuda() for i in range(4)]
    for k in range(300):
        for i, p in enumerate(dev_p):
            p.grad = dev_g[i][k]
        opt.step(max_norm=3.0)
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=(0.9, 0.999), eps=EPS, max_norm=3.0)
    C.check_against("300 steps", _optim_result(opt, dev_p), ref, gates, yard)


# ---------------------------------------------------------------------------------------------------------------- 8
def _edge_run(label, params, group_of, groups, steps, eps=EPS, frozen=()):
    dev_p = [torch.nn.Parameter(p.clone().cuda(), requires_grad=i not in frozen) for i, p in enumerate(params)]
    pg = [{"params": [dev_p[i] for i in range(len(params)) if group_of[i] == gi], "lr": lr, "weight_decay": wd} for gi, (lr, wd) in enumerate(groups)]
    opt = PO.AdamW(pg, lr=1e-3, betas=BETAS, eps=eps)
    for st in steps:
        for p, gr in zip(dev_p, st["grads"]):
            p.grad = None if gr is None else gr.clone().cuda()
        opt.step()
    order = [i for gi in range(len(groups)) for i in range(len(params)) if group_of[i] == gi]
    got = _optim_result(opt, [dev_p[i] for i in order])
    back = {j: k for k, j in enumerate(order)}
    got = {q: [got[q][back[i]] for i in range(len(params))] for q in got}
    ref, gates, yard = C.reference_and_gates(params, group_of, groups, steps, betas=BETAS, eps=eps)
    C.check_against(label, got, ref, gates, yard)
    return got, dev_p


EDGE_SHAPES = [(8193,), (33, 31), (5,)]


def _edge_inputs(seed=18):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s in EDGE_SHAPES]
    rnd = lambda: [torch.randn(s, generator=g) * 0.2 for s in EDGE_SHAPES]
    return g, params, rnd


def test_edge_zero_gradients_decay_moments_and_only_weight_decay_moves_p():
    """8. zero_grad(set_to_none=False): gradients of zeros are live gradients."""
    g, params, rnd = _edge_inputs()
    zeros = [torch.zeros(s) for s in EDGE_SHAPES]
    got, _ = _edge_run("edge[zero grads]", params, [0, 0, 1], [(1e-2, 0.05), (1e-2, 0.0)], [dict(grads=rnd()), dict(grads=zeros), dict(grads=zeros)])
    assert got["step"] == [3.0, 3.0, 3.0]


def test_edge_tiny_gradients():
    """8. Gradients of +-1e-20: their squares are fp32 subnormals."""
    g, params, rnd = _edge_inputs()
    tiny = lambda: [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0) * 1e-20 for s in EDGE_SHAPES]
    _edge_run("edge[+-1e-20]", params, [0, 0, 1], [(1e-2, 0.05), (1e-2, 0.0)], [dict(grads=tiny()), dict(grads=tiny())])


def test_edge_lr_zero_and_weight_decay_zero_groups():
    """8. A group with lr = 0 (moments move, parameters do not) next to one with weight_decay = 0."""
    g, params, rnd = _edge_inputs()
    got, dev_p = _edge_run("edge[lr 0 | wd 0]", params, [0, 1, 1], [(0.0, 0.05), (1e-2, 0.0)], [dict(grads=rnd()), dict(grads=rnd())])
    assert torch.equal(_bits(dev_p[0]), _bits(params[0])) and got["step"] == [2.0, 2.0, 2.0]


def test_edge_large_eps():
    """8. eps = 1e-3, the value the model-level tests train with."""
    g, params, rnd = _edge_inputs()
    _edge_run("edge[eps 1e-3]", params, [0, 0, 1], [(1e-2, 0.05), (1e-2, 0.0)], [dict(grads=rnd()), dict(grads=rnd())], eps=1e-3)


def test_edge_group_whose_parameters_are_all_frozen():
    """8. A group of frozen parameters next to a live one: untouched, without steps."""
    g, params, rnd = _edge_inputs()
    steps = [dict(grads=[a, None, None]) for a in (rnd()[0], rnd()[0])]
    got, dev_p = _edge_run("edge[frozen group]", params, [0, 1, 1], [(1e-2, 0.05), (1e-2, 0.05)], steps, frozen=(1, 2))
    assert got["step"] == [2.0, 0.0, 0.0]
    assert torch.equal(_bits(dev_p[1]), _bits(params[1])) and torch.equal(_bits(dev_p[2]), _bits(params[2]))
