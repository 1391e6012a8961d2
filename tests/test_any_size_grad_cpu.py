"""The backward at a run-time size other than the constructed one, without a GPU: the oracle's gradients at another size against the
UNMODIFIED reference's (tests/golden/painter_any_size_grads_*.npz, tests/golden/make_golden_any_size_grads.py), the host side of
include/painter_anysize_grad.h, and the float64 statement of the rel-pos resize adjoint against torch's own autograd."""
import os

import pytest
import torch

from oracle import painter_oracle as O
from tests import any_size_cases as C
from tests import golden_util as G
from tests.any_size_grad_cases import DYADIC_PAIRS, RESIZE_PAIRS, resize_adjoint_statement, torch_resize_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "painter_anysize_grad.h")
SYMBOLS = {"pa_attn_any_bwd", "pa_attn_any_bwd_workspace_bytes", "pa_attn_any_bwd_launches", "pa_relpos_resize_bwd"}


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_oracle_gradients_at_another_size_equal_the_reference(name):
    """Digests at 1e-5, the gate tests/test_any_size_cpu.py uses for pred (the worst tensor seen at A, B and F: 1.3e-7)."""
    fx, fxi = G.load("painter_any_size_grads_%s.npz" % name), G.load("painter_any_size_grads_%s_dimgs.npz" % name)
    cfg = C.config(name)
    assert tuple(fx["size"]) == tuple(C.CASES[name][3]) != tuple(cfg.img_size)
    P = {k: v.clone().requires_grad_(True) for k, v in O.random_params(cfg, C.CASES[name][1]).items()}
    imgs, tgts, mask, valid = C.inputs(name)
    xi, xt = imgs.clone().requires_grad_(True), tgts.clone().requires_grad_(True)
    loss, _, _ = O.forward(P, cfg, xi, xt, mask, valid)
    loss.backward()
    ref = float(fx["loss"])
    assert abs(loss.item() - ref) < 1e-5 * abs(ref), (loss.item(), ref)
    G.check_grad_digests(fx, "", [(n, p.grad) for n, p in P.items()], 1e-5, 1e-5, 1e-5, sample_rtol=1e-5)
    full = lambda n: fx["grad_full/" + n] if "grad_full/" + n in fx.files else fx["grad/" + n]
    for n, p in P.items():
        if "rel_pos" in n:
            assert float(p.grad.abs().max()) > 0 and G.rel_err(p.grad.reshape(-1), full(n).reshape(-1)) < 1e-5, n
    assert float(P["pos_embed"].grad.abs().max()) > 0
    assert G.rel_err(xi.grad, fxi["dimgs"]) < 1e-5 and G.rel_err(xt.grad, fx["dtgts"]) < 1e-5


def test_header_is_parsed_and_built():
    from painter_amd import _lib, build
    from tests.guard_bands import abi_symbols
    assert abi_symbols(open(HEADER).read()) == SYMBOLS
    assert HEADER in [os.path.abspath(p) for p in _lib.MORE_HEADERS] and HEADER in build.headers()
    # additions only: neither include/painter_hip.h nor include/painter_anysize.h knows them
    assert not SYMBOLS & set(_lib.parse_header())
    assert not SYMBOLS & set(_lib.parse_header(os.path.join(ROOT, "include", "painter_anysize.h")))
    protos = _lib.parse_header(HEADER)
    assert set(protos) == SYMBOLS and len(protos["pa_attn_any_bwd"][1]) == 21 and len(protos["pa_relpos_resize_bwd"][1]) == 9
    assert len(protos["pa_attn_any_bwd_workspace_bytes"][1]) == 7 and protos["pa_attn_any_bwd_launches"][1] == []


@pytest.mark.parametrize("n_src,n_dst", sorted({(s, d) for sh, sw, dh, dw in RESIZE_PAIRS for s, d in ((sh, dh), (sw, dw))} | set(DYADIC_PAIRS) | {(15, 5)}))
def test_resize_adjoint_statement_is_torch_float64_autograd(n_src, n_dst):
    g = torch.randn((n_dst, 8), generator=torch.Generator().manual_seed(100 * n_src + n_dst), dtype=torch.float64)
    want, got = torch_resize_grad(g, n_src, torch.float64), resize_adjoint_statement(g, n_src)
    # (two float64 evaluations of the same coordinate may differ in its last bit)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_the_exact_chain_case_is_exact_through_the_resize_adjoint():
    """tests/test_attention_any_bwd_exact_gpu.py::test_exact_chain_through_the_resize_adjoint rests on this: the exact table gradient of its
    tie case on 8 x 5 (lengths 15 and 9, multiples of 1/32) through the adjoint to the stored lengths 45 and 27 -- CPU torch's float32
    autograd of the resize equals its float64 autograd and the statement, bit for bit."""
    from tests import exact_cases as X
    kind, grid, hd = X.ANY_BWD_CHAIN
    case, exp = X.any_case(kind, *grid, hd)
    nh, nw = 2 * case.Hp - 1, 2 * case.Wp - 1
    assert (nh, nw) == (15, 9) and (45, 15) in DYADIC_PAIRS and (27, 9) in DYADIC_PAIRS
    assert X.any_bwd_condition_failed(case, exp, X.tie_algebra(case), fp32=True) is None
    assert torch.equal(exp.drcat.float().double(), exp.drcat)
    for g, n_src in ((exp.drcat[:nh], 45), (exp.drcat[nh:], 27)):
        assert float(g.abs().max()) > 0
        want = resize_adjoint_statement(g, n_src)
        assert torch.equal(torch_resize_grad(g, n_src, torch.float64), want)
        assert torch.equal(torch_resize_grad(g.float(), n_src, torch.float32).double(), want)


@pytest.mark.parametrize("n_src,n_dst", DYADIC_PAIRS + [(15, 5)])
def test_dyadic_pairs_with_integer_gradients_are_exact_in_float32(n_src, n_dst):
    """The condition under which tests/test_any_size_grad_gpu.py may demand torch.equal of the kernel: on these length pairs, with integer
    d out in [-64, 64], torch's own float32 autograd equals its float64 autograd, and both equal the statement, bit for bit."""
    for hd in (64, 80):
        g = torch.randint(-64, 65, (n_dst, hd), generator=torch.Generator().manual_seed(100 * n_src + n_dst)).float()
        want = resize_adjoint_statement(g, n_src)
        assert torch.equal(torch_resize_grad(g, n_src, torch.float64), want)
        assert torch.equal(torch_resize_grad(g, n_src, torch.float32).double(), want)
