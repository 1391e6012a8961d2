"""Guard-band tests of include/painter_anysize_grad.h, with the machinery of tests/guard_bands.py and tests/test_guard_bands_engines_gpu.py
as tests/test_guard_bands_any_size_gpu.py uses it: every case runs once the ordinary way and once with every device operand, every output
and the workspace at its exact size between 4 MiB of 0xFF on each side -- no guard byte may change, every entry point the case names must
have been reached, and the two runs must agree byte for byte.  Behind the last sample's last key and last query row lies NaN, and so does
the workspace before the kernels write it."""
import os

import pytest
import torch

from tests.guard_bands import abi_symbols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops, ops_anysize
    from tests.test_guard_bands_engines_gpu import run_case
    from tests.test_kernels_gpu import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("pa_attn_any_bwd", "pa_attn_any_bwd_workspace_bytes", "pa_attn_any_bwd_launches", "pa_relpos_resize_bwd")
F32, BF16 = torch.float32, torch.bfloat16


def _case(T, Hp, Wp, hd, B=2, H=2, src=(15, 7)):
    """One attention backward on the grid, and its table gradient carried back to the lengths of a model built at 8 x 4 tokens."""
    def fn(c):
        L, dh, dw = Hp * Wp, 2 * Hp - 1, 2 * Wp - 1
        rel_h, rel_w = gen((dh, hd), 2, 0.2), gen((dw, hd), 3, 0.2)
        rcat = c.dev(ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), "rcat")
        rcatT = c.dev(ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T), "rcatT")
        qkv = c.dev(gen((B * L, 3 * H * hd), 1, 1.0, T), "qkv")
        dout = c.dev(gen((B * L, H * hd), 4, 1.0, T), "dout")
        out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, hd ** -0.5)
        out, lse = c.dev(out, "out"), c.dev(lse, "lse")
        n0 = ops_anysize.attn_any_bwd_launches()
        dqkv, drcat = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, hd ** -0.5)
        assert ops_anysize.attn_any_bwd_launches() == n0 + 1
        dtab = ops_anysize.relpos_resize_bwd(drcat, src[0], src[1], dh, dw)
        assert torch.isfinite(dqkv.float()).all() and torch.isfinite(drcat).all() and torch.isfinite(dtab).all()
        return dict(dqkv=dqkv, drcat=drcat, dtab=dtab)
    return fn


GUARD_CASES = [("%s-%dx%d-hd%d" % (str(T)[6:], Hp, Wp, hd), _case(T, Hp, Wp, hd), ["ops_anysize"], ALL)
               for T in (F32, BF16) for (Hp, Wp) in ((10, 5), (3, 11)) for hd in (64, 80)]


@pytest.mark.parametrize("fn,modules,symbols", [pytest.param(f, m, s, id=i) for i, f, m, s in GUARD_CASES])
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, tuple(modules), tuple(symbols), monkeypatch)


def test_every_symbol_of_the_anysize_grad_header_is_guarded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_anysize_grad.h")).read())
    assert abi == set(ALL)
    claimed = set()
    for _, _, _, symbols in GUARD_CASES:
        claimed |= set(symbols)
    assert abi - claimed == set(), "symbols of include/painter_anysize_grad.h that no guard-band case places: %s" % sorted(abi - claimed)
