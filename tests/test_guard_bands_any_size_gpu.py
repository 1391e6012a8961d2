"""Guard-band tests of include/painter_anysize.h, with the machinery of tests/guard_bands.py and tests/test_guard_bands_engines_gpu.py:
every case runs once the ordinary way and once with every device operand and every output at its exact size between 4 MiB of 0xFF on
each side -- no guard byte may change, every entry point the case names must have been reached, and the two runs must agree byte for
byte.  For the attention that is the point of the kernel: behind the last sample's last key, and behind its last query row, lies NaN."""
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
ALL = ("pa_attn_any_fwd", "pa_attn_any_launches", "pa_relpos_resize")
F32, BF16 = torch.float32, torch.bfloat16


def _case(T, Hp, Wp, hd, B=2, H=2, nb=2, src=(15, 7)):
    """Tables of a model built at 8 x 4 tokens, resized for the grid, packed, and one attention forward on them."""
    def fn(c):
        L, dh, dw = Hp * Wp, 2 * Hp - 1, 2 * Wp - 1
        hs = [c.dev(gen((src[0], hd), 30 + k, 0.2), "rel_pos_h %d" % k) for k in range(nb)]
        ws = [c.dev(gen((src[1], hd), 40 + k, 0.2), "rel_pos_w %d" % k) for k in range(nb)]
        tabs = c.dev(torch.tensor([t.data_ptr() for t in hs] + [t.data_ptr() for t in ws], dtype=torch.int64), "table addresses")
        resized = ops_anysize.relpos_resize(tabs, nb, src[0], src[1], dh, dw, hd)
        rcat = c.dev(ops.relpos_pack_batch(ops_anysize.table_addresses(resized, dh), nb, Hp, Wp, hd, T)[0][nb - 1], "rcat")
        qkv = c.dev(gen((B * L, 3 * H * hd), 1, 1.0, T), "qkv")
        n0 = ops_anysize.attn_any_launches()
        out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, hd ** -0.5)
        assert ops_anysize.attn_any_launches() == n0 + 1
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(resized).all()
        return dict(resized=resized, out=out, lse=lse)
    return fn


GUARD_CASES = [("%s-%dx%d-hd%d" % (str(T)[6:], Hp, Wp, hd), _case(T, Hp, Wp, hd), ["ops_anysize"], ALL)
               for T in (F32, BF16) for (Hp, Wp) in ((10, 5), (3, 11)) for hd in (64, 80)]


@pytest.mark.parametrize("fn,modules,symbols", [pytest.param(f, m, s, id=i) for i, f, m, s in GUARD_CASES])
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, tuple(modules), tuple(symbols), monkeypatch)


def test_every_symbol_of_the_anysize_header_is_guarded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_anysize.h")).read())
    assert abi == set(ALL)
    claimed = set()
    for _, _, _, symbols in GUARD_CASES:
        claimed |= set(symbols)
    assert abi - claimed == set(), "symbols of include/painter_anysize.h that no guard-band case places: %s" % sorted(abi - claimed)
