"""Guard-band tests of include/painter_minmax.h, with the machinery of tests/guard_bands.py and tests/test_guard_bands_engines_gpu.py:
every case runs once the ordinary way and once with every device input, packed output and workspace at its exact size between 4 MiB of
0xFF on each side -- no guard byte may change, every entry point the case names must have been reached, and the two runs must agree byte
for byte (each case also compares itself with tests/painter_minmax_host.py in both runs)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import painter_minmax_cases as C
from tests import painter_minmax_host as H
from tests.guard_bands import abi_symbols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from tests.test_guard_bands_engines_gpu import run_case
    from tests.test_painter_minmax_gpu import case, check_result, default_palette, direct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("pa_minmax_workspace_bytes", "pa_minmax_decode", "pa_minmax_nearest", "pa_minmax_masks")


def _direct_odd(c):
    pic, want = case("thr19_c")                              # 5063 pixels, 6401 colours: nothing is a multiple of a tile
    return direct(c, pic, default_palette(), want)


def _direct_two_chunks(c):
    pic, want = case("two_blocks_33x65")
    return direct(c, pic, default_palette(), want)


def _direct_capacity(c):
    pic, pal = C.capacity_case()
    return direct(c, pic, pal, H.decode(pic, pal))


def _direct_slot_window(c):
    pic, pal = C.ties_case()
    return direct(c, pic, pal, H.decode(pic, pal), first=1, n_cap=2)


def _direct_one_pixel(c):
    pic, pal = np.array([[[7, 200, 90]]], np.uint8), H.with_background([[7, 200, 91]])
    return direct(c, pic, pal, H.decode(pic, pal))


def _engine(c):
    pic, want = case("few")
    dec = E.MinmaxDecode(c.dev(pic, "picture"))
    res = dec.result(with_bits=True)
    bits = res.pop("bits")
    check_result(res, want, *pic.shape[:2])
    entries = E.instance_results(dec, 3)
    return dict(res, bits=bits, out=dec.out, workspace=dec.workspace, text=np.frombuffer(json.dumps(entries).encode(), np.uint8))


GUARD_CASES = [
    ("direct-61x83-6401-colours", _direct_odd, [], ALL),
    ("direct-33x65-two-statistics-chunks", _direct_two_chunks, [], ALL),
    ("direct-16x16-16384-colours", _direct_capacity, [], ALL),
    ("direct-slot-window", _direct_slot_window, [], ALL),
    ("direct-one-pixel", _direct_one_pixel, [], ALL),
    ("engine-MinmaxDecode-instance_results", _engine, ["painter_engine"],
     ("pa_minmax_workspace_bytes", "pa_minmax_decode", "pa_minmax_masks", "pa_rle_encode", "pa_rle_encode_workspace_bytes")),
]


@pytest.mark.parametrize("fn,modules,symbols", [pytest.param(f, m, s, id=i) for i, f, m, s in GUARD_CASES])
def test_guard_bands(fn, modules, symbols, monkeypatch):
    run_case(fn, tuple(modules), tuple(symbols), monkeypatch)


def test_every_symbol_of_the_minmax_header_is_guarded():
    abi = abi_symbols(open(os.path.join(ROOT, "include", "painter_minmax.h")).read())
    assert abi == set(ALL)
    claimed = set()
    for _, _, _, symbols in GUARD_CASES:
        claimed |= {s for s in symbols if s.startswith("pa_minmax_")}
    assert abi - claimed == set(), "symbols of include/painter_minmax.h that no guard-band case places: %s" % sorted(abi - claimed)
