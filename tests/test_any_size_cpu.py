"""The oracle at a run-time size other than the constructed one (its get_rel_pos / get_abs_pos interpolation branches) against the
UNMODIFIED reference's output at that size (tests/golden/painter_any_size*.npz, tests/golden/make_golden_any_size.py), and the host side of
include/painter_anysize.h."""
import os

import numpy as np
import pytest
import torch

from oracle import painter_oracle as O
from tests import any_size_cases as C
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "painter_anysize.h")
SYMBOLS = {"pa_attn_any_fwd", "pa_attn_any_launches", "pa_relpos_resize"}


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_oracle_at_another_size_equals_the_reference(name):
    _, seed_p, _, size, fname = C.CASES[name]
    fx = G.load(fname)
    cfg = C.config(name)
    assert tuple(fx[name + "/size"]) == tuple(size) != tuple(cfg.img_size)
    assert float(fx[name + "/zero_tables_move"]) > 10 * C.FP32_GATE          # a wrong (or missing) bias would be visible in pred
    P = O.random_params(cfg, seed_p)
    assert P["blocks.0.attn.rel_pos_h"].shape[0] != 2 * C.run_config(name).grid[0] - 1      # the tables ARE resized in this run
    imgs, tgts, mask, valid = C.inputs(name)
    with torch.no_grad():
        loss, pred, _ = O.forward(P, cfg, imgs, tgts, mask, valid)
    ref = float(fx[name + "/loss"])
    assert abs(float(loss) - ref) < 1e-5 * abs(ref), (float(loss), ref)
    assert pred.shape == fx[name + "/pred"].shape
    e = G.rel_err(pred, fx[name + "/pred"])
    assert e < 1e-5, e


def test_stored_bf16_yardstick_is_the_deviation_of_the_stored_bf16_pred():
    bf = G.load(C.BF16_FILE)
    for name, case in C.CASES.items():
        fx = G.load(case[4])
        pb = torch.from_numpy(bf[name + "/pred_bf16_bits"].view(np.int16)).view(torch.bfloat16).float()
        dev = G.rel_fro(pb, fx[name + "/pred"])
        stored = float(fx[name + "/bf16_dev"])
        assert 1e-3 < stored < 2e-2 and abs(dev - stored) < 0.05 * stored, (name, dev, stored)      # (the stored pred is rounded to bf16 once more)


def test_header_is_parsed_and_built():
    from painter_amd import _lib, build
    from tests.guard_bands import abi_symbols
    assert abi_symbols(open(HEADER).read()) == SYMBOLS
    assert HEADER in [os.path.abspath(p) for p in _lib.MORE_HEADERS] and HEADER in build.headers()
    assert not SYMBOLS & set(_lib.parse_header())                  # additions only: include/painter_hip.h does not know them
    protos = _lib.parse_header(HEADER)
    assert set(protos) == SYMBOLS and len(protos["pa_attn_any_fwd"][1]) == 15 and len(protos["pa_relpos_resize"][1]) == 9


def test_route_predicate_restates_pa_attn_fwd_refusal():
    from painter_amd import ops_anysize
    assert ops_anysize.attn_fwd_takes(128, 16, 8) and ops_anysize.attn_fwd_takes(1568, 56, 28)
    for Hp, Wp in ((70, 35), (10, 5), (6, 3), (12, 6), (2, 1), (3, 11)):
        assert not ops_anysize.attn_fwd_takes(Hp * Wp, Hp, Wp)
