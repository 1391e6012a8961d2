"""COCO RLE without a GPU: the vectors of the format against the host statement (tests/painter_rle_host.py), the statement against
itself, and the C ABI of include/painter_rle.h as far as the host reaches it."""
import os

import numpy as np
import pytest

from tests import painter_rle_cases as C
from tests import painter_rle_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLE_HEADER = os.path.join(ROOT, "include", "painter_rle.h")
SYMBOLS = {"pa_rle_encode", "pa_rle_encode_workspace_bytes", "pa_rle_decode", "pa_rle_decode_workspace_bytes"}


@pytest.mark.parametrize("name,mask,counts,string", C.table(), ids=[t[0] for t in C.table()])
def test_the_vectors_of_the_format(name, mask, counts, string):
    fast = H.encode_fast(mask)
    assert fast == counts
    if mask.size <= 4096:
        assert H.encode(mask) == counts                        # the per-pixel loop is the definition
    assert H.to_string(counts) == string.encode("ascii")
    assert H.from_string(string) == counts and H.values(string)[1] == 0 and H.check(string, *mask.shape) == 0
    assert np.array_equal(H.decode(counts, *mask.shape), mask)
    assert H.area(counts) == int(mask.sum())


def test_the_checkerboard_joins_its_columns():
    cnts = H.encode_fast(C.checkerboard(480, 640))
    assert len(cnts) == 306561 and set(cnts) == {1, 2} and cnts.count(2) == 639          # where two columns join, a run of 2
    small = C.checkerboard(48, 64)
    assert H.encode(small) == H.encode_fast(small) and len(H.encode(small)) == 48 * 64 - 63


@pytest.mark.parametrize("name,mask", C.cases(), ids=[c[0] for c in C.cases()])
def test_statement_round_trip_and_the_vectorised_form(name, mask):
    h, w = mask.shape
    cnts = H.encode_fast(mask)
    if mask.size <= 8192:
        assert H.encode(mask) == cnts
    assert cnts[0] == 0 if mask[0, 0] else cnts[0] > 0
    assert all(c > 0 for c in cnts[1:]) and sum(cnts) == h * w
    s = H.to_string(cnts)
    assert len(s) <= 7 * len(cnts) and all(48 <= b <= 111 for b in s)
    assert H.from_string(s) == cnts and H.from_string(s.decode("ascii")) == cnts
    assert np.array_equal(H.decode(cnts, h, w), mask)
    assert H.area(cnts) == int(mask.sum())
    ys, xs = np.nonzero(mask)
    box = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if len(ys) else [0, 0, 0, 0]
    assert H.to_bbox(cnts, h, w) == box
    assert np.array_equal(H.unpack_bits(H.pack_bits(mask[None]), h, w)[0], mask)


def test_batch_masks_round_trip():
    masks = C.batch()
    runs = [len(H.encode_fast(m)) for m in masks]
    assert min(runs) == 1 and max(runs) > 100 * sorted(runs)[len(runs) // 3]          # very different run counts
    for m in masks[:8]:
        assert H.encode(m) == H.encode_fast(m)


def test_malformed_strings_are_refused_by_the_statement():
    h, w = 9, 7
    flags = set()
    for name, counts, flag in C.malformed(h, w):
        assert H.check(counts, h, w) == flag, name
        flags.add(flag)
    assert flags == {1, 2, 3, 4, 7}
    assert H.check(H.to_string([h * w - 3, 3]), h, w) == 0
    assert H.check(H.to_string([10, 0, 0, h * w - 10]), h, w) == 0          # zero counts inside are legal


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd import _lib
    from painter_amd._lib import lib, parse_header
    from tests.guard_bands import abi_symbols
    protos = parse_header(RLE_HEADER)
    assert set(protos) == SYMBOLS == abi_symbols(open(RLE_HEADER).read())
    for name in SYMBOLS:
        assert getattr(lib, name) is not None                  # the built library exports them, the binding resolves them
    assert RLE_HEADER in [os.path.abspath(p) for p in _lib.MORE_HEADERS]
    assert len(protos["pa_rle_encode"][1]) == 11 and len(protos["pa_rle_decode"][1]) == 12
    main = parse_header()
    assert len(main) == 134 and not set(main) & SYMBOLS          # painter_hip.h's own set is unchanged
    assert getattr(lib, "pa_inst_decode") is not None and lib.pa_abi_version() == 9          # `lib` resolves both headers


def test_record_layouts_match_the_header():
    from painter_amd import painter_engine as E
    assert E.RLE_HEADER.itemsize == 32 and E.RLE_RECORD.itemsize == 40
    assert E.RLE_RECORD.fields["runs"][1] == 16 and E.RLE_RECORD.fields["bbox"][1] == 24


def test_size_helpers():
    from painter_amd._lib import lib
    up16 = lambda x: -(-x // 16) * 16
    for h, w, n in ((1, 1, 1), (480, 640, 100), (37, 53, 7), (3, 2500, 65535)):
        c = n * w
        want = 2 * up16(16 * c) + up16(8 * c) + 2 * up16(4 * c) + 2 * up16(8 * n) + up16(4 * n)
        assert lib.pa_rle_encode_workspace_bytes(h, w, n) == want, (h, w, n)
        assert lib.pa_rle_decode_workspace_bytes(n, h, w, 1000) == 8000 + up16(4 * n)
    assert lib.pa_rle_decode_workspace_bytes(3, 5, 7, 0) == 16
    for bad in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -3, 1), (5, 5, 0), (5, 5, -1), (5, 5, 65536), (46341, 46341, 1), (1 << 16, 1 << 15, 1),
                (2**31 - 1, 2, 1)):
        assert lib.pa_rle_encode_workspace_bytes(*bad) == -1, bad
        assert lib.pa_rle_decode_workspace_bytes(bad[2], bad[0], bad[1], 10) == -1, bad
    assert lib.pa_rle_encode_workspace_bytes(1, 2**31 - 1, 1) > 0 and lib.pa_rle_encode_workspace_bytes(46340, 46340, 1) > 0
    assert lib.pa_rle_decode_workspace_bytes(1, 5, 5, -1) == -1


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """hipErrorInvalidValue (1): no pointer is touched, so this needs no GPU."""
    from painter_amd._lib import lib
    a = 256
    ok = dict(masks=a, count=a, h=5, w=7, n=3, ws=a, cap=10, header=a, records=a, pool=a)
    enc = lambda **kw: lib.pa_rle_encode(*dict(ok, **kw).values(), None)
    for bad in (dict(masks=None), dict(count=None), dict(ws=None), dict(header=None), dict(records=None), dict(pool=None), dict(h=0), dict(w=0),
                dict(n=0), dict(n=65536), dict(h=65536, w=32768), dict(cap=-1), dict(ws=a + 8), dict(header=a + 4), dict(records=a + 4),
                dict(masks=a + 2)):
        assert enc(**bad) == 1, bad
    ok = dict(pool=a, compressed=1, spans=a, n=3, h=5, w=7, pool_len=10, run_cap=10, ws=a, bits=a, flags=a)
    dec = lambda **kw: lib.pa_rle_decode(*dict(ok, **kw).values(), None)
    for bad in (dict(pool=None), dict(spans=None), dict(ws=None), dict(bits=None), dict(flags=None), dict(n=0), dict(n=65536), dict(h=0),
                dict(w=-1), dict(h=65536, w=32768), dict(pool_len=-1), dict(run_cap=-1), dict(ws=a + 8), dict(spans=a + 4), dict(bits=a + 2),
                dict(flags=a + 1), dict(pool=a + 1, compressed=0)):
        assert dec(**bad) == 1, bad
