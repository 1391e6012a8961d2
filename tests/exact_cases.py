"""Operands for which attention and the decoder's 3x3 convolution have an EXACT answer, built on the CPU in plain torch.

Attention: softmax as an exact gather.  One key's logit exceeds every other key's by at least 150 in every query row, so exp() of every
other term is zero in fp32 (exp(-150) = 7e-66) and the row's softmax is one-hot in any correct implementation: out[q] is the V row of
key t(q) bit for bit, dV is an integer scatter-add of dO rows, and dS = P o (dP - Delta) -- hence dQ, dK and the rel-pos table gradient --
is exactly zero.  Every operand is an integer that bf16 holds exactly and scale is a power of two, so every logit, lse, dP and Delta is an
integer fp32 holds exactly.  V is position-coded: a wrong output row names the key, head and sample that arrived in its place.

Attention with tied winners (tie_case, further down): 1, 2 or 4 keys tie at logit exactly 0 in every row, so P = 1/n and dS, dQ, dK and the
table gradients are non-zero dyadic rationals; the expectation is the fp64 autograd of attn_reference.

Attention on any token grid (ANY_ROUTES, further down): the same cases on ragged grids for the forward of csrc/attn_any.hip, one more kind
(below_zero: every logit <= -150) and any_algebra, an fp64 forward over that kernel's own key walk that also returns what named wrong
kernels would.  ANY_BWD_ROUTES, behind it: the backward of csrc/attn_any_bwd.hip on tie cases for ragged L (tie_loners) and on the gather
kinds, with any_bwd_algebra, the fp64 backward over that kernel's key walk and its named wrong kernels.

Convolution (64 channels, 3x3, padding 1): small integers, int64 references from nine shifted matmuls.

The parametrisations of tests/test_attention_exact_gpu.py, tests/test_attention_ties_gpu.py, tests/test_attention_any_exact_gpu.py,
tests/test_attention_any_bwd_exact_gpu.py and tests/test_conv3x3_exact_gpu.py live here, so that
tests/test_exact_cases_cpu.py can assert, without a GPU, the conditions those tests rest on -- for every one of them."""
import functools
from dataclasses import dataclass

import torch
from torch.overrides import TorchFunctionMode

from tests.test_kernels_gpu import attn_reference
from tests.test_vit_huge_kernels_gpu import _conv3x3, _conv3x3_dgrad, _conv3x3_wgrad, _tail

SCALE = 0.125                 # head_dim 64 AND head_dim 80: a power of two keeps every logit an integer (80 ** -0.5 would not)
MIN_MARGIN = 150.0
AMPLITUDES = (6, 8, 10)       # a_q, cycling over q: neighbouring rows differ in lse and Delta
TARGET_MAPS = ("identity", "reversal", "permutation", "all_to_last", "all_to_first")
ATTN_KINDS = TARGET_MAPS + ("bias_rank",)


# ------------------------------------------------------------------------------------------------ attention
@dataclass(frozen=True)
class AttnCase:
    kind: str
    B: int
    H: int
    Hp: int
    Wp: int
    hd: int
    qkv: torch.Tensor         # f32 [B*L, 3*H*hd], integer-valued, the layout ops.attn_fwd takes
    rel_h: torch.Tensor       # f32 [2Hp-1, hd]
    rel_w: torch.Tensor       # f32 [2Wp-1, hd]
    dout: torch.Tensor        # f32 [B*L, H*hd], entries in {-1, 0, 1}
    scale: float = SCALE

    @property
    def L(self):
        return self.Hp * self.Wp


def _sign(c):
    """+1 / -1 by the parity of the number of set bits of the channel index: no shift or swap of channels maps the pattern onto itself."""
    return 1 - 2 * (bin(c).count("1") & 1)


def position_coded_v(B, H, Hp, Wp, hd):
    """-> f32 [B, L, H, hd]: blocks of 16 channels hold kh + 1, kw + 1, head + 1, sample + 1 (and for head_dim 80 1 + key mod 64), each
    times _sign(channel).  Every magnitude is in 1 .. 64."""
    assert hd % 16 == 0 and hd >= 64 and Hp <= 63 and Wp <= 63 and H <= 63 and B <= 63
    L = Hp * Wp
    k = torch.arange(L)
    fields = [(k // Wp + 1)[None, :, None].expand(B, L, H), (k % Wp + 1)[None, :, None].expand(B, L, H),
              (torch.arange(H) + 1)[None, None, :].expand(B, L, H), (torch.arange(B) + 1)[:, None, None].expand(B, L, H),
              (k % 64 + 1)[None, :, None].expand(B, L, H)]
    v = torch.stack([fields[c // 16] * _sign(c) for c in range(hd)], -1)
    return v.float()


def decode_v_row(row):
    """What a position-coded V row says about itself -> dict(kh, kw, head, sample), or None when `row` is no V row (a mixture, zeros)."""
    row = row.double().cpu()
    vals = []
    for blk in range(4):
        seg = row[blk * 16:(blk + 1) * 16] * torch.tensor([_sign(c) for c in range(blk * 16, (blk + 1) * 16)], dtype=torch.float64)
        if float(seg.min()) != float(seg.max()) or float(seg[0]) < 1 or float(seg[0]) != int(seg[0]):
            return None
        vals.append(int(seg[0]) - 1)
    return dict(kh=vals[0], kw=vals[1], head=vals[2], sample=vals[3])


def _ternary(shape, g):
    return (torch.randint(0, 3, shape, generator=g) - 1).float()


def _pack_qkv(q, k, v):
    """[B, H, L, hd] x 3 -> [B*L, 3*H*hd] (qkv.reshape(B, L, 3, H, hd))."""
    B, H, L, hd = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * hd).contiguous()


def _target_map(kind, B, H, L, g):
    q = torch.arange(L)
    if kind == "identity":
        t = q
    elif kind == "reversal":
        t = L - 1 - q
    elif kind == "all_to_last":
        t = torch.full((L,), L - 1)
    elif kind == "all_to_first":
        t = torch.zeros(L, dtype=torch.int64)
    elif kind == "permutation":
        return torch.stack([torch.randperm(L, generator=g) for _ in range(B * H)]).reshape(B, H, L)
    else:
        raise ValueError(kind)
    return t[None, None, :].expand(B, H, L).contiguous()


def content_case(B, H, Hp, Wp, hd, target_map, seed):
    """The content term alone decides: key k carries a random sign code c_k in {-8, +8}^hd (drawn per sample and head), query q asks for
    key t(q) with a_q * sign(c_t(q)).  Target logit 0.125 * hd * 8 * a_q >= 384; every other key's is a sum of hd random signs, a_q * 8 *
    0.125 each.  Rel-pos tables are zero."""
    g = torch.Generator().manual_seed(seed)
    L = Hp * Wp
    code = (torch.randint(0, 2, (B, H, L, hd), generator=g) * 16 - 8).float()
    t = _target_map(target_map, B, H, L, g)
    amp = torch.tensor(AMPLITUDES, dtype=torch.float32)[torch.arange(L) % len(AMPLITUDES)]
    q = torch.gather(code, 2, t[..., None].expand(B, H, L, hd)) / 8 * amp[None, None, :, None]
    v = position_coded_v(B, H, Hp, Wp, hd).permute(0, 2, 1, 3)
    dout = _ternary((B * L, H * hd), g)
    return AttnCase(target_map, B, H, Hp, Wp, hd, _pack_qkv(q, code, v), torch.zeros(2 * Hp - 1, hd), torch.zeros(2 * Wp - 1, hd), dout)


def bias_rank_case(B, H, Hp, Wp, hd, seed):
    """The bias alone decides, no row excluded: K = 0; q = +8 in channels 0..31; rel_pos_h[j][0..31] = w_h(j), rel_pos_w[j][0..31] = w_w(j),
    seeded permutations of 0 .. 2Hp-2 and 0 .. 2Wp-2.  logit(q, k) = 256 * (w_h(qh-kh+Hp-1) + w_w(qw-kw+Wp-1)) (the bias term takes the
    unscaled q): every query has one best reachable row offset and one best column offset, and the margin is 256 times the smaller of the
    two gaps to the second best.  Logits reach 4e4: only the subtraction of the running maximum keeps exp() finite."""
    g = torch.Generator().manual_seed(seed)
    L = Hp * Wp
    q = torch.zeros(B, H, L, hd)
    q[..., :32] = 8.0
    rel_h, rel_w = torch.zeros(2 * Hp - 1, hd), torch.zeros(2 * Wp - 1, hd)
    rel_h[:, :32] = torch.randperm(2 * Hp - 1, generator=g).float()[:, None]
    rel_w[:, :32] = torch.randperm(2 * Wp - 1, generator=g).float()[:, None]
    v = position_coded_v(B, H, Hp, Wp, hd).permute(0, 2, 1, 3)
    dout = _ternary((B * L, H * hd), g)
    return AttnCase("bias_rank", B, H, Hp, Wp, hd, _pack_qkv(q, torch.zeros(B, H, L, hd), v), rel_h, rel_w, dout)


class _CaptureLogits(TorchFunctionMode):
    """Keeps the tensor attn_reference hands to torch.logsumexp: the fp64 logits as that function builds them, without restating it.
    This rests on attn_reference calling torch.logsumexp on the complete logits exactly once; reference() asserts the call count, the dtype
    and the [B*H, L, L] shape, so a rewrite of attn_reference that breaks it fails there and not silently."""
    logits = None
    calls = 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is torch.logsumexp:
            self.logits = args[0]
            self.calls += 1
        return func(*args, **(kwargs or {}))


@dataclass(frozen=True)
class AttnExpect:
    target: torch.Tensor      # int64 [B, H, L]: argmax of the fp64 logits
    margin: torch.Tensor      # f64 [B, H, L]: top-1 minus top-2
    top: torch.Tensor         # f64 [B, H, L]: the winning logit (= lse wherever the margin holds)
    lse: torch.Tensor         # f64 [B*H, L]: attn_reference's own
    out: torch.Tensor         # f32 [B*L, H*hd]: the gathered V rows
    dv: torch.Tensor          # int64 [B*L, H*hd]: scatter-add of dO rows
    runner_up: torch.Tensor   # int64 [B, H, L]


def reference(case):
    """-> AttnExpect.  dq, dk and the rel-pos table gradient are expected to be exactly zero (nothing to return)."""
    B, H, L, hd = case.B, case.H, case.L, case.hd
    with _CaptureLogits() as cap:
        _, lse = attn_reference(case.qkv, case.rel_h, case.rel_w, B, L, H, case.Hp, case.Wp, case.scale)
    logits = cap.logits
    assert cap.calls == 1 and logits is not None and logits.dtype == torch.float64 and logits.shape == (B * H, L, L)
    if L == 1:                                      # a single key: no runner-up, the margin is infinite
        top2, idx2 = torch.cat([logits, torch.full_like(logits, float("-inf"))], -1), torch.zeros(B * H, 1, 2, dtype=torch.int64)
    else:
        top2, idx2 = logits.topk(2, dim=-1)
    target = idx2[..., 0].reshape(B, H, L)
    v = case.qkv.reshape(B, L, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3)                    # [B, H, L, hd]
    out = torch.gather(v, 2, target[..., None].expand(B, H, L, hd)).permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous()
    do = case.dout.reshape(B, L, H, hd).permute(0, 2, 1, 3).to(torch.int64)
    dv = torch.zeros(B, H, L, hd, dtype=torch.int64).scatter_add_(2, target[..., None].expand(B, H, L, hd), do)
    return AttnExpect(target, (top2[..., 0] - top2[..., 1]).reshape(B, H, L), top2[..., 0].reshape(B, H, L), lse, out,
                      dv.permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous(), idx2[..., 1].reshape(B, H, L))


def dv_fp32_bound(case, exp):
    """-> f64 [B*L, H*hd]: how far the fp32 build's dV may be from the integer scatter-add.  The backward kernels rebuild P from an lse kept
    in natural-log units, so at the winner P = 1 +- |logit_q| * 2^-22 (tests/test_attention_exact_gpu.py); dV[k] = sum_q P_q dO_q then errs
    by at most sum_q |dO_q| |logit_q| 2^-22, plus A[k] N[k] 2^-24 for the fp32 accumulation of N[k] terms whose magnitudes sum to A[k]."""
    B, H, L, hd = case.B, case.H, case.L, case.hd
    idx = exp.target[..., None].expand(B, H, L, hd)
    absdo = case.dout.reshape(B, L, H, hd).permute(0, 2, 1, 3).abs().double()
    add = lambda src: torch.zeros(B, H, L, hd, dtype=torch.float64).scatter_add_(2, idx, src)
    A, N, Atop = add(absdo), add(torch.ones_like(absdo)), add(absdo * exp.top.abs()[..., None])
    return (Atop * 2.0 ** -22 + A * N * 2.0 ** -24).permute(0, 2, 1, 3).reshape(B * L, H * hd)


@functools.lru_cache(maxsize=None)
def attn_case(kind, B, H, Hp, Wp, hd):
    """The case of one (kind, shape) and its reference, built once per process and shared by every route that runs it: read-only."""
    seed = 1000 * Hp + 10 * Wp + hd + ATTN_KINDS.index(kind)
    case = bias_rank_case(B, H, Hp, Wp, hd, seed) if kind == "bias_rank" else content_case(B, H, Hp, Wp, hd, kind, seed)
    return case, reference(case)


# route -> (dtype name, head_dim, generation to set, kernel family the launch counters must show (0 generic, 1 generation 2, 2 generation 3),
#           [(B, H, Hp, Wp)])
_G3 = [(2, 2, 8, 28), (2, 2, 16, 28)]
_G2_SHAPE = [(2, 2, 8, 12), (2, 2, 8, 20), (2, 2, 16, 16), (2, 2, 8, 24)]
_GENERIC = [(2, 2, 8, 4), (2, 2, 16, 8), (2, 2, 4, 32)]
_HD80_G2, _HD80_WP32, _HD80_GENERIC = [(2, 2, 8, 12), (2, 2, 16, 28)], [(2, 2, 4, 32)], [(2, 2, 8, 4)]
FULL_GRID = (1, 1, 56, 28)                                     # 13 workgroups per head, the 13th with one live wave of four
FULL_GRID_KINDS = ("reversal", "all_to_last", "all_to_first", "bias_rank")
ATTN_ROUTES = {
    "bf16_hd64_gen3": ("bf16", 64, 0, 2, _G3),
    "bf16_hd64_gen3_full": ("bf16", 64, 0, 2, [FULL_GRID]),
    "bf16_hd64_gen2_forced": ("bf16", 64, 2, 1, _G3),
    "bf16_hd64_gen2": ("bf16", 64, 0, 1, _G2_SHAPE),
    "bf16_hd64_generic": ("bf16", 64, 0, 0, _GENERIC),
    "bf16_hd80_gen2": ("bf16", 80, 0, 1, _HD80_G2),
    "bf16_hd80_gen2_wp32": ("bf16", 80, 0, 1, _HD80_WP32),
    "bf16_hd80_generic": ("bf16", 80, 0, 0, _HD80_GENERIC),
    "fp32_hd64": ("fp32", 64, 0, 0, _G3 + _G2_SHAPE + _GENERIC),
    "fp32_hd64_full": ("fp32", 64, 0, 0, [FULL_GRID]),
    "fp32_hd80": ("fp32", 80, 0, 0, _HD80_G2 + _HD80_WP32 + _HD80_GENERIC),
}
# the shortest grids the generation-2 kernels run through the C ABI (L = 64 and L = 96; attn2_ok alone would admit (2, 16), but pa_attn_fwd and
# pa_attn_bwd refuse Hp % 4 != 0): new to the suite, kept apart and run after the rest
SHORT_GRIDS = [(2, 2, 4, 16), (2, 2, 4, 24)]
SHORT_ROUTES = {"bf16_hd64_gen2_short": ("bf16", 64, 0, 1, SHORT_GRIDS), "bf16_hd80_gen2_short": ("bf16", 80, 0, 1, SHORT_GRIDS)}
PREP_LAUNCH_GRID = (2, 2, 16, 28)                              # the generation-3 backward with prep="launch"
# ... on every kind there, and bias_rank once more on the full grid: the one case in which P's bf16 bits at the winner are not those of 1
PREP_LAUNCH_CASES = [(kind, PREP_LAUNCH_GRID) for kind in ATTN_KINDS] + [("bias_rank", FULL_GRID)]


def route_params(routes):
    """-> [(route, kind, B, H, Hp, Wp)] in the order the GPU tests run them."""
    out = []
    for route, (_, _, _, _, grids) in routes.items():
        for grid in grids:
            for kind in (FULL_GRID_KINDS if grid == FULL_GRID else ATTN_KINDS):
                out.append((route, kind) + grid)
    return out


def attn_shapes():
    """Every distinct (kind, B, H, Hp, Wp, hd) the GPU tests build."""
    seen = []
    for routes in (ATTN_ROUTES, SHORT_ROUTES):
        for route, kind, B, H, Hp, Wp in route_params(routes):
            key = (kind, B, H, Hp, Wp, routes[route][1])
            if key not in seen:
                seen.append(key)
    return seen


# ------------------------------------------------------------------------------------------------ attention: tied winners
# Several keys tie exactly for first place, every other key is >= 150 below: P is exactly 1/n on the n winners (n in {1, 2, 4}) and 0
# elsewhere, so dS = P o (dP - Delta) is a NON-ZERO dyadic rational of a few bits and so are dQ, dK, dV and both table gradients: the fp64
# autograd of attn_reference is the exact answer (tests/test_attention_ties_gpu.py; conditions in tests/test_exact_cases_cpu.py).
TIE_AMPLITUDES = (12, 14, 16)                       # a_q, cycling over q
TIE_WINNERS = (4, 2, 1)                             # winners of a row: index (r % 3 + r % 5) % 3 with r = L - 1 - q -- the last row has four
TIE_PLACEMENTS = ("near", "quarter", "mirror")
TIE_KINDS = tuple("tie_" + p for p in TIE_PLACEMENTS) + tuple("tie_%s_sparse" % p for p in TIE_PLACEMENTS)     # dO dense | ~6 % non-zero


def tie_kinds(grid, hd):
    """A dense dO on the head-dim-64 grids below the full one; the sparse one everywhere.  Where V's magnitudes (key rows up to 56, the
    fifth field of head dim 80 up to 64) meet a dense dO, some dS need a ninth significant bit and bf16 no longer holds them (asserted
    case by case in tests/test_exact_cases_cpu.py for what IS built); the full grid runs once per placement in any case."""
    return TIE_KINDS if hd == 64 and grid != FULL_GRID else TIE_KINDS[3:]

TIE_SPARSE_DENSITY = 1.0 / 16


def tie_layout(hd):
    """-> (active, S1, S2, shift channels, offset channel): channel index lists.  The hd - 20 `active` channels carry the group's code, S1
    and S2 (8 channels each) the two flip sets, the three shift channels (one per number of code channels a query keeps) bring every
    winning logit to 0, and the offset channel codes the table row in both tables."""
    na = hd - 20
    # interleave the roles over the head dim, so that no 16-channel k-step holds one role alone
    order = sorted(range(hd), key=lambda c: (c * 37) % hd)
    return order[:na], order[na:na + 8], order[na + 8:na + 16], order[na + 16:na + 19], order[na + 19]


def tie_loners(L, Wp):
    """-> the L % 4 keys of a ragged grid that stay outside every group of four (ascending; none where L % 4 == 0).  A loner has a group
    code of its own, so a row that asks for it has ONE winner.  Loners are taken from the interior: outside the first and the last key row
    and the first and the last 32-key tile where the grid has such keys; else outside both key rows and the last tile; else anywhere but
    key 0 and the last tile -- never in the last tile, whose keys must all carry a non-zero dS, unless the grid has one tile only
    (L <= 32), and never key 0 or L - 1, which the `near` and `mirror` placements pair up.  Wish i is key L // 2 - 3 - 5 i; the nearest
    free key of the tier is taken."""
    n, last = L % 4, (L - 1) // 32 * 32
    if n == 0:
        return []
    keys = range(L)
    tiers = ([k for k in keys if Wp <= k < L - Wp and 32 <= k < last], [k for k in keys if Wp <= k < L - Wp and k < last],
             [k for k in keys if 0 < k < min(last, L - 1)], [k for k in keys if Wp <= k < L - Wp and L <= 32],
             [k for k in keys if 0 < k < L - 1 and L <= 32])
    room = next((t for t in tiers if len(t) >= n), None)
    if room is None:
        raise ValueError("a grid of %d keys has no room for %d loners: use the gather kinds there" % (L, n))
    out = []
    for i in range(n):
        out.append(min((k for k in room if k not in out), key=lambda k: (abs(k - (L // 2 - 3 - 5 * i)), k)))
    return sorted(out)


def tie_members(placement, L, Wp=None):
    """-> int64 [L // 4, 4]: the keys of each group; member m and member m ^ 2 are the pair a two-way tie leaves.  On a ragged grid
    (L % 4 != 0; Wp is needed then) the groups are placed over the L - L % 4 keys that are no loners, in key order."""
    if L % 4:
        loners = tie_loners(L, Wp)
        rest = torch.tensor([k for k in range(L) if k not in loners])
        return rest[tie_members(placement, L - L % 4)]
    g = torch.arange(L // 4)
    if placement == "near":                         # neighbours, two keys off the multiples of four: mostly one 32-key tile and one key row,
        m = [(4 * g + 2 + i) % L for i in range(4)]  # some across a row or tile boundary, and one group is keys L - 2, L - 1, 0, 1
    elif placement == "quarter":                    # a quarter of the grid apart: other tiles, key rows and dKV workgroups
        m = [g, g + L // 4, g + L // 2, g + 3 * (L // 4)]
    elif placement == "mirror":                     # k and L - 1 - k pair up: the first and last key rows and the last tile take part
        m = [g, L // 2 - 1 - g, L - 1 - g, L // 2 + g]
    else:
        raise ValueError(placement)
    return torch.stack(m, 1)


def tie_winner_count(L):
    r = L - 1 - torch.arange(L)
    return torch.tensor(TIE_WINNERS)[(r % 3 + r % 5) % 3]


def tie_case(B, H, Hp, Wp, hd, placement, sparse, seed):
    """Keys come in groups of four that share a random code in {-8, +8} on the active channels and differ by the sign of one or both
    flip sets; query q asks for the group of key t(q) (a permutation per (sample, head)) with a_q * sign(code), and is zero on both flip sets
    (four winners), on S2 only (two: t and its partner) or on neither (one).  The nearest loser differs on a flip set the query kept: 16 a_q
    >= 192 below.  Shift channels: a query keeps n_c = hd - 20, hd - 12 or hd - 4 code channels; the shift channel of that count holds
    K = -8 n_c in every key and q = a_q there (zero in the other two), so every logit of the row moves down by the row's top logit a_q n_c
    and the winners sit at exactly 0 -- as an integer sum inside the Q.K^T product.  (NOT through the tables: a constant table entry
    times q would do the same in exact arithmetic, but the generation-2 kernels keep q . rel_pos_h times log2 e as bf16 -- attn2.hip:61 --
    and the generic ones as a rounded fp32 -- attn_common.h:151 --, which un-ties nothing but moves lse by up to 2.  So q . R is exactly
    zero in every tie case: q is zero wherever a table is not.)  Offset channel: q = K = 0, rel_pos_h[j] = rel_pos_w[j] = j + 1 -- no
    logit changes, and dQ there is sum_k dS[q, k] (Rh[qh - kh] + Rw[qw - kw]), which names the offsets the kernel used.  Every q entry is 0
    or +-a_q, three significant bits: that keeps the fp32 sums of the table gradients exact.
    Ragged grids (L % 4 != 0): the L % 4 keys of tie_loners each form a group of their own and the groups of four are placed over the
    other keys; with L % 4 == 0 the draws, and so the case, are what they were before ragged grids were admitted."""
    g = torch.Generator().manual_seed(seed)
    L = Hp * Wp
    active, s1, s2, shift, offset = tie_layout(hd)
    members, loners = tie_members(placement, L, Wp), tie_loners(L, Wp)
    ng = L // 4 + len(loners)                       # groups of four, then one group per loner (member 0 of its own code)
    assert L // 4 >= 4
    group_of, member_of = torch.empty(L, dtype=torch.int64), torch.zeros(L, dtype=torch.int64)
    group_of[members] = torch.arange(L // 4)[:, None].expand(L // 4, 4)
    member_of[members] = torch.arange(4)[None, :].expand(L // 4, 4)
    group_of[loners] = L // 4 + torch.arange(len(loners))
    while True:                                     # group codes at least 8 active channels apart (>= 192 below, as the flip sets are)
        gcode = (torch.randint(0, 2, (B, H, ng, hd), generator=g) * 16 - 8).float()
        a = gcode[..., active] / 8
        if int(((len(active) - a @ a.transpose(-1, -2)) / 2 + 99 * torch.eye(ng)).min()) >= 8:
            break
    k = gcode[:, :, group_of]                       # [B, H, L, hd]
    k[..., s1] *= (1 - 2 * (member_of & 1)).float()[None, None, :, None]
    k[..., s2] *= (1 - 2 * (member_of >> 1)).float()[None, None, :, None]
    k[..., shift] = -8.0 * torch.tensor([len(active), len(active) + 8, len(active) + 16])       # for rows of 4, 2, 1 winners
    k[..., offset] = 0
    t = _target_map("permutation", B, H, L, g)
    amp = torch.tensor(TIE_AMPLITUDES, dtype=torch.float32)[torch.arange(L) % len(TIE_AMPLITUDES)]
    n = tie_winner_count(L)
    if L % 4:
        # dK = scale * dS q with dS a multiple of 1/16 in a four-winner row whose V rows sum to an odd number (groups placed over a ragged
        # grid do): amplitude 14 would make dK a multiple of 1/64 there, the expectations are to stay multiples of 1/32
        amp = torch.where((n == 4) & (amp == 14), torch.tensor(16.0), amp)
    # a row that asks for a loner has one winner whatever n says: hand every loner to a row that is to have one winner anyway (the first
    # such rows whose own target is no loner), so that the rows keep the winner counts of tie_winner_count -- the last row its four
    for bh in range(B * H if loners else 0):
        tb = t[bh // H, bh % H]
        is_loner = torch.zeros(L, dtype=torch.bool)
        is_loner[loners] = True
        free = [q for q in range(L) if int(n[q]) == 1 and not bool(is_loner[tb[q]])]
        for q in [q for q in range(L) if int(n[q]) != 1 and bool(is_loner[tb[q]])]:
            q2 = free.pop(0)
            tb[q], tb[q2] = int(tb[q2]), int(tb[q])
    q = torch.gather(k, 2, t[..., None].expand(B, H, L, hd)) / 8 * amp[None, None, :, None]
    q[:, :, :, s1] *= (n < 4).float()[None, None, :, None]
    q[:, :, :, s2] *= (n < 2).float()[None, None, :, None]
    q[..., shift] = (amp[:, None] * (torch.tensor(TIE_WINNERS)[None, :] == n[:, None]).float())[None, None]
    q[..., offset] = 0
    rel_h, rel_w = torch.zeros(2 * Hp - 1, hd), torch.zeros(2 * Wp - 1, hd)
    rel_h[:, offset], rel_w[:, offset] = torch.arange(1, 2 * Hp).float(), torch.arange(1, 2 * Wp).float()
    v = position_coded_v(B, H, Hp, Wp, hd).permute(0, 2, 1, 3)
    dout = _ternary((B * L, H * hd), g)
    if sparse:
        dout = dout * (torch.rand((B * L, H * hd), generator=g) < 1.5 * TIE_SPARSE_DENSITY).float()     # 2/3 * 3/32 = 1/16 non-zero
    return AttnCase("tie_" + placement + ("_sparse" if sparse else ""), B, H, Hp, Wp, hd, _pack_qkv(q, k, v), rel_h, rel_w, dout)


def tie_algebra(case, fault=None):
    """Softmax attention forward and backward written out by hand in fp64 -> dict(logits, P, dP, delta, dS, dG_h, dG_w, out, lse, dq, dk,
    dv, drh, drw), every matrix [B*H, L, .], the data gradients [B*L, H*hd], the tables [2Hp-1 | 2Wp-1, hd].  Without `fault` this is the
    expectation once more (tie_reference asserts it against autograd); with one it is what a named wrong BACKWARD would return from the
    right forward:
      delta_next_row     Delta of query q + 1 (of the head's first query for its last)
      kh_class_phase     the rel_pos_h row of the keys of one tile phase -- the 32-key tiles whose number is that of the last tile mod 7 --
                         taken one too high (clamped), in dQ and in the table gradient
      last_key_row       the keys of the last key row left out of the rel_pos_h gradient
      l_previous_row     P divided by the l of query q - 1 instead of its own
      dg_column_dropped  the middle column of the per-query bias gradient (rel_pos_h row Hp - 1: key row = query row) left out of the
                         table-gradient contraction
    On a tie case P is set to exactly 1 / n on the winners (fp64's exp(-log n) is 1e-16 off, and every loser's exp() is below 1e-65)."""
    B, H, L, hd, Hp, Wp, s = case.B, case.H, case.L, case.hd, case.Hp, case.Wp, case.scale
    q, k, v = case.qkv.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, B * H, L, hd).unbind(0)
    do = case.dout.double().reshape(B, L, H, hd).permute(0, 2, 1, 3).reshape(B * H, L, hd)
    Rh, Rw = case.rel_h.double(), case.rel_w.double()
    key = torch.arange(L)
    ih = (key[:, None] // Wp - key[None, :] // Wp + Hp - 1)                      # [L, L]: table row of (query, key)
    iw = (key[:, None] % Wp - key[None, :] % Wp + Wp - 1)
    Gh, Gw = q @ Rh.t(), q @ Rw.t()                                               # the per-query bias tables [B*H, L, 2Hp-1 | 2Wp-1]
    BH = B * H
    logits = s * q @ k.transpose(1, 2) + torch.gather(Gh, 2, ih.expand(BH, L, L)) + torch.gather(Gw, 2, iw.expand(BH, L, L))
    lse = torch.logsumexp(logits, -1)
    P = torch.exp(logits - lse[..., None])
    if case.kind.startswith("tie"):
        P = (logits == 0).double() / (logits == 0).sum(-1, keepdim=True)
    out = P @ v
    dP = do @ v.transpose(1, 2)
    delta = (out * do).sum(-1)
    Pb, delta_b, ih_b = P, delta, ih
    if fault == "delta_next_row":
        delta_b = delta.roll(-1, 1)
    elif fault == "l_previous_row":
        Pb = P * torch.exp(lse - lse.roll(1, 1))[..., None]
    elif fault == "kh_class_phase":
        ih_b = torch.where(((key // 32) % 7 == ((L - 1) // 32) % 7)[None, :], (ih + 1).clamp_max(2 * Hp - 2), ih)
    elif fault not in (None, "last_key_row", "dg_column_dropped"):
        raise ValueError(fault)
    dS = Pb * (dP - delta_b[..., None])
    dS_h = dS * (key // Wp != Hp - 1)[None, None, :] if fault == "last_key_row" else dS
    dG_hq = torch.zeros(BH, L, 2 * Hp - 1, dtype=torch.float64).scatter_add_(2, ih_b.expand(BH, L, L), dS)       # what dQ contracts
    dG_h = dG_hq if fault != "last_key_row" else torch.zeros_like(dG_hq).scatter_add_(2, ih_b.expand(BH, L, L), dS_h)
    dG_w = torch.zeros(BH, L, 2 * Wp - 1, dtype=torch.float64).scatter_add_(2, iw.expand(BH, L, L), dS)
    dq = s * dS @ k + dG_hq @ Rh + dG_w @ Rw
    if fault == "dg_column_dropped":
        dG_h = dG_h.clone()
        dG_h[..., Hp - 1] = 0
    dk = s * dS.transpose(1, 2) @ q
    dv = Pb.transpose(1, 2) @ do
    rows = lambda t: t.reshape(B, H, L, hd).permute(0, 2, 1, 3).reshape(B * L, H * hd)
    return dict(logits=logits, P=P, dP=dP, delta=delta, dS=dS, dG_h=dG_h, dG_w=dG_w, Gh=Gh, Gw=Gw, out=rows(out), lse=lse,
                dq=rows(dq), dk=rows(dk), dv=rows(dv), drh=torch.einsum("bqj,bqc->jc", dG_h, q), drw=torch.einsum("bqj,bqc->jc", dG_w, q))


def tie_quantum(t):
    """The smallest spacing of the values of `t`: the largest power of two (down to 2^-10) that divides every one of them."""
    for e in range(12, -11, -1):
        x = t.double() * 2.0 ** -e
        if float((x - x.round()).abs().max()) < 1e-9:
            return 2.0 ** e
    raise AssertionError("not dyadic to 2^-10")


def tie_fp32_bounds(case, alg, n_dq=20, n_dg=4):
    """(n_dq, n_dg: the term counts of dQ and of one bias-gradient entry; the defaults are attn_bwd.hip's, derived below;
    any_bwd_fp32_bounds passes attn_any_bwd.hip's.)
    -> dict(dq, dk, dv [B*L, H*hd], drcat [2Hp-1 + 2Wp-1, hd]), f64: how far the fp32 build may be from the exact answer, element by
    element, as (sum of |terms|) * c * 2^-22.  The fp32 build runs the generic kernels.  At a winner s = 0 and the bias is 0, so the
    backward's exponent is -lse2 alone, lse2 = lse * LOG2E_F (attn_bwd.hip:139, :201-204 and :415-418) with lse = (m + log2 l) * LN2_F
    (attn_fwd.hip:150), m = 0 and l = n exactly: v_log_f32 is good to 1 ulp (2^-23 relative), the two multiplications round by 2^-24 each
    and LN2_F * LOG2E_F is 1 - 2^-26.5, so the exponent is off by at most 2.13 * 2^-23 * log2 n <= 4.26 * 2^-23, P by a factor
    1 +- (ln 2 * 4.26 + 1) * 2^-23 (v_exp_f32: 1 ulp) -- under 2 * 2^-22 -- and dS = P * (dP - Delta) (attn_bwd.hip:205-208) by 2.25 * 2^-22
    of itself, dP and Delta being exact.  An fp32 sum of N non-zero terms in whatever order adds at most N * 2^-24 = (N / 4) * 2^-22 of the
    sum of their magnitudes.  So c = 2.25 + N / 4 (dV: 2 + N / 4, it takes P), with N
      dq     20: at most 4 winners -- 4 content products, 4 + 4 additions into the two bias-gradient tables (attn_bwd.hip:209-217), 4 + 4
             table products (attn_bwd.hip:286);
      dk dv  the number of queries the key wins;
      drcat  in three steps.  The bias gradient dG[q][j] is a sum of at most 4 dS, 3.25 * 2^-22 of the sum of their magnitudes off, and
             often far smaller than that sum.  The table gradient is a split-K GEMM over the B * L token rows, one batch per head
             (attn_bwd.hip:618-640): slab (split z, head h) holds the rows [z * klen, (z + 1) * klen) of head h, klen = ceil(ceil(B L / 32) /
             splits) * 32 with splits = min(16, ceil(B L / 32)) (gemm_engine.h:66-71, :228-229; BK = 32 for fp32, common.h:20; 16 is the
             default that ops.py leaves in place), and one accumulator per output element adds a slab's products dG * q in sequence
             (gemm_engine.h:192-217): (N_s / 4) * 2^-22 of the slab's
             sum of |dG| |q|, N_s = its rows with a non-zero dG in that table row.  pa_slab_reduce then adds the S = splits * heads slabs in
             an order this bound does not depend on: (S / 4) * 2^-22 of the whole sum.  (Both taken 1.001 times, for dG's own error.)"""
    B, H, L, hd, Hp, Wp, s = case.B, case.H, case.L, case.hd, case.Hp, case.Wp, case.scale
    q, k, _ = case.qkv.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, B * H, L, hd).unbind(0)
    do = case.dout.double().reshape(B, L, H, hd).permute(0, 2, 1, 3).reshape(B * H, L, hd)
    key = torch.arange(L)
    ih = (key[:, None] // Wp - key[None, :] // Wp + Hp - 1).expand(B * H, L, L)
    iw = (key[:, None] % Wp - key[None, :] % Wp + Wp - 1).expand(B * H, L, L)
    adS = alg["dS"].abs()
    aGh = torch.zeros(B * H, L, 2 * Hp - 1, dtype=torch.float64).scatter_add_(2, ih, adS)
    aGw = torch.zeros(B * H, L, 2 * Wp - 1, dtype=torch.float64).scatter_add_(2, iw, adS)
    fan = (alg["P"] != 0).sum(1).double()[..., None]                                   # [B*H, L, 1]: queries the key wins
    rows = lambda t: t.reshape(B, H, L, hd).permute(0, 2, 1, 3).reshape(B * L, H * hd)
    u = 2.0 ** -22
    aG = torch.cat([aGh, aGw], 2)
    dG = torch.cat([alg["dG_h"], alg["dG_w"]], 2).abs()
    R, nku = B * L, (B * L + 31) // 32
    splits = min(16, nku)
    klen = (nku + splits - 1) // splits * 32
    nsl = (R + klen - 1) // klen

    def slabs(t):       # [B*H, L, X] -> [H, slab, klen, X], token rows b * L + l, zero rows behind the end
        t = t.reshape(B, H, L, -1).permute(1, 0, 2, 3).reshape(H, R, -1)
        return torch.cat([t, t.new_zeros(H, nsl * klen - R, t.shape[-1])], 1).reshape(H, nsl, klen, -1)
    a_slab = torch.einsum("hsrj,hsrc->hsjc", slabs(dG), slabs(q.abs()))
    n_slab = (slabs(aG) != 0).sum(2).double()                                           # [H, slab, J]
    tab_sum = (a_slab * n_slab[..., None] / 4).sum((0, 1)) + a_slab.sum((0, 1)) * (splits * H) / 4
    return dict(dq=rows(s * adS @ k.abs() + aGh @ case.rel_h.double().abs() + aGw @ case.rel_w.double().abs()) * (2.25 + n_dq / 4) * u,
                dk=rows(s * adS.transpose(1, 2) @ q.abs() * (2.25 + fan / 4)) * u,
                dv=rows(alg["P"].transpose(1, 2) @ do.abs() * (2 + fan / 4)) * u,
                drcat=(torch.einsum("bqj,bqc->jc", aG, q.abs()) * (2.25 + n_dg / 4) + tab_sum * 1.001) * u)


def tie_exact_sums(case, alg):
    """-> dict name -> the largest sum of |terms| of any fp32 accumulation behind that tensor, in units of 1/64 (dS is a multiple of 1/16, K
    of 8 = 1 / scale, q of 2, the table entries and dO are integers, P a multiple of 1/4: every term of every sum is a multiple of 1/64 at
    the least).  Below 2^24 every partial sum, in any order, is a multiple of 1/64 that fp32 holds exactly."""
    B, H, L, hd, Hp, Wp, s = case.B, case.H, case.L, case.hd, case.Hp, case.Wp, case.scale
    q, k, v = case.qkv.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, B * H, L, hd).unbind(0)
    do = case.dout.double().reshape(B, L, H, hd).permute(0, 2, 1, 3).reshape(B * H, L, hd)
    key = torch.arange(L)
    ih = (key[:, None] // Wp - key[None, :] // Wp + Hp - 1).expand(B * H, L, L)
    iw = (key[:, None] % Wp - key[None, :] % Wp + Wp - 1).expand(B * H, L, L)
    adS = alg["dS"].abs()
    aGh = torch.zeros(B * H, L, 2 * Hp - 1, dtype=torch.float64).scatter_add_(2, ih, adS)
    aGw = torch.zeros(B * H, L, 2 * Wp - 1, dtype=torch.float64).scatter_add_(2, iw, adS)
    return {"q.k": float((q.abs() @ k.abs().transpose(1, 2)).max()) * 64, "dP": float((do.abs() @ v.abs().transpose(1, 2)).max()) * 64,
            "delta": float((alg["P"] @ v.abs() * do.abs()).sum(-1).max()) * 64, "out": float((alg["P"] @ v.abs()).max()) * 64,
            "dq": float((adS @ k.abs() + aGh @ case.rel_h.double().abs() + aGw @ case.rel_w.double().abs()).max()) * 64,
            "dk": float((adS.transpose(1, 2) @ q.abs()).max()) * 64, "dv": float((alg["P"].transpose(1, 2) @ do.abs()).max()) * 64,
            "drcat": float(torch.einsum("bqj,bqc->jc", torch.cat([aGh, aGw], 2), q.abs()).max()) * 64}


TIE_FAULTS = ("delta_next_row", "kh_class_phase", "last_key_row", "l_previous_row", "dg_column_dropped")


@dataclass(frozen=True)
class TieExpect:
    nwin: torch.Tensor        # int64 [B, H, L]: winners of the row (logit exactly 0)
    loser: torch.Tensor       # f64: the largest logit below the winners, over the whole case
    out: torch.Tensor         # f64 [B*L, H*hd]
    lse: torch.Tensor         # f64 [B*H, L]: log nwin
    dq: torch.Tensor          # f64 [B*L, H*hd] x 3: autograd of attn_reference, the exact dyadic answer
    dk: torch.Tensor
    dv: torch.Tensor
    drcat: torch.Tensor       # f64 [2Hp-1 + 2Wp-1, hd]: d rel_pos_h over d rel_pos_w, the rows attn_bwd_relpos returns in front of its padding


def tie_reference(case):
    """fp64 autograd through attn_reference; the logits it built say who won."""
    B, H, L = case.B, case.H, case.L
    qkv = case.qkv.double().requires_grad_(True)
    rh, rw = case.rel_h.double().requires_grad_(True), case.rel_w.double().requires_grad_(True)
    with _CaptureLogits() as cap:
        out, lse = attn_reference(qkv, rh, rw, B, L, H, case.Hp, case.Wp, case.scale)
    logits = cap.logits.detach()
    assert cap.calls == 1 and logits.dtype == torch.float64 and logits.shape == (B * H, L, L)
    out.backward(case.dout.double())
    D = H * case.hd
    g = qkv.grad
    nwin = (logits == 0).sum(-1)

    def snap(t):        # autograd's values are the dyadic ones to 1e-80 or so; make them the dyadic ones, so that rounding them to bf16 is one rounding
        r = (t.detach() * 1024).round() / 1024
        assert float((r - t.detach()).abs().max()) < 1e-9
        return r.contiguous()
    return TieExpect(nwin.reshape(B, H, L), logits[logits != 0].max(), snap(out), lse.detach(), snap(g[:, :D]), snap(g[:, D:2 * D]),
                     snap(g[:, 2 * D:]), snap(torch.cat([rh.grad, rw.grad], 0)))


@functools.lru_cache(maxsize=None)
def tie_attn_case(kind, B, H, Hp, Wp, hd):
    """As attn_case: one (kind, shape) and its expectation, built once per process, read-only."""
    i = TIE_KINDS.index(kind)
    case = tie_case(B, H, Hp, Wp, hd, TIE_PLACEMENTS[i % 3], i >= 3, 7000 * Hp + 70 * Wp + hd + i)
    return case, tie_reference(case)


def tie_route_params(routes):
    """-> [(route, kind, B, H, Hp, Wp)]: every route and grid of route_params, on the tie kinds of that grid and head dim."""
    out = []
    for route, (_, _, _, _, grids) in routes.items():
        for grid in grids:
            for kind in tie_kinds(grid, routes[route][1]):
                out.append((route, kind) + grid)
    return out


TIE_PREP_LAUNCH_CASES = [(kind, PREP_LAUNCH_GRID) for kind in TIE_KINDS] + [("tie_mirror_sparse", FULL_GRID)]


def tie_shapes():
    """Every distinct (kind, B, H, Hp, Wp, hd) the tie GPU tests build."""
    seen = []
    for routes in (ATTN_ROUTES, SHORT_ROUTES):
        for route, kind, B, H, Hp, Wp in tie_route_params(routes):
            key = (kind, B, H, Hp, Wp, routes[route][1])
            if key not in seen:
                seen.append(key)
    return seen


# ------------------------------------------------------------------------------------------------ attention on any token grid
# csrc/attn_any.hip (pa_attn_any_fwd) is the generic forward with other index arithmetic: the exact cases above carry over to ragged grids.
# This section: the forward (tests/test_attention_any_exact_gpu.py; conditions and named wrong forwards in tests/test_exact_cases_cpu.py);
# the backward of csrc/attn_any_bwd.hip has the section after it.
# (B, H, Hp, Wp), each the smallest grid that reaches what it names:
ANY_RAGGED = [(2, 2, 2, 1),       # L = 2, Wp = 1, one wave live
              (2, 2, 6, 3),       # the Wp < 4 branch, a single partial tile
              (2, 2, 11, 2),      # the same with Wp = 2
              (1, 2, 3, 11),      # L = 33: the last tile holds 1 key
              (2, 2, 9, 7),       # L = 63: the last tile holds 31 keys
              (2, 2, 10, 5),      # the grid of the model-level fixture
              (2, 2, 5, 13),      # L = 65: three query tiles and one idle wave
              (2, 2, 4, 33),      # Wp > 32: a tile lies inside one key row; five tiles, the second workgroup has one live wave
              (2, 2, 12, 6),      # L % 4 == 0 and Wp % 4 != 0
              (1, 1, 35, 17)]     # L = 595, half of 70 x 35: 19 tiles, five workgroups
ANY_BIAS_ONLY = (1, 1, 62, 31)    # L = 1922, bias_rank alone: the content cases' margin drops to 132 there, below MIN_MARGIN
ANY_ALIGNED = [(2, 2, 8, 4), (2, 2, 8, 28)]       # grids pa_attn_fwd takes as well: both kernels must equal the expectation
ANY_TIE_ONLY = [(2, 2, 10, 6),    # L = 60: tied winners with a partial tile
                (2, 2, 12, 3)]    # ... and in the Wp < 4 branch
ANY_HD80_MAX_L = 200
ANY_KINDS = ATTN_KINDS + ("below_zero",)
# 70 x 35 itself (the COCO panoptic size) stays with the tolerance test tests/test_any_size_gpu.py::test_attn_any_vs_float64:
# position_coded_v holds Hp, Wp <= 63.


def _any_grids(hd):
    grids = ANY_RAGGED + [ANY_BIAS_ONLY] + ANY_ALIGNED + ANY_TIE_ONLY
    return [g for g in grids if hd == 64 or g[2] * g[3] <= ANY_HD80_MAX_L]


# route -> (dtype name, head_dim, the launch counter that must move by one per call, [(B, H, Hp, Wp)])
ANY_ROUTES = {"any_bf16_hd64": ("bf16", 64, "pa_attn_any_launches", _any_grids(64)),
              "any_bf16_hd80": ("bf16", 80, "pa_attn_any_launches", _any_grids(80)),
              "any_fp32_hd64": ("fp32", 64, "pa_attn_any_launches", _any_grids(64)),
              "any_fp32_hd80": ("fp32", 80, "pa_attn_any_launches", _any_grids(80))}


def any_kinds(grid):
    """The kinds one grid runs: the six gather kinds and below_zero, and all six tie kinds where L % 4 == 0 (forward only: a dense dO
    costs nothing here, so head dim 80 runs the dense kinds too)."""
    if grid == ANY_BIAS_ONLY:
        return ("bias_rank",)
    if grid in ANY_TIE_ONLY:
        return TIE_KINDS
    return ANY_KINDS + (TIE_KINDS if grid[2] * grid[3] % 4 == 0 else ())


def any_route_params():
    """-> [(route, kind, B, H, Hp, Wp)] in the order the GPU tests run them."""
    return [(route, kind) + grid for route, spec in ANY_ROUTES.items() for grid in spec[3] for kind in any_kinds(grid)]


def any_shapes():
    """Every distinct (kind, B, H, Hp, Wp, hd) the any-grid GPU tests build."""
    seen = []
    for route, kind, B, H, Hp, Wp in any_route_params():
        key = (kind, B, H, Hp, Wp, ANY_ROUTES[route][1])
        if key not in seen:
            seen.append(key)
    return seen


BELOW_ZERO_CHANNEL = 37


def below_zero_case(B, H, Hp, Wp, hd, seed):
    """content_case on a permutation with channel 37 turned into a shift channel, the way tie_case does it: K = -8 (hd + 24) there in
    every key and q = a_q.  The target's logit is a_q (hd - 1) from the hd - 1 code channels and -a_q (hd + 24) from the shift channel:
    -25 a_q = -150, -200 or -250, every other key's lower by 2 a_q per code channel it differs in.  EVERY logit of every row is far below
    zero -- the first tile's running maximum too, the regime of the generation-2 / 3 NaN -- and a key >= L that stayed alive with its zeroed
    K row (logit 0) would win every row by >= 150 and return its zero V row."""
    base = content_case(B, H, Hp, Wp, hd, "permutation", seed)
    L = Hp * Wp
    x = base.qkv.clone().reshape(B, L, 3, H, hd)
    amp = torch.tensor(AMPLITUDES, dtype=torch.float32)[torch.arange(L) % len(AMPLITUDES)]
    x[:, :, 0, :, BELOW_ZERO_CHANNEL] = amp[None, :, None]
    x[:, :, 1, :, BELOW_ZERO_CHANNEL] = -8.0 * (hd + 24)
    return AttnCase("below_zero", B, H, Hp, Wp, hd, x.reshape(B * L, 3 * H * hd).contiguous(), base.rel_h, base.rel_w, base.dout)


@functools.lru_cache(maxsize=None)
def any_case(kind, B, H, Hp, Wp, hd):
    """-> (case, AttnExpect | TieExpect) of one (kind, shape): the cases of attn_case and tie_attn_case as they are (shared with the routes
    above where the grid is), below_zero built here.  Read-only."""
    if kind in TIE_KINDS:
        return tie_attn_case(kind, B, H, Hp, Wp, hd)
    if kind == "below_zero":
        case = below_zero_case(B, H, Hp, Wp, hd, 1000 * Hp + 10 * Wp + hd + len(ATTN_KINDS))
        return case, reference(case)
    return attn_case(kind, B, H, Hp, Wp, hd)


ANY_FAULTS = ("row_of_first_key", "column_wrap_zero", "carry_lost", "tail_keys_alive", "last_key_dropped", "tail_tile_dropped",
              "pad_row_stored")


def any_key_walk(L, Hp, Wp, fault=None):
    """The key walk of attn_any.hip restated -> (kh, kw, zero_col), [ceil(L / 32) * 32] each: for every key slot of every 32-key tile the
    key row (clamped to Hp - 1, as the kernel clamps it) and key column whose table entries the logit takes, and whether the column entry
    reads as 0.  A tile is eight runs of four keys; a run starts at the (kh, kw) its lane carries from tile to tile -- + 32 / Wp rows,
    + 32 % Wp columns, one carry -- and steps key by key.  (For Wp >= 4 the kernel does not step: it selects between two row entries and
    reads four consecutive column entries from a table that repeats its first three behind its end, which is the same walk.)  Faults:
      row_of_first_key   the keys of a run behind a row crossing take the run's first row
      column_wrap_zero   the same keys read a zero column entry (the repeated entries were never written)
      carry_lost         the per-tile column wrap does not bump the row"""
    nt = (L + 31) // 32
    kh, kw = torch.empty(nt * 32, dtype=torch.int64), torch.empty(nt * 32, dtype=torch.int64)
    zero = torch.zeros(nt * 32, dtype=torch.bool)
    start = [((4 * r) // Wp, (4 * r) % Wp) for r in range(8)]
    for j in range(nt):
        for r in range(8):
            h0, w0 = start[r]
            hh, ww = h0, w0
            for t in range(4):
                k = 32 * j + 4 * r + t
                kh[k] = h0 if fault == "row_of_first_key" else hh
                kw[k] = ww
                zero[k] = fault == "column_wrap_zero" and hh != h0
                ww += 1
                if ww == Wp:
                    ww, hh = 0, hh + 1
            h0, w0 = h0 + 32 // Wp, w0 + 32 % Wp
            if w0 >= Wp:
                h0, w0 = h0 + (0 if fault == "carry_lost" else 1), w0 - Wp
            start[r] = (h0, w0)
    return kh.clamp_max(Hp - 1), kw, zero


def any_algebra(case, fault=None):
    """The any-grid forward written out in fp64 over the kernel's own key walk -> dict(logits [B*H, L, Lp], out [B*L, H*hd], lse [B*H, L]),
    Lp = the keys of whole tiles.  Without `fault` it is the expectation once more; with one it is what a named wrong kernel would
    return (real outputs, not an argmax).  The walk faults: any_key_walk.  The others:
      tail_keys_alive    keys >= L keep their zeroed K and V rows, a clamped row entry and a FINITE logit
      last_key_dropped   key L - 1 is left out
      tail_tile_dropped  the partial last tile is skipped (with a single tile every row is 0 / 0 = NaN)
      pad_row_stored     rows >= L of the last query tile -- copies of row L - 1 -- are written where they point: the next sample's first rows
    Winners at a common logit with every other key >= 150 below give exactly 1 / n here: exp(0) = 1, the losers' exp() is below 1e-65."""
    B, H, L, hd, Hp, Wp, s = case.B, case.H, case.L, case.hd, case.Hp, case.Wp, case.scale
    assert fault is None or fault in ANY_FAULTS
    q, k, v = case.qkv.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, B * H, L, hd).unbind(0)
    Rh, Rw = case.rel_h.double(), case.rel_w.double()
    kh, kw, zero = any_key_walk(L, Hp, Wp, fault)
    Lp, BH = kh.numel(), B * H
    alive = torch.arange(Lp) < L
    if fault == "tail_keys_alive":
        alive[:] = True
    elif fault == "last_key_dropped":
        alive[L - 1] = False
    elif fault == "tail_tile_dropped" and L % 32:
        alive[L // 32 * 32:] = False
    pad = torch.zeros(BH, Lp - L, hd, dtype=torch.float64)
    kx, vx = torch.cat([k, pad], 1), torch.cat([v, pad], 1)
    qi = torch.arange(L)
    ih = (qi[:, None] // Wp - kh[None, :] + Hp - 1).expand(BH, L, Lp)                # the table rows of (query, key slot)
    iw = (qi[:, None] % Wp - kw[None, :] + Wp - 1).expand(BH, L, Lp)
    Gh, Gw = q @ Rh.t(), q @ Rw.t()
    logits = (s * q) @ kx.transpose(1, 2) + torch.gather(Gh, 2, ih) + torch.gather(Gw, 2, iw) * (~zero).double()[None, None, :]
    logits = logits.masked_fill(~alive[None, None, :], float("-inf"))
    m = logits.max(-1, keepdim=True).values
    e = torch.exp(logits - m)
    l = e.sum(-1, keepdim=True)
    out = ((e / l) @ vx).reshape(B, H, L, hd).permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous()
    if fault == "pad_row_stored":
        for b in range(B - 1):
            n = min(Lp - L, L)
            out[(b + 1) * L:(b + 1) * L + n] = out[b * L + L - 1]
    return dict(logits=logits, out=out, lse=(m + torch.log(l)).squeeze(-1))


# ------------------------------------------------------------------------------------------------ attention on any token grid: the backward
# csrc/attn_any_bwd.hip (pa_attn_any_bwd): the tie cases on ragged grids (tie_loners lifts L % 4 == 0) and the gather kinds, held to
# equality by tests/test_attention_any_bwd_exact_gpu.py; conditions, caps and named wrong backwards in tests/test_exact_cases_cpu.py.
# (B, H, Hp, Wp) of the tie kinds, each the smallest grid that reaches what it names:
ANY_BWD_TIE_GRIDS = [(2, 2, 12, 3),     # the Wp < 4 stepping branch; L = 36: a partial second tile
                     (2, 2, 6, 3),      # the same with L = 18: one partial tile
                     (2, 2, 9, 7),      # 4 <= Wp < 8; L = 63
                     (2, 2, 10, 5),     # the grid of the model-level fixture
                     (2, 2, 12, 6),     # L % 4 == 0 and Wp % 4 != 0
                     (1, 2, 3, 11),     # Wp >= 8; L = 33: one key and one query row in the last tile
                     (2, 2, 5, 13),     # L = 65: the same, and one idle wave in both kernels
                     (2, 2, 4, 33),     # Wp > 32
                     (2, 2, 8, 4),      # aligned: pa_attn_bwd must return the same values
                     (2, 2, 31, 19)]    # L = 589: 19 tiles, five workgroups.  (In place of (1, 1, 35, 17), which misses its cap: with one
#                                         sample and one head every kind leaves a key of the last tile, or a tie row of the last query
#                                         tile, without a non-zero dS; (2, 2, 35, 17) loses tie_near_sparse to the same condition.)
ANY_BWD_GATHER_ONLY = [(2, 2, 1, 1), (2, 2, 2, 1), (2, 2, 11, 2), (2, 2, 5, 2)]       # too few keys for groups of four, or Wp = 2 once more
ANY_BWD_ALIGNED = (2, 2, 8, 4)
ANY_BWD_CHAIN = ("tie_mirror_sparse", (2, 2, 8, 5), 64)      # through the resize adjoint: table lengths 15 -> 45 and 9 -> 27, both dyadic pairs
# route -> (dtype name, head_dim, the launch counter that must move by one per call, [(B, H, Hp, Wp)])
ANY_BWD_ROUTES = {"any_bwd_%s_hd%d" % (t, hd): (t, hd, "pa_attn_any_bwd_launches", ANY_BWD_TIE_GRIDS + ANY_BWD_GATHER_ONLY)
                  for t in ("bf16", "fp32") for hd in (64, 80)}
# Tie kinds that are NOT exact on a grid, (head dim, grid) -> {kind: the condition of any_bwd_condition_failed that fails}: found by running
# that function, and asserted -- each entry fails as it says, every kind not listed passes -- by tests/test_exact_cases_cpu.py.  A dense dO
# meets V magnitudes up to 64 (the fifth field of head dim 80, key rows and columns of the larger grids): some dS or class sum then needs a
# ninth significant bit.
_DS, _DK, _ROWS = "bf16-exact dS", "dyadic to 1/32: dk", "last query tile: every tie row has a non-zero dS"
ANY_BWD_LEFT_OUT = {
    (64, (2, 2, 12, 3)): {"tie_near": _DK, "tie_near_sparse": _DK},       # L % 4 == 0: the case is today's, amplitude 14 in four-winner rows
    (64, (2, 2, 9, 7)): {"tie_quarter_sparse": _ROWS},
    (64, (2, 2, 4, 33)): {"tie_near": _DS, "tie_mirror": _DS},
    (64, (2, 2, 8, 4)): {"tie_quarter_sparse": _ROWS},
    (64, (2, 2, 31, 19)): {"tie_near": _DS, "tie_quarter": _DS, "tie_mirror": _DS},
    (80, (2, 2, 12, 3)): {"tie_near": _DK, "tie_near_sparse": _DK},
    (80, (2, 2, 9, 7)): {"tie_quarter": _DS, "tie_mirror": _DS, "tie_mirror_sparse": _DS},
    (80, (2, 2, 10, 5)): {"tie_near": _DS, "tie_quarter": _DS, "tie_mirror": _DS},
    (80, (2, 2, 12, 6)): {"tie_quarter": _DS, "tie_mirror": _DS},
    (80, (1, 2, 3, 11)): {"tie_quarter": _DS, "tie_mirror": _DS},
    (80, (2, 2, 5, 13)): {"tie_near": _DS, "tie_quarter": _DS},
    (80, (2, 2, 4, 33)): {"tie_near": _DS, "tie_quarter": _DS, "tie_mirror": _DS},
    (80, (2, 2, 31, 19)): {"tie_near": _DS, "tie_quarter": _DS, "tie_mirror": _DS, "tie_quarter_sparse": _DS},
}
# ... and in the fp32 build alone (the bound of any_bwd_fp32_bounds reaches half a quantum somewhere): none
ANY_BWD_LEFT_OUT_FP32 = {}


def any_bwd_kinds(route, grid):
    """The kinds one route runs on one grid: the gather kinds and below_zero everywhere, and every tie kind that is exact there."""
    tname, hd = ANY_BWD_ROUTES[route][:2]
    if grid in ANY_BWD_GATHER_ONLY:
        return ANY_KINDS
    out = set(ANY_BWD_LEFT_OUT.get((hd, grid), {})) | (set(ANY_BWD_LEFT_OUT_FP32.get((hd, grid), {})) if tname == "fp32" else set())
    return ANY_KINDS + tuple(k for k in TIE_KINDS if k not in out)


def any_bwd_route_params():
    """-> [(route, kind, B, H, Hp, Wp)] in the order the GPU tests run them."""
    return [(route, kind) + grid for route, spec in ANY_BWD_ROUTES.items() for grid in spec[3] for kind in any_bwd_kinds(route, grid)]


def any_bwd_shapes():
    """Every distinct (kind, B, H, Hp, Wp, hd) the any-grid backward tests build, the chain case included."""
    seen = [(ANY_BWD_CHAIN[0],) + ANY_BWD_CHAIN[1] + (ANY_BWD_CHAIN[2],)]
    for route, kind, B, H, Hp, Wp in any_bwd_route_params():
        key = (kind, B, H, Hp, Wp, ANY_BWD_ROUTES[route][1])
        if key not in seen:
            seen.append(key)
    return seen


def _bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).double(), t.double())


def any_bwd_fp32_bounds(case, alg):
    """tie_fp32_bounds for csrc/attn_any_bwd.hip.  The arithmetic per logit is attn_bwd.hip's in the same form: lse = (m + log2 l) * LN2_F
    (attn_any.hip:177), lse2 = lse * LOG2E_F (attn_any_bwd.hip:74; kernel B reads the same lse2 from the aux tile, :86 and :426),
    p = exp2(fma(s, scale * log2e, bias) - lse2) (:163, :434), dS = p * (dP - Delta) (:164, :436): dS is 2.25 * 2^-22 of itself off, dV's
    P 2 * 2^-22, as derived in tie_fp32_bounds.  The term counts differ:
      bias gradient  one entry of a query's row or column table takes a non-zero dS through at most 5 additions: the partial sum over the
                     eight keys of a register group (r0 / r1, :179-183; acc, :185-196) holds at most 4 non-zero values -- a row has at most 4
                     winners -- and is added to the table once (:182, :183, :191, :196); a column entry takes them one by one (:210, :214).
                     n_dg = 5: (2.25 + 5 / 4) * 2^-22 of the sum of |dS|.
      dq             4 content products (:229) + 5 + 5 for the two tables + 4 + 4 table products (:288): n_dq = 22.
      dk dv          the number of queries the key wins (:451, :452), as before.
      drcat          the same pa_attn_bwd_relpos at B * L token rows (:629): the slab arithmetic of tie_fp32_bounds, which pads the last
                     slab with zero rows where B * L is no multiple of its length -- the GEMM engine bounds its K tiles by B * L."""
    return tie_fp32_bounds(case, alg, n_dq=22, n_dg=5)


def any_bwd_condition_failed(case, exp, alg, fp32=False):
    """The conditions a tie case must meet for the any-grid backward to be exact on it -> None, or the name of the first that fails."""
    B, H, L, hd = case.B, case.H, case.L, case.hd
    loners = tie_loners(L, case.Wp)
    last = (L - 1) // 32 * 32
    logits, dS = alg["logits"], alg["dS"]
    nwin = (logits == 0).sum(-1)
    if set(nwin.unique().tolist()) != {1, 2, 4} or not torch.equal(nwin.reshape(B, H, L), exp.nwin) or float(logits.max()) != 0:
        return "winner counts"
    if not bool((nwin[:, L - 1] == 4).all()):
        return "last row has four winners"
    if float(exp.loser) > -MIN_MARGIN:
        return "margin"
    if L > 32 and any(k >= last for k in loners):
        return "last tile in full groups"
    alive = [k for k in range(last, L) if k not in loners]
    if not bool((dS[:, :, alive] != 0).any(1).any(0).all()):
        return "last tile: every key has a non-zero dS"
    tie_rows = (nwin[:, last:] > 1)
    if not bool(((dS[:, last:] != 0).any(-1) | ~tie_rows).any(0).all()):
        return "last query tile: every tie row has a non-zero dS"
    if max(tie_exact_sums(case, alg).values()) >= 2 ** 24:
        return "fp32 sums below 2^24"
    for name in ("out", "P", "dS", "dG_h", "dG_w"):
        if not _bf16_exact(alg[name]):
            return "bf16-exact " + name
    want = dict(dq=exp.dq, dk=exp.dk, dv=exp.dv, drcat=exp.drcat)
    for name, t in want.items():
        if float((t * 32 - (t * 32).round()).abs().max()) > 1e-9 or float(t.abs().max()) >= 2 ** 15:
            return "dyadic to 1/32: " + name
    if fp32:
        bound = any_bwd_fp32_bounds(case, alg)
        for name, t in want.items():
            if float(bound[name].max()) >= 0.5 * tie_quantum(t):
                return "fp32 bound below half a quantum: " + name
    return None


ANY_BWD_FAULTS = ("row_carry_lost_in_group", "half1_offset_no_wrap", "tile_carry_lost", "column_wrap_lost", "tail_keys_alive_dq",
                  "tail_keys_alive_dkv", "tail_rows_alive_dkv", "aux_row_shift", "dg_emit_off_by_one", "last_tile_skipped_in_table_gradient")


def any_bwd_key_walk(L, Hp, Wp, fault=None):
    """Kernel A's key walk (attn_any_bwd.hip:106-236) restated -> (bh, bw, rh, cw), int64 [ceil(L / 32) * 32] each: per key slot the row
    entry (clamped to Hp - 1) and column entry of the bias READ, and the row entry (Hp: none, the value is dropped) and column entry
    (>= Wp: behind the table, lost) that its dS is ADDED to.  Per tile and register group rg the two half-waves of a query hold keys
    8 rg .. 8 rg + 7; (kh8, kw8) is the row and column of key 8 rg, advanced per tile by 32 / Wp rows and 32 % Wp columns with one carry.
      read   half g starts 4 g keys behind (kh8, kw8), wrapping with a while loop; Wp >= 4: row entry hh for the keys in front of the
             crossing and hh + 1 behind it, four consecutive column entries; Wp < 4: (hh, ww) steps per key;
      rows   half 0: Wp >= 8: r0 = the keys in front of the crossing into row hh, r1 = the rest into row hh + 1 (dropped where hh + 1 = Hp:
             keys >= L only); Wp < 8: stepping, the sum flushed at every crossing;
      cols   half 1: the column steps per key and wraps to 0.
    Faults: row_carry_lost_in_group (r1 into row hh), half1_offset_no_wrap (the read of half 1 keeps row kh8 across the wrap of its + 4
    columns), tile_carry_lost (the per-tile wrap of kw8 does not bump kh8), column_wrap_lost (the column sum's ww runs on past Wp)."""
    nt = (L + 31) // 32
    bh, bw, rh, cw = (torch.empty(nt * 32, dtype=torch.int64) for _ in range(4))
    kh8, kw8 = [8 * rg // Wp for rg in range(4)], [8 * rg % Wp for rg in range(4)]
    for j in range(nt):
        for rg in range(4):
            for g in (0, 1):
                hh, ww = kh8[rg], kw8[rg]
                if g:
                    ww += 4
                    while ww >= Wp:
                        ww -= Wp
                        hh += 0 if fault == "half1_offset_no_wrap" else 1
                for t in range(4):
                    slot = 32 * j + 8 * rg + 4 * g + t
                    if Wp >= 4:
                        bh[slot] = min(hh if t < Wp - ww else hh + 1, Hp - 1)
                        bw[slot] = (ww + t) % Wp                    # (the column part repeats its first three entries behind its end)
                    else:
                        bh[slot], bw[slot] = min(hh, Hp - 1), ww
                        ww += 1
                        if ww == Wp:
                            ww, hh = 0, hh + 1
            hh, ww = kh8[rg], kw8[rg]
            w2 = ww
            for t in range(8):
                slot = 32 * j + 8 * rg + t
                if Wp >= 8:
                    if t < Wp - kw8[rg]:
                        rh[slot] = min(hh, Hp - 1)
                    else:
                        rh[slot] = Hp if hh + 1 >= Hp else (min(hh, Hp - 1) if fault == "row_carry_lost_in_group" else hh + 1)
                else:
                    rh[slot] = min(hh, Hp - 1)
                    ww += 1
                    if ww == Wp:
                        ww, hh = 0, hh + 1
                cw[slot] = w2
                w2 += 1
                if w2 == Wp and fault != "column_wrap_lost":
                    w2 = 0
            kh8[rg] += 32 // Wp
            kw8[rg] += 32 % Wp
            if kw8[rg] >= Wp:
                kw8[rg] -= Wp
                kh8[rg] += 0 if fault == "tile_carry_lost" else 1
    return bh, bw, rh, cw


def any_bwd_algebra(case, fault=None, base=None):
    """The any-grid backward written out in fp64 over kernel A's own key walk (any_bwd_key_walk), kernel B and the dG emit
    (attn_any_bwd.hip:254-270) -> dict(dS [B*H, L, L], tab_h [B*H, L, Hp], tab_w [B*H, L, Wp], dG_h, dG_w, dq, dk, dv [B*L, H*hd], drh, drw,
    drcat), from the right forward (`base` = tie_algebra(case): lse, Delta, dP).  Without `fault` it is tie_algebra's backward once more;
    with one it is what a named wrong kernel would return (inf and NaN included: an fp64 exp() overflows later than fp32's).  The walk
    faults: any_bwd_key_walk.  The others:
      tail_keys_alive_dq    kernel A, keys >= L keep p = exp2(bias - lse2) with their zeroed K and V rows: dS = -p Delta into the clamped
                            row entry and a column entry
      tail_keys_alive_dkv   kernel B computes and stores keys >= L (zeroed K and V, the table rows of key L - 1): their dK and dV rows land
                            where they point, on the next sample's first rows
      tail_rows_alive_dkv   kernel B counts the query rows >= L of the last tile as copies of row L - 1
      aux_row_shift         kernel B reads the lse and Delta of the next query (of the head's first for its last)
      dg_emit_off_by_one    khh = qh + Hp - r: the emitted dG_h is one table row off, in dQ's bias part and in the table gradient
      last_tile_skipped_in_table_gradient   the contraction stops at floor(B L / 32) * 32 token rows"""
    assert fault is None or fault in ANY_BWD_FAULTS
    B, H, L, hd, Hp, Wp, s = case.B, case.H, case.L, case.hd, case.Hp, case.Wp, case.scale
    base = base if base is not None else tie_algebra(case)
    q, k, v = case.qkv.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, B * H, L, hd).unbind(0)
    do = case.dout.double().reshape(B, L, H, hd).permute(0, 2, 1, 3).reshape(B * H, L, hd)
    Rh, Rw = case.rel_h.double(), case.rel_w.double()
    bh, bw, rh, cw = any_bwd_key_walk(L, Hp, Wp, fault)
    Lp, BH = bh.numel(), B * H
    pad = torch.zeros(BH, Lp - L, hd, dtype=torch.float64)
    kx, vx = torch.cat([k, pad], 1), torch.cat([v, pad], 1)
    qi = torch.arange(L)
    qh, qw = qi // Wp, qi % Wp
    lse, delta, Gh, Gw = base["lse"], base["delta"], base["Gh"], base["Gw"]
    # kernel A
    ih = (qh[:, None] - bh[None, :] + Hp - 1).expand(BH, L, Lp)
    iw = (qw[:, None] - bw[None, :] + Wp - 1).expand(BH, L, Lp)
    logits = (s * q) @ kx.transpose(1, 2) + torch.gather(Gh, 2, ih) + torch.gather(Gw, 2, iw)
    true = torch.cat([base["logits"], torch.full((BH, L, Lp - L), float("-inf"), dtype=torch.float64)], 2)
    P = torch.where(logits == true, torch.cat([base["P"], torch.zeros(BH, L, Lp - L, dtype=torch.float64)], 2),
                    torch.exp(logits - lse[..., None]))
    alive = torch.arange(Lp) < (Lp if fault == "tail_keys_alive_dq" else L)
    dS = torch.where(alive[None, None, :], P * (do @ vx.transpose(1, 2) - delta[..., None]), torch.zeros((), dtype=torch.float64))
    tab_h = torch.zeros(BH, L, Hp + 1, dtype=torch.float64).index_add_(2, rh, dS)[..., :Hp]
    tab_w = torch.zeros(BH, L, Wp + 8, dtype=torch.float64).index_add_(2, cw, dS)[..., :Wp]
    khh = qh[:, None] + Hp - 1 - torch.arange(2 * Hp - 1)[None, :] + (1 if fault == "dg_emit_off_by_one" else 0)
    kww = qw[:, None] + Wp - 1 - torch.arange(2 * Wp - 1)[None, :]
    dG_h = torch.gather(tab_h, 2, khh.clamp(0, Hp - 1).expand(BH, L, -1)) * ((khh >= 0) & (khh < Hp))[None]
    dG_w = torch.gather(tab_w, 2, kww.clamp(0, Wp - 1).expand(BH, L, -1)) * ((kww >= 0) & (kww < Wp))[None]
    dq = s * dS @ kx + dG_h @ Rh + dG_w @ Rw
    tok = (torch.arange(B)[:, None, None] * L + qi[None, None, :]).expand(B, H, L).reshape(BH, L)
    live = (tok < (B * L // 32 * 32 if fault == "last_tile_skipped_in_table_gradient" else B * L)).double()[..., None]
    drh, drw = torch.einsum("bqj,bqc->jc", dG_h * live, q), torch.einsum("bqj,bqc->jc", dG_w * live, q)
    # kernel B: each key's own (row, column), lse2 and Delta from the aux tile
    lse_b, delta_b = (lse.roll(-1, 1), delta.roll(-1, 1)) if fault == "aux_row_shift" else (lse, delta)
    Pb = base["P"] * torch.exp(lse - lse_b)[..., None]
    dSb = Pb * (base["dP"] - delta_b[..., None])
    dk, dv = s * dSb.transpose(1, 2) @ q, Pb.transpose(1, 2) @ do
    if fault == "tail_rows_alive_dkv":
        dk = dk + (Lp - L) * s * dSb[:, L - 1, :, None] * q[:, L - 1, None, :]
        dv = dv + (Lp - L) * Pb[:, L - 1, :, None] * do[:, L - 1, None, :]
    rows = lambda t: t.reshape(B, H, L, hd).permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous()
    dk, dv = rows(dk), rows(dv)
    if fault == "tail_keys_alive_dkv" and Lp > L:
        ihl, iwl = qh + Hp - 1 - (L - 1) // Wp, qw + Wp - 1 - (L - 1) % Wp
        p = torch.exp(Gh[:, qi, ihl] + Gw[:, qi, iwl] - lse)                                   # [BH, L]
        pk, pv = s * torch.einsum("bq,bqc->bc", -p * delta, q), torch.einsum("bq,bqc->bc", p, do)
        n = min(Lp - L, L)
        for b in range(B - 1):
            dk.reshape(B, L, H, hd)[b + 1, :n] = pk.reshape(B, H, hd)[b][None]
            dv.reshape(B, L, H, hd)[b + 1, :n] = pv.reshape(B, H, hd)[b][None]
    return dict(dS=dS[..., :L], tab_h=tab_h, tab_w=tab_w, dG_h=dG_h, dG_w=dG_w, dq=rows(dq), dk=dk, dv=dv, drh=drh, drw=drw,
                drcat=torch.cat([drh, drw], 0))


# ------------------------------------------------------------------------------------------------ 3x3 convolution
C = 64
# route -> (dtype name, (B, Hi, Wi), P, takes the tile kernels of conv64.h)
CONV_ROUTES = {"bf16_tile": ("bf16", (2, 8, 128), 8, True), "bf16_gather_p16": ("bf16", (2, 16, 96), 16, False),
               "bf16_gather_p14": ("bf16", (2, 28, 56), 14, False), "fp32": ("fp32", (2, 8, 64), 8, False)}
CONV_KINDS = ("int", "stamp")
WGRAD_CAPS = (0, 1, 3, 5)     # knob 9 on the tile route: workgroups that walk many tiles


@dataclass(frozen=True)
class ConvCase:
    kind: str
    x: torch.Tensor           # f32 NHWC [B, Hi, Wi, 64]
    dy: torch.Tensor          # f32 NHWC: the output gradient of the data-gradient check
    dy_w: torch.Tensor        # f32 NHWC: the output gradient of the weight-gradient check
    w3: torch.Tensor          # f32 [cout, cin, 3, 3]
    b3: torch.Tensor          # f32 [64]
    hot: tuple = ()           # stamp case: ((b, row, col, channel), ...), the hot pixels of x and of dy


def conv_int_case(B, Hi, Wi, seed):
    """x and dy sparse ternary (non-zero with probability 1/3), w3 ternary, b3 an integer in [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    sparse = lambda: _ternary((B, Hi, Wi, C), g) * (torch.rand((B, Hi, Wi, C), generator=g) < 0.5).float()      # 2/3 * 1/2 = 1/3 non-zero
    x, dy = sparse(), sparse()
    return ConvCase("int", x, dy, dy, _ternary((C, C, 3, 3), g), torch.randint(-8, 9, (C,), generator=g).float())


def stamp_weight():
    """w3[co][ci][ky][kx] = s(co) * (1 + 3 ky + kx + 9 (ci mod 8)), s alternating over co: magnitudes 1 .. 72 (inside the 81 allowed)."""
    co, ci, ky, kx = torch.meshgrid(torch.arange(C), torch.arange(C), torch.arange(3), torch.arange(3), indexing="ij")
    return ((1 - 2 * (co % 2)) * (1 + 3 * ky + kx + 9 * (ci % 8))).float()


def stamp_bias():
    return (torch.arange(C) % 17 - 8).float()


def decode_stamp(value):
    """|weight| -> (ky, kx, ci mod 8) of stamp_weight(), or None."""
    m = int(round(abs(float(value)))) - 1
    if m < 0 or m >= 72 or abs(float(value)) != m + 1:
        return None
    return dict(ky=(m % 9) // 3, kx=m % 3, ci_mod_8=m // 9)


def stamp_pixels(B, Hi, Wi):
    """Hot pixels (b, row, col), at least 3 apart within a sample: sample 0 -- the four corners (the last one is the sample's last pixel),
    the middle of each edge, rows 1 | 2 (weight-gradient tile boundary) and rows 3 | 4 (forward tile boundary); sample 1 -- its first pixel,
    its last pixel, columns 63 | 64 (strip boundary) where Wi > 64, and rows 1 | 2 and 3 | 4 once more at other columns."""
    px = [(0, 0, 0), (0, 0, Wi - 1), (0, Hi - 1, 0), (0, Hi - 1, Wi - 1),
          (0, 0, Wi // 2), (0, Hi - 1, Wi // 2), (0, Hi // 2, 0), (0, Hi // 2, Wi - 1),
          (0, 1, 5), (0, 2, 8), (0, 3, 11), (0, 4, 14)]
    if B > 1:
        px += [(1, 0, 0), (1, Hi - 1, Wi - 1), (1, 1, 20), (1, 2, 23), (1, 3, 26), (1, 4, 29)]
        if Wi > 64:
            px += [(1, 2, 63), (1, 5, 64)]
    for i, (b, r, c) in enumerate(px):
        assert 0 <= r < Hi and 0 <= c < Wi
        for (b2, r2, c2) in px[:i]:
            assert b != b2 or max(abs(r - r2), abs(c - c2)) >= 3, ((b, r, c), (b2, r2, c2))
    return px


def conv_stamp_case(B, Hi, Wi):
    """x (and dy for the data gradient) zero except single ones at stamp_pixels(), each in another channel: the output around a hot pixel is
    the flipped (data gradient: un-flipped) kernel of that channel, stamped; everywhere else it is b3 (data gradient: 0).  For the weight
    gradient dy_w is hot one tap away from each hot x pixel -- the tap cycles over the nine, clipped at the border, and is forced across
    each boundary: row 1 -> 2, 2 -> 1, 3 -> 4, 4 -> 3, column 63 -> 64, 64 -> 63, and sample 0's last pixel pairs with the hot first pixel of
    sample 1, which is NOT its neighbour."""
    px = stamp_pixels(B, Hi, Wi)
    x, dy, dy_w = (torch.zeros(B, Hi, Wi, C) for _ in range(3))
    hot = []
    for i, (b, r, c) in enumerate(px):
        ch = (11 * i + 3) % C
        hot.append((b, r, c, ch))
        x[b, r, c, ch] = 1.0
        dy[b, r, c, ch] = 1.0
        dr, dc = i % 3 - 1, (i // 3) % 3 - 1
        if r in (1, 3) and c not in (0, Wi - 1):
            dr = 1
        elif r in (2, 4) and c not in (0, Wi - 1, 63):
            dr = -1
        if c == 63:
            dr, dc = 0, 1
        elif c == 64 and r not in (0, Hi - 1):
            dr, dc = 0, -1
        r2, c2 = min(max(r + dr, 0), Hi - 1), min(max(c + dc, 0), Wi - 1)
        dy_w[b, r2, c2, (7 * i + 1) % C] = 1.0
    return ConvCase("stamp", x, dy, dy_w, stamp_weight(), stamp_bias(), tuple(hot))


@dataclass(frozen=True)
class ConvExpect:
    y3: torch.Tensor          # int64 NHWC: conv + b3
    dx: torch.Tensor          # int64 NHWC: the transposed conv of dy
    dw: torch.Tensor          # int64 [cout, cin, 3, 3]: the weight gradient of (dy_w, x)


def conv_reference(case):
    """int64, by the shifted matmuls of tests/test_vit_huge_kernels_gpu.py (checked there against torch's own conv in fp64)."""
    x, dy, dy_w, w3 = (t.to(torch.int64) for t in (case.x, case.dy, case.dy_w, case.w3))
    return ConvExpect(_conv3x3(x, w3) + case.b3.to(torch.int64), _conv3x3_dgrad(dy, w3), _conv3x3_wgrad(dy_w, x))


def unshuffle(dx, B, Hp, Wp, P):
    """NHWC [B, Hp*P, Wp*P, 64] -> token rows [B*Hp*Wp, P*P*64] (the inverse of the decoder's pixel shuffle)."""
    return dx.reshape(B, Hp, P, Wp, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B * Hp * Wp, P * P * C)


@functools.lru_cache(maxsize=None)
def conv_case(kind, B, Hi, Wi):
    case = conv_stamp_case(B, Hi, Wi) if kind == "stamp" else conv_int_case(B, Hi, Wi, 100 * Hi + Wi)
    return case, conv_reference(case)


def tail_reference(y3, gamma, beta, w1, b1, eps):
    """LayerNorm2D(64) . GELU . Conv1x1(64 -> 3) in fp64 on NHWC y3 -> NCHW pred."""
    return _tail(y3.double(), gamma.double(), beta.double(), w1.double(), b1.double(), eps)
