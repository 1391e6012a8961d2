"""Tensor-level wrappers over include/painter_anysize.h: the attention forward for any token grid and the rel-pos table resize, the two
kernels a forward at a run-time input size other than the constructed one needs beside those of painter_amd/ops.py (csrc/attn_any.hip).
Same rules as ops.py: PyTorch only for device memory, the current stream and dtype tags."""
import torch

from ._lib import check, lib
from .ops import code, p, stream


def attn_fwd_takes(L, Hp, Wp):
    """Does pa_attn_fwd (ops.attn_fwd: the three kernel generations) accept this grid?  Its refusal, restated (include/painter_hip.h)."""
    return L == Hp * Wp and L % 32 == 0 and Hp % 4 == 0 and Wp % 4 == 0


def attn_any_fwd(qkv, rcat, batch, L, heads, Hp, Wp, scale):
    """qkv [batch*L, 3*heads*hd] T (row stride free), rcat T [NRP, hd] packed for (Hp, Wp) -> (out [batch*L, heads*hd] T,
    lse [batch*heads, L] f32), for any Hp, Wp >= 1.  Forward only: no tables for a backward."""
    T = qkv.dtype
    hd = rcat.shape[1]
    assert qkv.is_cuda and qkv.stride(1) == 1 and qkv.shape == (batch * L, 3 * heads * hd), (qkv.shape, batch, L, heads, hd)
    assert rcat.dtype == T and rcat.is_contiguous() and rcat.shape[0] == lib.pa_relpos_rows_padded(Hp, Wp)
    out = torch.empty((batch * L, heads * hd), dtype=T, device=qkv.device)
    lse = torch.empty((batch * heads, L), dtype=torch.float32, device=qkv.device)
    check(lib.pa_attn_any_fwd(code(T), p(qkv), qkv.stride(0), p(rcat), p(out), out.stride(0), p(lse), batch, L, heads, Hp, Wp, hd,
                              float(scale), stream()), "pa_attn_any_fwd")
    return out, lse


def attn_any_launches():
    """Number of pa_attn_any_fwd launches since process start (ops.attn_launch_counts() does not count them)."""
    return int(lib.pa_attn_any_launches())


def relpos_resize(tabs, nblocks, src_h, src_w, dst_h, dst_w, hd, out=None):
    """Every block's rel-pos tables at the lengths (dst_h, dst_w) = (2Hp - 1, 2Wp - 1) of a run-time grid, in one launch:
    F.interpolate(mode="linear", align_corners=False) along the length, fp32.  tabs: int64 device tensor of 2 * nblocks addresses (what
    ops.relpos_pack_batch takes: rel_pos_h [src_h, hd] of every block, then rel_pos_w [src_w, hd] of every block).
    -> f32 [nblocks, dst_h + dst_w, hd] (block b: its rel_pos_h rows, then its rel_pos_w rows), or None -- and no launch -- when both
    lengths stay: the stored tables are the operands then."""
    assert tabs.dtype == torch.int64 and tabs.numel() == 2 * nblocks and tabs.is_cuda and tabs.is_contiguous()
    if (src_h, src_w) == (dst_h, dst_w):
        return None
    if out is None:
        out = torch.empty((nblocks, dst_h + dst_w, hd), dtype=torch.float32, device=tabs.device)
    assert out.shape == (nblocks, dst_h + dst_w, hd) and out.dtype == torch.float32 and out.is_contiguous()
    check(lib.pa_relpos_resize(p(tabs), p(out), nblocks, src_h, src_w, dst_h, dst_w, hd, stream()), "pa_relpos_resize")
    return out


def table_addresses(resized, dst_h):
    """-> int64 device tensor of 2 * nblocks addresses into relpos_resize's result, in ops.relpos_pack_batch's order: rel_pos_h of every
    block, then rel_pos_w of every block."""
    nblocks, rows, hd = resized.shape
    assert resized.dtype == torch.float32 and resized.is_contiguous()
    base, step = resized.data_ptr(), rows * hd * 4
    return torch.tensor([base + b * step for b in range(nblocks)] + [base + b * step + dst_h * hd * 4 for b in range(nblocks)],
                        dtype=torch.int64).to(resized.device)
