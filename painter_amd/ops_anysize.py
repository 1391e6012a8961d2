"""Tensor-level wrappers over include/painter_anysize.h and include/painter_anysize_grad.h: the attention forward and backward for any token
grid, the rel-pos table resize and its adjoint -- the kernels a run at an input size other than the constructed one needs beside those of
painter_amd/ops.py (csrc/attn_any.hip, csrc/attn_any_bwd.hip).
Same rules as ops.py: PyTorch only for device memory, the current stream and dtype tags."""
import torch

from ._lib import check, lib
from .ops import code, p, stream, workspace


def attn_fwd_takes(L, Hp, Wp):
    """Does pa_attn_fwd (ops.attn_fwd: the three kernel generations) accept this grid?  Its refusal, restated (include/painter_hip.h)."""
    return L == Hp * Wp and L % 32 == 0 and Hp % 4 == 0 and Wp % 4 == 0


def attn_any_fwd(qkv, rcat, batch, L, heads, Hp, Wp, scale):
    """qkv [batch*L, 3*heads*hd] T (row stride free), rcat T [NRP, hd] packed for (Hp, Wp) -> (out [batch*L, heads*hd] T,
    lse [batch*heads, L] f32), for any Hp, Wp >= 1.  attn_any_bwd is its backward (it needs out and lse, no tables)."""
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


def attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, batch, L, heads, Hp, Wp, scale, need_drcat=True, drcat=None):
    """The backward of attn_any_fwd, for any Hp, Wp >= 1: -> (dqkv T [batch*L, 3*heads*hd] in qkv's layout, drcat f32 [NRP, hd] =
    [d rel_pos_h ; d rel_pos_w ; 0] at the RUN-TIME lengths, or None with need_drcat=False: frozen tables, the contraction is not launched).
    rcat [NRP, hd] / rcatT [hd, NRP] T packed for (Hp, Wp); out, lse as attn_any_fwd returned them; row strides of qkv, out, dout free.
    Deterministic: no floating-point atomics."""
    T = qkv.dtype
    nrp, hd = rcat.shape
    assert qkv.is_cuda and qkv.stride(1) == 1 and qkv.shape == (batch * L, 3 * heads * hd), (qkv.shape, batch, L, heads, hd)
    assert rcat.dtype == T and rcat.is_contiguous() and nrp == lib.pa_relpos_rows_padded(Hp, Wp)
    assert rcatT.dtype == T and rcatT.is_contiguous() and rcatT.shape == (hd, nrp)
    for t in (out, dout):
        assert t.dtype == T and t.stride(1) == 1 and t.shape == (batch * L, heads * hd), (t.shape, t.dtype)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.shape == (batch * heads, L)
    nbytes = lib.pa_attn_any_bwd_workspace_bytes(code(T), batch, L, heads, Hp, Wp, hd)
    if nbytes <= 0:
        raise RuntimeError("painter_hip: pa_attn_any_bwd takes no %d x %d grid at head_dim %d (%s): its tables do not fit LDS" % (Hp, Wp, hd, T))
    ws = workspace(nbytes, qkv.device)
    # the kernels write dqkv at qkv's row pitch (as ops.attn_bwd_core): a contiguous tensor would be too small for a column-slice view of qkv
    dqkv = torch.empty((qkv.shape[0], qkv.stride(0)), dtype=T, device=qkv.device)[:, :qkv.shape[1]]
    if need_drcat and drcat is None:
        drcat = torch.empty((nrp, hd), dtype=torch.float32, device=qkv.device)
    assert not need_drcat or (drcat.shape == (nrp, hd) and drcat.dtype == torch.float32 and drcat.is_contiguous())
    check(lib.pa_attn_any_bwd(code(T), p(qkv), qkv.stride(0), p(rcat), p(rcatT), p(out), out.stride(0), p(dout), dout.stride(0), p(lse), p(dqkv),
                              p(drcat) if need_drcat else 0, p(ws), batch, L, heads, Hp, Wp, hd, float(scale), stream()), "pa_attn_any_bwd")
    return dqkv, (drcat if need_drcat else None)


def attn_any_bwd_launches():
    """Number of accepted pa_attn_any_bwd calls since process start (ops.attn_launch_counts() does not count them)."""
    return int(lib.pa_attn_any_bwd_launches())


def relpos_resize_bwd(drcat, src_h, src_w, dst_h, dst_w, out=None):
    """The adjoint of relpos_resize for one block: drcat f32 [>= dst_h + dst_w, hd] (attn_any_bwd's table gradient at the run-time
    lengths) -> f32 [rows, hd] = [d rel_pos_h at src_h ; d rel_pos_w at src_w ; 0], the gradient at the STORED lengths.  rows is out's
    (a block's flat gradient buffer: pa_relpos_rows_padded of the constructed grid), src_h + src_w without one.  A length that stays is
    copied bit for bit.  Deterministic: a gather in ascending order, no atomics."""
    hd = drcat.shape[1]
    assert drcat.is_cuda and drcat.dtype == torch.float32 and drcat.is_contiguous() and drcat.shape[0] >= dst_h + dst_w
    if out is None:
        out = torch.empty((src_h + src_w, hd), dtype=torch.float32, device=drcat.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[1] == hd and out.shape[0] >= src_h + src_w
    check(lib.pa_relpos_resize_bwd(p(drcat), p(out), out.shape[0], src_h, src_w, dst_h, dst_w, hd, stream()), "pa_relpos_resize_bwd")
    return out
