"""Forward / backward orchestration of the Painter / SegGPT ViT hot path over the C ABI.

This is the host-side mirror of Painter.forward_encoder / forward_decoder / forward_loss
(Painter/models_painter.py:385-472) and SegGPT's variants (SegGPT/SegGPT_inference/models_seggpt.py:391-479):
the control flow, buffer ownership and kernel order live here; every FLOP happens in libpainter_hip.so.
Backward is written by hand -- nothing is delegated to torch autograd or ATen.

Data layout in HBM (per rank):
  residual stream x        fp32 [B'*L, D]           B' = 2B for blocks 0..merge_idx, B afterwards
  GEMM operands / acts     T    (bf16 or fp32)      ln out [R,D], qkv [R,3D], attn out [R,D], fc1 act [R,4D] (+ gelu aux: fp32 pre-activation, or the 8-bit gelu' code)
  tap concat               T    [B*L, 4D]           LayerNorm of the 4 taps written straight into column slices
  decoder image            T    NHWC [B, H, W, 64]  pixel shuffle fused into decoder_embed's epilogue
  pred / loss              fp32 NCHW [B,3,H,W], [2]
"""
import os
from typing import NamedTuple

import torch

from . import hostmath, ops, ops_anysize
from ._lib import EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_RESID, KNOB_RELPOS_SPLITS, KNOB_WGRAD_TARGET


_SIDE_STREAM = os.environ.get("PAINTER_AMD_SIDE_STREAM", "1") != "0"
_DBG_SERIAL = os.environ.get("PAINTER_AMD_DEBUG_SERIAL", "0") == "1"   # diagnostics: serialise the two streams of the backward (no concurrency)
_DBG_TRACE = os.environ.get("PAINTER_AMD_DEBUG_TRACE", "0") == "1"     # checksums of the backward's intermediates -> HotPath.trace
_configured = False
# sizing of the parameter-gradient kernels when they run on the side stream, beside the data-gradient chain (0 = stand-alone sizing)
WGRAD_SIDE_TARGET = 96       # round 5 re-sweep on the lighter side stream (tools/step_knob_ab.py, profiles/r05_wgrad_side_target_sweep.log): 96 -> 53.08, 128 -> 53.42, 160 -> 54.09, 192 -> 54.47 ms/step
RELPOS_SIDE_SPLITS = 8


def _configure_library():
    """Process-wide tuning knobs of libpainter_hip.so, set ONCE from the environment (they are globals of the library: setting them per
    module instance would let the last constructed model decide for every model of the process)."""
    global _configured
    if _configured:
        return
    from ._lib import lib
    lib.pa_debug_set(KNOB_RELPOS_SPLITS, RELPOS_SIDE_SPLITS if _SIDE_STREAM else 0)       # K splits of the rel-pos table-gradient GEMM beside the main chain: round 2: 16 -> 54.54, 4 -> 54.35, 2 -> 55.0 ms/step; round 3 (tools/knob_sweep.py): 2 -> 56.18, 4 -> 55.10, 8 -> 54.89
    lib.pa_debug_set(KNOB_WGRAD_TARGET, WGRAD_SIDE_TARGET if _SIDE_STREAM else 0)     # wgrad GEMM workgroup target (gemm.hip: wgrad_fast_splits); round-2 sweep: 64 -> 59.7, 96 -> 57.7, 128 -> 57.7, 192 -> 58.9, 256 -> 59.2 ms/step
    _configured = True


class HotPathConfig:
    def __init__(self, img_size, patch_size, embed_dim, depth, num_heads, mlp_ratio, decoder_embed_dim,
                 pretrain_img_size, pretrain_use_cls_token, use_rel_pos, ln_eps, loss_func, seggpt, drop_path_rate, taps=None):
        self.H, self.W = img_size
        self.P = patch_size
        self.D = embed_dim
        self.depth = depth
        self.heads = num_heads
        self.hidden = int(embed_dim * mlp_ratio)
        self.dec = decoder_embed_dim
        self.Hp, self.Wp = self.H // patch_size, self.W // patch_size
        self.L = self.Hp * self.Wp
        self.src = pretrain_img_size // patch_size
        self.cls = 1 if pretrain_use_cls_token else 0
        self.use_rel_pos = use_rel_pos
        self.ln_eps = ln_eps
        self.loss_func = loss_func
        self.seggpt = seggpt
        self.merge_idx = 2                                   # models_painter.py:408
        # models_painter.py:416 hard-codes [5, 11, 17, 23]; another schedule has to be asked for explicitly (Painter(feature_taps=...))
        self.taps = [5, 11, 17, 23] if taps is None else [int(t) for t in taps]
        self.dpr = hostmath.drop_path_rates(drop_path_rate, depth)
        self.scale = (embed_dim // num_heads) ** -0.5
        self.check()

    def check(self):
        """The HIP path's structural requirements (fail loudly, there is no fallback)."""
        hd = self.D // self.heads
        err = []
        if hd not in (64, 80) or hd * self.heads != self.D:
            err.append("head_dim must be 64 (the reference factories) or 80 (ViT-H/14, BASELINE configs[4]); got %d" % hd)
        if self.dec != 64: err.append("decoder_embed_dim must be 64 (got %d)" % self.dec)
        if self.L % 32 or self.Hp % 4 or self.Wp % 4: err.append("token grid %dx%d must have Hp,Wp %% 4 == 0 and L %% 32 == 0" % (self.Hp, self.Wp))
        if self.H % self.P or self.W % self.P or self.W % 4: err.append("image %dx%d must be a whole number of %d-pixel patches, width a multiple of 4" % (self.H, self.W, self.P))
        if self.D % 8 or self.hidden % 8: err.append("embed/hidden dims must be multiples of 8")
        if not self.use_rel_pos: err.append("use_rel_pos=False is not built (the reference factories always enable it)")
        if self.H != 2 * self.W: err.append("img_size must be (2W, W) (patchify asserts H == 2W, models_painter.py:361)")
        if self.merge_idx >= self.depth or len(set(self.taps)) != 4 or sorted(self.taps) != self.taps or self.taps[-1] != self.depth - 1:
            err.append("depth %d is incompatible with the feature taps %s (four increasing blocks, the last one the last block; the reference's "
                       "hard-coded [5, 11, 17, 23] only fits depth 24 -- pass feature_taps=..., e.g. depth/4*k - 1)" % (self.depth, self.taps))
        if self.merge_idx in self.taps or min(self.taps) < self.merge_idx:
            # the backward handles a block that is a feature tap OR the stream merge, and taps are taken on the merged stream
            err.append("depth %d puts a feature tap at or before the stream merge (block %d)" % (self.depth, self.merge_idx))
        if err:
            raise NotImplementedError("painter_amd HIP path: " + "; ".join(err))


class _Grid:
    """The configuration at a run-time input size other than the constructed one (HotPath.grid): every field of the HotPathConfig it was
    derived from, with H, W, Hp, Wp, L of the run.  The backward reads the grid of its forward from _Saved.grid."""

    def __init__(self, cfg, H, W):
        self.__dict__.update(cfg.__dict__)
        self.H, self.W = int(H), int(W)
        self.Hp, self.Wp = self.H // cfg.P, self.W // cfg.P
        self.L = self.Hp * self.Wp
        self.attn_any = not ops_anysize.attn_fwd_takes(self.L, self.Hp, self.Wp)     # a grid such as 16 x 8 changes only the tables
        self.M = None              # per device: the sparse rows of abs_pos_operator(src, Hp, Wp) and of its transpose
        self.rel = {}              # the resized, packed rel-pos tables (HotPath.relpos_grid)


class _Saved:
    pass


class _Block(NamedTuple):
    """What one block's forward keeps for its backward (S.blocks[i]; the backward drops the entry as it consumes it)."""
    x: torch.Tensor            # the block's input (fp32 residual stream)
    mean1: torch.Tensor
    rstd1: torch.Tensor
    ln1: torch.Tensor
    qkv: torch.Tensor
    rcat: torch.Tensor
    ao: torch.Tensor           # attention output, the operand of proj
    lse: torch.Tensor
    x1: torch.Tensor           # residual stream after the attention branch
    mean2: torch.Tensor
    rstd2: torch.Tensor
    ln2: torch.Tensor
    gaux: torch.Tensor         # ops.linear_gelu's second result
    act: torch.Tensor
    Bc: int                    # samples in the stream at this block (2B up to the merge, B afterwards)
    atab: torch.Tensor         # ops.attn_fwd's tables (None where the kernels in use export none)
    group: int                 # SegGPT ensemble group size, 0 = no ensemble in this block


class _Tap(NamedTuple):
    """A feature tap's saved LayerNorm input and statistics (S.taps[k])."""
    x: torch.Tensor
    mean: torch.Tensor
    rstd: torch.Tensor


class _Streams:
    """The two HIP streams of one backward.  The data-gradient chain runs on `main`, the caller's stream; parameter gradients, which nothing
    downstream in the backward consumes, go to `side` (None: everything runs inline).  The rule between them, carried here once: the side
    stream waits for main before each piece of work; every main-stream tensor that work reads is recorded against the side stream, so that
    the allocator does not hand its memory out again before the side stream is done with it; PAINTER_AMD_DEBUG_SERIAL joins main behind
    every piece (no concurrency: diagnostics)."""
    __slots__ = ("main", "side")

    def __init__(self, main, side):
        self.main, self.side = main, side

    def run(self, fn, *reads):
        """-> fn(), a parameter-gradient computation that reads the main-stream tensors `reads` (None entries are ignored)."""
        if self.side is None:
            return fn()
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            r = fn()
        for t in reads:
            if t is not None:
                t.record_stream(self.side)
        if _DBG_SERIAL:
            self.main.wait_stream(self.side)
        return r

    def shared(self, t):
        """-> t, a main-stream allocation that work on the side stream reads or writes as well."""
        if self.side is not None:
            t.record_stream(self.side)
        return t

    def private(self, t):
        """-> a buffer the main stream may overwrite while the side stream may still read t: a new one, or t itself without a side stream."""
        return t if self.side is None else torch.empty_like(t)

    def ready(self, sync, G, names, flat=None):
        """Hand the bucket `names` of G to the GradSync (if any) behind both streams: its gradients come from both, and the exchange reads
        main-stream allocations (LayerNorm / rel-pos / tail gradients).  flat: one contiguous fp32 buffer that already holds every small
        gradient of `names` (they are views of it): it is exchanged as ONE message in place -- no flattening copy on the side stream."""
        if sync is not None:
            self.run(lambda: sync.ready(G, names, flat=flat), *[G[n] for n in names])

    def join(self, probe=None):
        """Order every gradient before whatever the caller enqueues next.  probe (tools/step_tail.py): two events, when each stream ran dry."""
        if self.side is not None:
            if probe is not None:
                probe[0].record(self.main)
                probe[1].record(self.side)
            self.main.wait_stream(self.side)


class _Backward:
    """The per-call context the parts of HotPath.backward share."""
    __slots__ = ("P", "S", "sync", "want", "st", "G", "flats", "rc_shape", "rel_shape", "dnorm")

    def __init__(self, P, S, sync, want, st):
        self.P, self.S, self.sync, self.want, self.st = P, S, sync, want, st
        self.G = {}
        self.flats = {}                                    # block -> its flat small-gradient buffer (HotPath.block_flat)
        self.rc_shape = tuple(S.blocks[-1].rcat.shape)     # Rcat [NRP, head_dim] of the forward's grid: the same for every block
        # the rel-pos gradient slot of a block's flat buffer: [NRP, head_dim] at the STORED table lengths (the constructed grid's)
        self.rel_shape = self.rc_shape
        if isinstance(S.grid, _Grid):
            sh, sw = P["blocks.0.attn.rel_pos_h"].shape[0], P["blocks.0.attn.rel_pos_w"].shape[0]
            self.rel_shape = (ops.lib.pa_relpos_rows_padded((sh + 1) // 2, (sw + 1) // 2), self.rc_shape[1])
        self.dnorm = None                                  # the four taps' accumulated d(norm.weight, norm.bias)

    def need(self, n):
        return self.want is None or n in self.want

    def param_grads(self, wname, bname, dy, x, bout=None, wgrad=None, colsum=None):
        """G[wname] = dy^T.x and G[bname] = colsum(dy) (into `bout`, a slice of the block's flat small-gradient buffer, when given), as far as
        they are wanted: a frozen parameter (outside `want`) costs nothing, and a bias that is already in G was summed by the kernel that
        produced dy (fc2 / proj: the LayerNorm backward; fc1: the fc2 data-gradient GEMM's epilogue).
        wgrad(dy, x) / colsum(dy, out=): the two computations, ops.linear_wgrad / ops.colsum unless given (the decoder's live-row route)."""
        G = self.G
        do_w, do_b = self.need(wname), bname not in G and self.need(bname)
        if not (do_w or do_b):
            return

        def fn():
            if do_w:
                G[wname] = (wgrad or ops.linear_wgrad)(dy, x)
            if do_b:
                G[bname] = (colsum or ops.colsum)(dy, out=bout)
        self.st.run(fn, dy, x if do_w else None)

    def ready(self, names, flat=None):
        self.st.ready(self.sync, self.G, names, flat=flat)


class HotPath:
    """Owns the per-module device constants and runs forward / backward."""

    def __init__(self, cfg: HotPathConfig, compute_dtype):
        self.cfg = cfg
        self.T = compute_dtype
        self._M = None
        self._wcache = {}
        self._pcache = {}
        self._rcache = {}
        self._grids = {}               # (H, W) -> _Grid: per-grid state of forwards at other sizes than the constructed one
        self._side = {}
        self._lnws = {}                # per device: ring of workspaces for the deferred LayerNorm-backward reductions (ln_workspace)
        # parameter-gradient kernels (dW = dY^T.X, bias column sums) are off the backward's critical path: they go to a second HIP
        # stream (+3.5 % at B=8; PAINTER_AMD_SIDE_STREAM=0 turns it off).  This mode exposed two things, both fixed: a cross-stream
        # allocator hazard on the gradient buckets, and SLP-packed fp32 VALU code mis-computing beside another kernel's MFMA
        # workgroups (build.py: -fno-slp-vectorize); DESIGN.md section 6.
        self.use_side_stream = _SIDE_STREAM
        self.grad_any_size = False     # the backward at another size than the constructed one is refused unless switched on
        _configure_library()

    def side_stream(self, device):
        s = self._side.get(device)
        if s is None:
            s = self._side[device] = torch.cuda.Stream(device=device)
        return s

    LN_RING = 6

    def ln_workspace(self, dev, nbytes, main, side):
        """A workspace for one deferred LayerNorm-backward reduction (ops.layernorm_bwd(defer=True, ws=...)), from a ring of LN_RING
        buffers per device that is reused across blocks and steps -- every call used to allocate 12.6 MB that the allocator could not
        hand out again before the side stream had caught up (up to ~0.6 GB of extra cached memory per step when it lagged).  Ordering:
        the main-stream kernel that refills a buffer waits for the event recorded behind the side-stream reduction that last read it
        (six launches earlier: practically never a stall).  -> (buffer, done) -- call done() after enqueueing the reduction."""
        ring = self._lnws.setdefault(dev, {"bufs": [None] * self.LN_RING, "events": [None] * self.LN_RING, "i": 0})
        k = ring["i"] % self.LN_RING
        ring["i"] += 1
        buf = ring["bufs"][k]
        if buf is None or buf.numel() < nbytes:
            if buf is not None and side is not None:
                buf.record_stream(side)            # the replaced buffer may still be read by a reduction in flight
            buf = ring["bufs"][k] = torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)
        ev = ring["events"][k]
        if ev is not None and side is not None:
            main.wait_event(ev)

        def done():
            if side is not None:
                e = ring["events"][k] or torch.cuda.Event()
                e.record(side)
                ring["events"][k] = e
        return buf, done

    # ------------------------------------------------------------------ run-time input sizes
    def grid(self, H, W):
        """-> the configuration a forward at H x W runs with: self.cfg itself at the constructed size (today's route, nothing derived),
        otherwise a _Grid, cached per size -- token grid, position-operator rows and the resized, packed rel-pos tables; a few sizes used
        alternately each keep their own.  What remains required of another size: H == 2W and both whole numbers of patches
        (NotImplementedError before anything is launched).  The constructed size's "width a multiple of 4" follows from that where a
        forward kernel needs it -- the patch embedding reads 8-pixel groups of a patch row only when P % 8 == 0, pixel by pixel otherwise
        (patch 14 at 140 x 70) -- and the loss, the decoder tail and patchify address single pixels.  A forward that saves for a backward
        at another size needs the switch grad_any_size."""
        c = self.cfg
        H, W = int(H), int(W)
        if (H, W) == (c.H, c.W):
            return c
        g = self._grids.get((H, W))
        if g is None:
            err = []
            if H != 2 * W: err.append("the stitched pair must be (2W, W)")
            if H < c.P or W < c.P or H % c.P or W % c.P: err.append("both sides must be whole numbers of %d-pixel patches" % c.P)
            if err:
                raise NotImplementedError("painter_amd HIP path: input size %d x %d (constructed at %d x %d): %s" % (H, W, c.H, c.W, "; ".join(err)))
            g = self._grids[(H, W)] = _Grid(c, H, W)
        return g

    def grid_pos_operator(self, g, device):
        """-> (sparse rows of M, sparse rows of M^T) of abs_pos_operator(src, Hp, Wp) for a run-time grid, cached on the grid: the bicubic
        resize of the position grid and its transpose, through which pos_embed gets its gradient."""
        if g.M is None or g.M[0][0].device != device:
            M = hostmath.abs_pos_operator(g.src, g.Hp, g.Wp)
            dev = lambda t: (torch.from_numpy(t[0]).to(device), torch.from_numpy(t[1]).to(device))
            g.M = (dev(hostmath.sparse_rows(M)), dev(hostmath.sparse_rows(M.T)))
        return g.M

    def relpos_grid(self, g, pre, P, transposed=False):
        """Rcat (or Rcat^T, for the backward) of block `pre` for the run-time grid g: every block's tables are resized to 2Hp - 1 / 2Wp - 1 rows by ONE launch
        (pa_relpos_resize: the reference's get_rel_pos, F.interpolate(mode="linear")) into a buffer that pa_relpos_pack_batch then packs
        for the grid -- two launches per (grid, table version), none afterwards.  Cached like relpos(), on the grid: keyed on the tables'
        addresses and versions, so two sizes used alternately each keep their tables."""
        c = self.cfg
        i = int(pre.split(".")[1])
        rh, rw = P[pre + "attn.rel_pos_h"], P[pre + "attn.rel_pos_w"]
        st = g.rel
        if st and st["dev"] == rh.device and st["T"] == self.T and st["ptr"][i] == (rh.data_ptr(), rw.data_ptr()) and \
                st["ver"][i] == (rh._version, rw._version):
            return (st["rcatT"] if transposed else st["rcat"])[i]
        hs = [P["blocks.%d.attn.rel_pos_h" % k] for k in range(c.depth)]
        ws = [P["blocks.%d.attn.rel_pos_w" % k] for k in range(c.depth)]
        hd, sh, sw = rh.shape[1], rh.shape[0], rw.shape[0]
        for t, n in [(t, sh) for t in hs] + [(t, sw) for t in ws]:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == rh.device and t.shape == (n, hd)
        ptr = [(h.data_ptr(), w.data_ptr()) for h, w in zip(hs, ws)]
        same = bool(st) and st["dev"] == rh.device and st["T"] == self.T and st["ptr"] == ptr
        tabs = st["tabs"] if same else torch.tensor([q[0] for q in ptr] + [q[1] for q in ptr], dtype=torch.int64).to(rh.device)
        dh, dw = 2 * g.Hp - 1, 2 * g.Wp - 1
        resized = ops_anysize.relpos_resize(tabs, c.depth, sh, sw, dh, dw, hd, out=st["resized"] if same else None)
        if resized is None:                       # both lengths stay: the stored tables are the operands
            addr = tabs
        else:
            addr = st["addr"] if same else ops_anysize.table_addresses(resized, dh)
        rcat, rcatT = ops.relpos_pack_batch(addr, c.depth, g.Hp, g.Wp, hd, self.T, rcat=st["rcat"] if same else None,
                                            rcatT=st["rcatT"] if same else None)
        st.clear()
        st.update(dev=rh.device, T=self.T, ptr=ptr, ver=[(h._version, w._version) for h, w in zip(hs, ws)], tabs=tabs, resized=resized,
                  addr=addr, rcat=rcat, rcatT=rcatT)
        return (rcatT if transposed else rcat)[i]

    # ------------------------------------------------------------------ constants / casts
    def pos_operator(self, device):
        """-> (sparse rows of M, sparse rows of M^T) on the device: the constant bicubic resize of the pre-training position grid."""
        if self._M is None or self._M[0][0].device != device:
            c = self.cfg
            M = hostmath.abs_pos_operator(c.src, c.Hp, c.Wp)
            fwd, bwd = hostmath.sparse_rows(M), hostmath.sparse_rows(M.T)
            dev = lambda t: (torch.from_numpy(t[0]).to(device), torch.from_numpy(t[1]).to(device))
            self._M = (dev(fwd), dev(bwd))
        return self._M

    def w(self, name, P):
        """T-typed copy of a weight matrix (K9: cast once per optimizer step, keyed on the tensor version)."""
        t = P[name]
        if self.T == torch.float32:
            return t.reshape(t.shape[0], -1)
        key = (name, t.data_ptr())
        ent = self._wcache.get(key)
        if ent is None or ent[0] != t._version or ent[1].device != t.device:
            buf = ent[1] if ent is not None and ent[1].device == t.device else torch.empty((t.shape[0], t.numel() // t.shape[0]), dtype=self.T, device=t.device)
            ops.cast_bf16(t, buf)
            self._wcache[key] = (t._version, buf)
            return buf
        return ent[1]

    def w_patch(self, P):
        """The patch-embed conv weight as the T [D, Kp] operand pa_patch_embed_fwd takes (Kp = 3*P*P rounded up to 8, zero padded).
        For P % 8 == 0 that is the ordinary T copy; otherwise (P = 14) a packed copy, cached on the parameter version like w()."""
        c = self.cfg
        if c.P % 8 == 0:
            return self.w("patch_embed.proj.weight", P)
        t = P["patch_embed.proj.weight"]
        key = ("patch_embed.proj.weight#packed", t.data_ptr())
        ent = self._pcache.get(key)
        if ent is None or ent[0] != t._version or ent[1].device != t.device:
            buf = ops.patch_weight_pack(t, self.T, c.P, out=ent[1] if ent is not None and ent[1].device == t.device else None)
            self._pcache = {key: (t._version, buf)}
            return buf
        return ent[1]

    def relpos(self, pre, P, transposed):
        """Rcat / Rcat^T operand of block `pre`.  Every block's pair is packed by ONE launch (pa_relpos_pack_batch, round 6) whenever the
        version of the asked-for block's tables has moved -- i.e. once per optimizer step in plain training (rounds 1 - 5: one launch per
        block and orientation, 48 per step; cached per parameter version since round 4, which only helped loops that leave the parameters
        alone: forward + backward timing, evaluation, accumulation micro-steps).  Keyed on addresses and tensor versions like every cache
        here: a write that bumps no version (p.data.copy_, an in-place collective) needs HotPath.invalidate().  The first call (and any call after
        the tables moved in memory) uploads the 2 * depth addresses: run one eager forward before capturing a hipGraph, as every caller here does."""
        c = self.cfg
        i = int(pre.split(".")[1])
        rh, rw = P[pre + "attn.rel_pos_h"], P[pre + "attn.rel_pos_w"]
        st = self._rcache
        if st and st["dev"] == rh.device and st["ptr"][i] == (rh.data_ptr(), rw.data_ptr()) and st["ver"][i] == (rh._version, rw._version):
            return (st["rcatT"] if transposed else st["rcat"])[i]
        hs = [P["blocks.%d.attn.rel_pos_h" % k] for k in range(c.depth)]
        ws = [P["blocks.%d.attn.rel_pos_w" % k] for k in range(c.depth)]
        hd = rh.shape[1]
        for t in hs + ws:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == rh.device and t.shape[1] == hd
        ptr = [(h.data_ptr(), w.data_ptr()) for h, w in zip(hs, ws)]
        same = bool(st) and st["dev"] == rh.device and st["ptr"] == ptr
        tabs = st["tabs"] if same else torch.tensor([q[0] for q in ptr] + [q[1] for q in ptr], dtype=torch.int64).to(rh.device)
        rcat, rcatT = ops.relpos_pack_batch(tabs, c.depth, c.Hp, c.Wp, hd, self.T, rcat=st["rcat"] if same else None, rcatT=st["rcatT"] if same else None)
        st.clear()
        st.update(dev=rh.device, ptr=ptr, ver=[(h._version, w._version) for h, w in zip(hs, ws)], tabs=tabs, rcat=rcat, rcatT=rcatT)
        return (rcatT if transposed else rcat)[i]

    def relpos_stale(self):
        """Mark the packed rel-pos tables stale, as an optimizer update of the tables does through their version counters (buffers and the
        address table stay): bench.py calls it before every timed step so that forward + backward is timed as training runs it."""
        st = self._rcache
        if st:
            st["ver"] = [None] * len(st["ver"])

    def invalidate(self):
        """Drop every cached operand copy (bf16 weights, packed patch weight, Rcat / Rcat^T): call after writing parameters in a way
        that leaves their version counters alone."""
        self._wcache.clear()
        self._pcache.clear()
        self._rcache.clear()
        for g in self._grids.values():
            g.rel.clear()

    def shadow_buffers(self):
        """{parameter data_ptr: cached bf16 copy} -- lets painter_amd.optim.AdamW refresh the copies inside its update pass."""
        return {key[1]: ent[1] for key, ent in self._wcache.items()}

    def mark_fresh(self, params):
        """The optimizer has rewritten these parameters AND their bf16 copies: adopt the new versions."""
        by_ptr = {p.data_ptr(): p for p in params}
        for key, ent in list(self._wcache.items()):
            p = by_ptr.get(key[1])
            if p is not None:
                self._wcache[key] = (p._version, ent[1])

    # ------------------------------------------------------------------ forward
    def forward(self, P, imgs, tgts, mask_u8, valid, seg_type=None, merge_between_batch=-1, drop_scales=None, need_grad=True, want=None):
        """need_grad: save what a backward needs (any input, parameter or the prediction may need a gradient).  want: the parameter names
        whose gradients the backward will be asked for (None = all): tensors that only serve frozen parameters' gradients are not kept --
        the im2col operand (patch weight), the tap concat (decoder_embed.weight), decoder_embed's output (decoder_pred.0.weight)."""
        T = self.T
        c = self.grid(imgs.shape[2], imgs.shape[3])        # self.cfg at the constructed size; the per-grid state of another size otherwise
        other = c is not self.cfg
        if other and need_grad and not self.grad_any_size:
            raise NotImplementedError("painter_amd HIP path: input size %d x %d differs from the constructed %d x %d, which is forward only "
                                      "by default: call under torch.no_grad(), or switch the backward at any size on "
                                      "(model.grad_at_any_size(True) / HotPath.grad_any_size)" % (c.H, c.W, self.cfg.H, self.cfg.W))
        dev = imgs.device
        B = imgs.shape[0]
        L, D = c.L, c.D
        assert tuple(imgs.shape) == (B, 3, c.H, c.W) and tgts.shape == imgs.shape and mask_u8.shape[-1] == L, (imgs.shape, tgts.shape, mask_u8.shape)
        S = _Saved()
        S.B, S.need_grad = B, need_grad
        S.grid = c                                         # the backward runs on the grid of its forward
        keep = lambda n: need_grad and (want is None or n in want)
        S.imgs, S.tgts, S.mask, S.valid = imgs, tgts, mask_u8, valid
        S.drop = drop_scales
        S.seg_type = seg_type if c.seggpt else None
        pe = P["pos_embed"][0, c.cls:]
        pos = ops.pos_fwd((self.grid_pos_operator(c, dev) if other else self.pos_operator(dev))[0], pe, L, D)
        tok_args = (P["patch_embed.proj.bias"], P["mask_token"], P["segment_token_x"], P["segment_token_y"], pos, mask_u8,
                    P.get("type_token_cls") if c.seggpt else None, P.get("type_token_ins") if c.seggpt else None,
                    seg_type if c.seggpt else None)
        S.cols = None
        if ops.patch_cols_ok(T, B, L, c.P, D):           # bf16, P % 8 == 0: materialised im2col operand + the 256 x 256 GEMM (kept for the weight gradient)
            cols = ops.patch_im2col(imgs, tgts, B, c.Hp, c.Wp, c.P)
            x = ops.patch_embed_fwd_cols(cols, self.w_patch(P), *tok_args, B, L, D)
            if keep("patch_embed.proj.weight"):
                S.cols = cols
        else:
            x = ops.patch_embed_fwd(T, imgs, tgts, self.w_patch(P), *tok_args, B, c.Hp, c.Wp, c.P, D)
        concat = torch.empty((B * L, 4 * D), dtype=T, device=dev)
        S.blocks, S.taps = [], []
        Bc = 2 * B
        for i in range(c.depth):
            pre = "blocks.%d." % i
            R = Bc * L
            merge = 0
            if c.seggpt and merge_between_batch >= 0 and i >= merge_between_batch:
                merge = 1 if c.merge_idx >= i else 2
            ds_a, ds_m = (None, None) if drop_scales is None else drop_scales[i]
            # DropPath skipping: a sample whose factor is 0 gets 0 * (branch) added to its residual, so the kernels of the branch do not compute
            # it (they read the factor vector themselves: no host synchronisation).  Not for the attention branch of an ensemble block: there a
            # dropped sample's proj output still enters the other samples' group mean.
            sk_a = None if merge > 0 else ds_a
            ln1, mean1, rstd1 = ops.layernorm_fwd(x, P[pre + "norm1.weight"], P[pre + "norm1.bias"], c.ln_eps, T)
            qkv = ops.linear_fwd(ln1, self.w(pre + "attn.qkv.weight", P), P[pre + "attn.qkv.bias"], EPI_BIAS, rowskip=sk_a, skip_rows_per_sample=L)
            rcat = self.relpos_grid(c, pre, P) if other else self.relpos(pre, P, False)
            if other and c.attn_any:       # a grid pa_attn_fwd refuses (70 x 35): the any-grid forward; a dropped sample is computed, its factor is 0
                ao, lse, atab = ops_anysize.attn_any_fwd(qkv, rcat, Bc, L, c.heads, c.Hp, c.Wp, c.scale) + (None,)
            else:
                ao, lse, atab = ops.attn_fwd(qkv, rcat, Bc, L, c.heads, c.Hp, c.Wp, c.scale, need_tables=True, rowskip=sk_a) if need_grad else \
                    ops.attn_fwd(qkv, rcat, Bc, L, c.heads, c.Hp, c.Wp, c.scale, rowskip=sk_a) + (None,)
            group = 0
            if merge > 0:
                # x1 = x0 + s_a * ens(proj(...)) (models_seggpt.py:207-238).  Differentiable like the reference's Block.forward: mean over
                # the group + broadcast is its own adjoint, the backward applies the same operator to the (DropPath-scaled) branch
                # gradient.  The reference itself only runs the ensemble under @torch.no_grad (seggpt_engine.py:26); with DropPath
                # factors (train mode) the scaled form is composed from the same kernels: ens alone, the row-scale kernel, a plain add
                # (= the ensemble kernel with groups of one).
                a = ops.linear_fwd(ao, self.w(pre + "attn.proj.weight", P), P[pre + "attn.proj.bias"], EPI_BIAS_F32)
                group = Bc // 2 if merge == 1 else Bc
                if ds_a is None:
                    x1 = ops.ensemble_resid(x, a, Bc, group, L, D)
                else:
                    e = ops.ensemble_resid(torch.zeros_like(x), a, Bc, group, L, D)
                    x1 = ops.ensemble_resid(x, ops.scale_cast(torch.float32, e, ds_a, L), Bc, 1, L, D)
                    del e
            else:
                x1 = ops.linear_fwd(ao, self.w(pre + "attn.proj.weight", P), P[pre + "attn.proj.bias"], EPI_BIAS_RESID,
                                    resid=x, rowscale=ds_a, rows_per_sample=L, rowskip=sk_a)
            ln2, mean2, rstd2 = ops.layernorm_fwd(x1, P[pre + "norm2.weight"], P[pre + "norm2.bias"], c.ln_eps, T)
            act, gaux = ops.linear_gelu(ln2, self.w(pre + "mlp.fc1.weight", P), P[pre + "mlp.fc1.bias"], need_aux=need_grad, rowskip=ds_m, rows_per_sample=L)
            x2 = ops.linear_fwd(act, self.w(pre + "mlp.fc2.weight", P), P[pre + "mlp.fc2.bias"], EPI_BIAS_RESID,
                                resid=x1, rowscale=ds_m, rows_per_sample=L, rowskip=ds_m)
            if need_grad:
                S.blocks.append(_Block(x, mean1, rstd1, ln1, qkv, rcat, ao, lse, x1, mean2, rstd2, ln2, gaux, act, Bc, atab, group))
            x = x2
            if i == c.merge_idx:
                Bc = B
                x = ops.merge_fwd(x, B * L, D)
            if i in c.taps:
                k = c.taps.index(i)
                _, mt, rt = ops.layernorm_fwd(x, P["norm.weight"], P["norm.bias"], c.ln_eps, T, out=concat[:, k * D:(k + 1) * D])
                if need_grad:
                    S.taps.append(_Tap(x, mt, rt))
        E = ops.linear_pixshuf(concat, self.w("decoder_embed.weight", P), P["decoder_embed.bias"], B, c.Hp, c.Wp, c.P, c.dec)
        w3r, wf = ops.conv3x3_pack(P["decoder_pred.0.weight"], T)
        w1 = P["decoder_pred.3.weight"].reshape(3, c.dec)
        pred, y3 = ops.decoder_tail_fwd(E, w3r, P["decoder_pred.0.bias"], P["decoder_pred.1.weight"], P["decoder_pred.1.bias"],
                                        w1, P["decoder_pred.3.bias"], 1e-6, save_y3=need_grad)
        loss_out = ops.loss_fwd(pred, tgts, valid, mask_u8, c.P, ignore_rule=not c.seggpt,
                                eps_den=0.0 if c.seggpt else 1e-2, kind=c.loss_func)
        pred_patch = ops.patchify(pred, c.Hp, c.Wp, c.P)
        if need_grad:
            S.y3, S.pred, S.loss_out, S.wf = y3, pred, loss_out, wf
            S.concat = concat if keep("decoder_embed.weight") else None
            S.E = E if keep("decoder_pred.0.weight") else None
        return loss_out, pred, pred_patch, S

    # ------------------------------------------------------------------ backward
    def backward(self, P, S, dloss, sync=None, want=None, want_imgs=False, want_tgts=False, dpatch=None):
        """-> {param name: fp32 grad}, or (that dict, d imgs, d tgts) when want_imgs / want_tgts is set (None where not asked for).
        dloss: 0-d / [1] fp32 device tensor (may carry a GradScaler factor), or None when the loss is not in the objective.
        sync: optional painter_amd.parallel.GradSync; buckets are handed over as soon as they are enqueued.
        want: the parameter names whose gradients are needed (None = all).  The others get no entry and none of their separable work runs:
        weight-gradient GEMMs + slab sums, the conv3x3 / patch-embed weight gradients, the rel-pos table reductions, the deferred LayerNorm
        parameter reductions and separate column sums.  Bias sums fused into data-gradient kernels (the LayerNorm backward's dxT_colsum,
        fc1's colsum_out) stay, so that the data-gradient chain runs the same kernels and gives the same bits.  With a GradSync every
        gradient is computed and exchanged (want is ignored).
        dpatch: f32 [B, L, P*P*3] gradient of the returned pred_patch, or None (then dpred is today's pa_loss_bwd).

        Two HIP streams (_Streams): the data-gradient chain (dgrad GEMMs, attention backward, LayerNorm backward) runs on the caller's
        stream; every parameter gradient (wgrad GEMM + slab reduction + column sum, the conv and rel-pos table gradients, the deferred
        LayerNorm reductions) is enqueued on a side stream behind it, because nothing downstream in the backward consumes it."""
        dev = S.imgs.device
        if sync is not None:
            want = None
        side = self.side_stream(dev) if self.use_side_stream and (want is None or len(want) > 0) else None
        X = _Backward(P, S, sync, want, _Streams(torch.cuda.current_stream(dev), side))
        self.trace = []
        dconcat, dpred_loss = self._backward_decoder(X, dloss, dpatch, want_tgts)
        dx = dyT_next = None
        for i in reversed(range(self.cfg.depth)):
            dx, dyT_next = self._backward_block(X, i, dconcat, dx, dyT_next)
        dimgs, dtgts = self._backward_tokens(X, dx, dpred_loss, want_imgs, want_tgts)
        del dpred_loss
        G = X.G
        if want is not None:
            G = {n: g for n, g in G.items() if g is not None and n in want}
        X.st.join(getattr(self, "tail_probe", None))       # every gradient is ordered before whatever the caller enqueues next
        if sync is not None:
            sync.finish()
        if want_imgs or want_tgts:
            return G, dimgs, dtgts
        return G

    def _tr(self, name, t):
        if _DBG_TRACE:
            self.trace.append((name, t.detach().double().abs().sum()))

    def _backward_decoder(self, X, dloss, dpatch, want_tgts):
        """Loss, decoder tail and decoder_embed -> (dconcat T [B*L, 4D], the loss's own term of dpred or None)."""
        c, T, P, S, G, st, need = X.S.grid, self.T, X.P, X.S, X.G, X.st, X.need
        B = S.B
        dpred_loss = None          # the loss's own term of dpred: its direct gradient w.r.t. tgts is -dpred_loss
        if dpatch is None:
            dpred = ops.loss_bwd(S.pred, S.tgts, S.valid, S.mask, dloss, S.loss_out, c.P, c.loss_func)
            if want_tgts:
                dpred_loss = dpred
        else:
            dpred, dpred_loss = ops.pred_bwd(S.pred, S.tgts, S.valid, S.mask, dloss, S.loss_out, dpatch, c.P, c.loss_func,
                                             want_loss_term=want_tgts and dloss is not None)
        w1 = P["decoder_pred.3.weight"].reshape(3, c.dec)
        dy3, tg = ops.decoder_tail_bwd_pointwise(dpred, S.y3, P["decoder_pred.1.weight"], P["decoder_pred.1.bias"], w1, 1e-6)
        G["decoder_pred.1.weight"] = tg[0:64]
        G["decoder_pred.1.bias"] = tg[64:128]
        G["decoder_pred.3.weight"] = tg[128:320].reshape(3, c.dec, 1, 1)
        G["decoder_pred.3.bias"] = tg[320:323]
        npix = B * c.H * c.W
        if need("decoder_pred.0.weight") or need("decoder_pred.0.bias"):
            G["decoder_pred.0.weight"], G["decoder_pred.0.bias"] = st.run(
                lambda: (ops.conv3x3_wgrad(dy3, S.E) if need("decoder_pred.0.weight") else None,
                         ops.colsum(dy3.view(npix, c.dec)) if need("decoder_pred.0.bias") else None), dy3, S.E)
        w_de = self.w("decoder_embed.weight", P)
        if dpatch is None and ops.decoder_live_ok(T, B, c.Hp, c.Wp, c.P, w_de.shape[1]):
            # The loss touches masked patches only: dE is exactly zero on every token without a masked patch in its 3 x 3 neighbourhood.  The
            # conv's data gradient writes the live rows compacted, both decoder_embed GEMMs and the bias sum run over those rows alone (their
            # number stays on the device), and the data gradient is scattered back into a dconcat whose dead rows are zero.
            # A gradient on pred_patch (dpatch) makes every row live: that case, the fp32 build and ragged shapes stay dense.
            rowmap, live, count = ops.live_rows(S.mask, B, c.Hp, c.Wp)
            st.shared(count)                       # (rowmap / live / count share one allocation; the side stream's GEMM and sums read it)
            dE = ops.conv3x3_dgrad_unshuffle_live(dy3, S.wf, rowmap, count, B, c.Hp, c.Wp, c.P)
            del dy3
            X.param_grads("decoder_embed.weight", "decoder_embed.bias", dE, S.concat,
                          wgrad=lambda dy, x: ops.linear_wgrad(dy, x, live=(live, count)),
                          colsum=lambda dy, out=None: ops.colsum_live(dy, count, out=out))
            dconcat = ops.linear_dgrad(dE, w_de, live=(live, rowmap, count))
            if _DBG_TRACE:
                self._tr("dE", dE[:int(count.item())])
        else:
            dE = ops.conv3x3_dgrad_unshuffle(dy3, S.wf, B, c.Hp, c.Wp, c.P)
            del dy3
            X.param_grads("decoder_embed.weight", "decoder_embed.bias", dE, S.concat)
            dconcat = ops.linear_dgrad(dE, w_de)
            self._tr("dE", dE)
        self._tr("dconcat", dconcat)
        del dE
        X.ready(["decoder_embed.weight", "decoder_embed.bias"])
        X.ready([n for n in G if n.startswith("decoder_pred.")])
        return dconcat, dpred_loss

    def block_flat(self, X, i):
        """(buffer, named views) of block i's small gradients (LayerNorm affine, the four biases, the rel-pos tables), which live in ONE flat
        buffer so that the gradient exchange sends them as one message without a flattening copy:
        [norm1 g,b | norm2 g,b | qkv.b | proj.b | fc1.b | fc2.b | d rcat].  Allocated on first use: block i + 1's norm1 backward already
        writes block i's fc2 bias gradient into it."""
        if i not in X.flats:
            D = self.cfg.D
            sizes = [2 * D, 2 * D, 3 * D, D, self.cfg.hidden, D, X.rel_shape[0] * X.rel_shape[1]]
            fb = X.st.shared(torch.empty((sum(sizes),), dtype=torch.float32, device=X.S.imgs.device))
            X.flats[i] = (fb, dict(zip(("n1", "n2", "qkv", "proj", "fc1", "fc2", "rel"), torch.split(fb, sizes))))
        return X.flats[i]

    def _backward_block(self, X, i, dconcat, dx, dyT_next):
        """Block i: (dx of its output -- None at the last block --, the dY of its fc2 when block i + 1's norm1 backward emitted it)
        -> (dx of its input, the dY of block i - 1's fc2 or None)."""
        c, T, P, S, G, st, need = X.S.grid, self.T, X.P, X.S, X.G, X.st, X.need
        other = c is not self.cfg                  # a backward at another size than the constructed one (grad_any_size)
        B, L, D = S.B, c.L, c.D
        dev = S.imgs.device
        tr = self._tr
        pre = "blocks.%d." % i
        b = S.blocks[i]
        S.blocks[i] = None
        R = b.Bc * L
        ds_a, ds_m = (None, None) if S.drop is None else S.drop[i]
        # DropPath skipping (see forward): the dY rows of a dropped sample are exact zeros (the LayerNorm backward / merge_bwd multiplied
        # them by the factor), so the branch's data-gradient kernels leave them out.  The ensemble mixes samples: no skipping there.
        sk_a = None if b.group > 0 else ds_a
        nrp, hd = X.rc_shape
        flat, fl = self.block_flat(X, i)
        del X.flats[i]
        # dyT = bf16(ds_m * dx) is emitted by the kernel that produces the final dx of this block's output: the tap
        # LayerNorm backward, block i+1's norm1 backward (dyT_next), or the stream-merge backward
        if i in c.taps:
            k = c.taps.index(i)
            tap = S.taps[k]
            dyT = torch.empty((R, D), dtype=T, device=dev)
            # (the LayerNorm backward kernels also sum the columns of the dxT they emit: dxT is the dY of fc2 / proj, so that
            # sum is the layer's bias gradient -- no separate pass over dxT)
            dx, gb = ops.layernorm_bwd(dconcat[:, k * D:(k + 1) * D], tap.x, tap.mean, tap.rstd, P["norm.weight"], dres=dx, dx=dx, dxT=dyT,
                                       rowscale=ds_m, rows_per_sample=L, dxT_colsum=fl["fc2"])
            G[pre + "mlp.fc2.bias"] = fl["fc2"]
            if need("norm.weight") or need("norm.bias"):
                X.dnorm = gb if X.dnorm is None else _add_(X.dnorm, gb)
        elif i == c.merge_idx:
            dx, dyT = ops.merge_bwd(T, dx, ds_m, L, B * L, D)
        else:
            dyT = dyT_next
        # ---- MLP branch: x2 = x1 + s_m * fc2(gelu(fc1(LN2(x1))))
        X.param_grads(pre + "mlp.fc2.weight", pre + "mlp.fc2.bias", dyT, b.act, fl["fc2"])
        tr("%d.dyT" % i, dyT)
        # (the GEMM's epilogue also sums the columns of the dpre it stores: fc1's bias gradient, no separate pass over [R, 4D])
        dpre = ops.linear_dgrad(dyT, self.w(pre + "mlp.fc2.weight", P), gelu_aux=b.gaux, colsum_out=fl["fc1"], rowskip=ds_m, rows_per_sample=L)
        G[pre + "mlp.fc1.bias"] = fl["fc1"]
        tr("%d.dpre" % i, dpre)
        X.param_grads(pre + "mlp.fc1.weight", pre + "mlp.fc1.bias", dpre, b.ln2, fl["fc1"])
        dln2 = ops.linear_dgrad(dpre, self.w(pre + "mlp.fc1.weight", P), rowskip=ds_m, rows_per_sample=L)
        tr("%d.dln2" % i, dln2)
        del dpre
        dyA = st.private(dyT)                      # dyT may still be read by the side stream: the attention branch's dY gets its own buffer
        # (the reduction of the LayerNorm parameter-gradient partials is a parameter gradient too: side stream)
        lnws, lndone = self.ln_workspace(dev, ops.layernorm_bwd_workspace_bytes(R, D), st.main, st.side)
        dx, fin = ops.layernorm_bwd(dln2, b.x1, b.mean2, b.rstd2, P[pre + "norm2.weight"], dres=dx, dx=dx, dxT=dyA,
                                    rowscale=ds_a, rows_per_sample=L, gb=fl["n2"].view(2, D), dxT_colsum=fl["proj"], defer=True, ws=lnws)
        gb = None
        if need(pre + "norm2.weight") or need(pre + "norm2.bias") or need(pre + "attn.proj.bias"):
            gb = st.run(fin)
            lndone()
            G[pre + "norm2.weight"], G[pre + "norm2.bias"] = gb[0], gb[1]
        G[pre + "attn.proj.bias"] = fl["proj"]
        del dyT
        tr("%d.dx_ln2" % i, dx); tr("%d.dyA" % i, dyA)
        if gb is not None:
            tr("%d.gb2" % i, gb)
        # ---- attention branch: x1 = x0 + s_a * proj(attn(LN1(x0)))
        if b.group > 0:
            # SegGPT feature ensemble (forward: x1 = x0 + s_a * ens(proj(...))): the branch gradient is ens applied to s_a * dx (fp32: the
            # kernel's own type), re-rounded to the operand type.  Column sums are unchanged by a mean + broadcast over samples, so
            # the proj bias gradient the LayerNorm backward already summed (of s_a * dx) stands.
            da = ops.ensemble_resid(torch.zeros_like(dx), dx if ds_a is None else ops.scale_cast(torch.float32, dx, ds_a, L), b.Bc, b.group, L, D)
            dyA = da if T == torch.float32 else ops.cast_bf16(da, out=dyA)
            del da
        X.param_grads(pre + "attn.proj.weight", pre + "attn.proj.bias", dyA, b.ao, fl["proj"])
        dao = ops.linear_dgrad(dyA, self.w(pre + "attn.proj.weight", P), out=dln2, rowskip=sk_a, rows_per_sample=L)
        tr("%d.dao" % i, dao)
        del dyA
        want_rel = need(pre + "attn.rel_pos_h") or need(pre + "attn.rel_pos_w")
        if other:
            # The tables of this run are the stored ones resized (relpos_grid): the attention backward gives their gradient at the run-time
            # lengths (scratch), pa_relpos_resize_bwd -- a parameter gradient: side stream -- carries it to the stored lengths, into the
            # block's flat buffer.  A grid pa_attn_bwd refuses goes through the any-grid backward, which computes a dropped sample too
            # (its dout rows are zeros); a grid such as 16 x 8 through the existing kernels.
            rcatT = self.relpos_grid(c, pre, P, transposed=True)
            dG = None
            if c.attn_any:
                dqkv, drun = ops_anysize.attn_any_bwd(b.qkv, b.rcat, rcatT, b.ao, dao, b.lse, b.Bc, L, c.heads, c.Hp, c.Wp, c.scale, need_drcat=want_rel)
            else:
                dqkv, dG = ops.attn_bwd_core(b.qkv, b.rcat, rcatT, b.ao, dao, b.lse, b.Bc, L, c.heads, c.Hp, c.Wp, c.scale, tables=b.atab, rowskip=sk_a)
            if want_rel:
                sh, sw = P[pre + "attn.rel_pos_h"].shape[0], P[pre + "attn.rel_pos_w"].shape[0]

                def table_grads():
                    d = drun if dG is None else ops.attn_bwd_relpos(dG, b.qkv, nrp, b.Bc, L, c.heads, c.Hp, c.Wp)
                    return ops_anysize.relpos_resize_bwd(d, sh, sw, 2 * c.Hp - 1, 2 * c.Wp - 1, out=fl["rel"].view(X.rel_shape))
                drcat = st.run(table_grads, dG, b.qkv, drun if dG is None else None)
                G[pre + "attn.rel_pos_h"] = drcat[:sh]
                G[pre + "attn.rel_pos_w"] = drcat[sh:sh + sw]
            del dG
        else:
            rcatT = self.relpos(pre, P, True)
            dqkv, dG = ops.attn_bwd_core(b.qkv, b.rcat, rcatT, b.ao, dao, b.lse, b.Bc, L, c.heads, c.Hp, c.Wp, c.scale, tables=b.atab, rowskip=sk_a)
            if want_rel:
                # (the dQ kernel still writes its rel-pos partials / dG when the tables are frozen: only this reduction is skipped)
                drcat = st.run(lambda: ops.attn_bwd_relpos(dG, b.qkv, nrp, b.Bc, L, c.heads, c.Hp, c.Wp, out=fl["rel"].view(nrp, hd)), dG, b.qkv)
                nh, nw = 2 * c.Hp - 1, 2 * c.Wp - 1
                G[pre + "attn.rel_pos_h"] = drcat[:nh]
                G[pre + "attn.rel_pos_w"] = drcat[nh:nh + nw]
            del dG
        tr("%d.dqkv" % i, dqkv)
        X.param_grads(pre + "attn.qkv.weight", pre + "attn.qkv.bias", dqkv, b.ln1, fl["qkv"])
        dln1 = ops.linear_dgrad(dqkv, self.w(pre + "attn.qkv.weight", P), out=dao, rowskip=sk_a, rows_per_sample=L)
        del dqkv
        nxt = i - 1
        if nxt >= 0 and nxt not in c.taps and nxt != c.merge_idx:
            dyT_next = torch.empty((R, D), dtype=T, device=dev)
        else:
            dyT_next = None
        ds_next = None if (S.drop is None or nxt < 0) else S.drop[nxt][1]
        cs_next = None
        if dyT_next is not None:               # dyT_next is block nxt's fc2 dY: its column sum goes into block nxt's flat buffer
            cs_next = self.block_flat(X, nxt)[1]["fc2"]
            G["blocks.%d.mlp.fc2.bias" % nxt] = cs_next
        lnws, lndone = self.ln_workspace(dev, ops.layernorm_bwd_workspace_bytes(R, D), st.main, st.side)
        dx, fin = ops.layernorm_bwd(dln1, b.x, b.mean1, b.rstd1, P[pre + "norm1.weight"], dres=dx, dx=dx, dxT=dyT_next,
                                    rowscale=ds_next if dyT_next is not None else None, rows_per_sample=L, gb=fl["n1"].view(2, D),
                                    dxT_colsum=cs_next, defer=True, ws=lnws)
        if need(pre + "norm1.weight") or need(pre + "norm1.bias") or (cs_next is not None and need("blocks.%d.mlp.fc2.bias" % nxt)):
            gb = st.run(fin)
            lndone()
            G[pre + "norm1.weight"], G[pre + "norm1.bias"] = gb[0], gb[1]
        tr("%d.dx_ln1" % i, dx)
        del b
        X.ready([n for n in G if n.startswith(pre)], flat=flat)
        return dx, dyT_next

    def _backward_tokens(self, X, dx, dpred_loss, want_imgs, want_tgts):
        """Token assembly + patch embedding (and the last gradient bucket) -> (d imgs, d tgts), None where not asked for."""
        c, T, P, S, G, need = X.S.grid, self.T, X.P, X.S, X.G, X.need
        B, L, D = S.B, c.L, c.D
        if X.dnorm is not None:
            G["norm.weight"], G["norm.bias"] = X.dnorm[0], X.dnorm[1]
        dpe, sums = ops.tokens_bwd(T, dx, S.mask, B, L, D)
        if need("patch_embed.proj.weight"):
            if S.cols is not None:
                G["patch_embed.proj.weight"] = ops.linear_wgrad(dpe, S.cols).view(D, 3, c.P, c.P)
            else:
                G["patch_embed.proj.weight"] = ops.patch_embed_wgrad(dpe, S.imgs, S.tgts, B, c.Hp, c.Wp, c.P, D).view(D, 3, c.P, c.P)
        if need("patch_embed.proj.bias"):
            G["patch_embed.proj.bias"] = ops.colsum(dpe)
        if need("pos_embed"):
            dposemb = torch.zeros_like(P["pos_embed"])
            opT = (self.grid_pos_operator(c, S.imgs.device) if c is not self.cfg else self.pos_operator(S.imgs.device))[1]
            ops.pos_bwd(opT, sums[0], sums[1], dposemb[0, c.cls:], c.src * c.src, D)
            G["pos_embed"] = dposemb
        for k_, nm in enumerate(("segment_token_x", "segment_token_y", "mask_token")):
            if need(nm):
                G[nm] = ops.colsum(sums[k_]).view(1, 1, 1, D)
        small_tail = []
        if c.seggpt and S.seg_type is not None and (need("type_token_cls") or need("type_token_ins")):
            # SegGPT's two segmentation-type tokens (models_seggpt.py:415-420: added to every token of both streams of the samples of their
            # type): gradient = sum of dx over those samples' rows -- per-sample row weights (1 where the type matches) through the
            # row-scale kernel, then a column sum.  Only reached when a SegGPT module is differentiated (the reference never does).
            # A token no sample of the batch uses gets NO gradient (None), as under the reference's autograd -- a weight-decaying optimizer
            # then leaves it alone instead of decaying it towards zero.  (One host read of the [B] type vector at the very end of the
            # backward.  With a gradient exchange installed every rank must take part in the same collectives, so zeros are produced
            # there: the reference's DDP wrapper would refuse the unused parameter outright.)
            types_present = set(S.seg_type.reshape(-1).tolist())
            for t_, nm in ((0.0, "type_token_cls"), (1.0, "type_token_ins")):
                if (t_ not in types_present and X.sync is None) or not need(nm):
                    continue
                w = (S.seg_type.reshape(-1) == t_).to(torch.float32)
                sel = ops.scale_cast(torch.float32, dx, torch.cat((w, w)).contiguous(), L)
                G[nm] = ops.colsum(sel).view(1, 1, 1, D)
                small_tail.append(nm)
        X.ready(["norm.weight", "norm.bias", "patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed",
                 "segment_token_x", "segment_token_y", "mask_token"] + small_tail)
        if not (want_imgs or want_tgts):
            return None, None
        # input gradients (pa_patch_embed_dgrad): d tgts also carries the loss's direct term, -dpred_loss
        return ops.patch_embed_dgrad(dpe, self.w_patch(P), B, c.Hp, c.Wp, c.P, D, want_imgs, want_tgts,
                                     addend=dpred_loss if want_tgts else None, alpha=-1.0)

def _add_(a, b):
    """a += b for two small fp32 device tensors through the slab reducer (keeps arithmetic inside the library)."""
    from ._lib import check, lib
    check(lib.pa_slab_reduce(b.data_ptr(), a.data_ptr(), a.numel(), 1, a.numel(), 1, ops.stream()), "pa_slab_reduce")
    return a
