"""Guard-band tests: every kernel-enqueuing function of painter_amd/ops.py stays inside the buffers the C ABI sizes.

Each case runs its ops twice on the same seeded operands:
  (a) the ordinary way -- contiguous operands, torch.empty outputs, the grow-only 1 MiB-floored ops.workspace();
  (b) under tests/guard_bands.guarded_ops -- every operand copied into, and every output, side output and scratch buffer allocated from,
      a byte buffer [4 MiB guard | payload | 4 MiB guard] pre-filled with 0xFF (NaN as bf16 / fp32), scratch at EXACTLY the bytes its
      pa_*_bytes helper returns, and every matrix that has an ld* argument in the C ABI a column slice of a wider payload.
and asserts that no guard or row-gap byte changed, that no float result of (b) still holds the poison, and that (b) is bit-identical to
(a).  The premise of the bit-identity is the one tests/test_engine_streams_gpu.py states: no kernel, split count or tile plan depends on
anything but shapes and knobs, and the float accumulation orders are fixed -- so a leading dimension that is 0 mod 8 elements and a
16-byte-aligned offset take the same code path.  It also carries the second check: every operand of (b) is surrounded by NaN, so a
kernel that loads past K or N and relies on multiplying by zero, or reads a neighbour's row, would not reproduce the bits of (a).
The one route that does depend on a leading dimension (the weight gradient with a bf16 pitch that is no multiple of 8) is held to fp64."""
import pytest
import torch

from tests.guard_bands import Arena, guarded_ops, roundup

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import hostmath, ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_GELU, EPI_BIAS_RESID, lib

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
BOTH = (BF, F32)
PAD, OFF = 32, 16                     # elements: the strided views of (b) are columns [16, 16 + cols) of a [rows, cols + 32] payload


def gen(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def tname(T):
    return "bf16" if T == BF else "fp32"


def rel64(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Ctx:
    """What a case builds its operands with: run (a) has arena = None."""

    def __init__(self, arena=None):
        self.arena = arena

    @property
    def guarded(self):
        return self.arena is not None

    def inp(self, t):
        """an operand without a leading dimension in the ABI: exact-size and surrounded by NaN in (b)"""
        return t if t is None or not self.guarded else self.arena.place(t)

    def mat(self, t, ld=None, off=None, align=16):
        """a matrix operand with an ld* argument: a column slice of a wider NaN payload in (b)"""
        if not self.guarded:
            return t
        ld, off = self._ld(t.shape[1], t.element_size(), ld, off)
        return self.arena.place(t, ld=ld, col_off=off, align=align)

    def out(self, shape, dtype, ld=None, off=None):
        """an optional `out=` matrix: None in (a) (the op allocates it), a strided arena view in (b)"""
        if not self.guarded:
            return None
        return self.buf(shape, dtype, ld=ld, off=off, strided=True)

    def buf(self, shape, dtype, ld=None, off=None, strided=False, align=16):
        """an output the caller has to bring: torch.empty in (a), an arena tensor (strided on request) in (b)"""
        if not self.guarded:
            return torch.empty(shape, dtype=dtype, device=DEV)
        if not strided:
            return self.arena.empty(shape, dtype)
        ld, off = self._ld(shape[1], torch.empty((), dtype=dtype).element_size(), ld, off)
        return self.arena.empty(shape, dtype, ld=ld, col_off=off, align=align)

    @staticmethod
    def _ld(cols, es, ld, off):
        assert cols % 8 == 0
        return (cols + PAD if ld is None else ld), (OFF if off is None else off)


class Rows:
    """A compact live-row buffer: rows [0, count) hold results, rows up to roundup(count, 128) are zero (when zero_pad), the rest is not
    touched -- and must still be poison in (b)."""

    def __init__(self, t, count, zero_pad=True):
        self.t, self.count, self.zero_pad = t, int(count), zero_pad


class Gate:
    """A result held to an fp64 reference instead of to the bits of (a)."""

    def __init__(self, t, ref, tol):
        self.t, self.ref, self.tol = t, ref, tol


def bits(t):
    return t.contiguous().view(torch.uint8)


def compare(name, a, b, arena):
    if not isinstance(a, (torch.Tensor, Rows, Gate)):
        assert a == b, "%s: (a) %r, (b) %r" % (name, a, b)
        return
    if isinstance(b, Gate):
        assert arena.unwritten(b.t) == 0, "%s: %d element(s) of the guarded result were never written" % (name, arena.unwritten(b.t))
        e = rel64(b.t, b.ref)
        print("%s: guarded run against fp64 %.3e (gate %.3e; unguarded %.3e)" % (name, e, b.tol, rel64(a.t, a.ref)))
        assert e < b.tol, (name, e, b.tol)
        return
    if isinstance(b, Rows):
        assert a.count == b.count, (name, a.count, b.count)
        n, pad = b.count, (roundup(b.count, 128) if b.zero_pad else b.count)
        assert torch.equal(bits(a.t[:n]), bits(b.t[:n])), "%s: live rows differ" % name
        assert float(b.t[n:pad].float().abs().sum()) == 0.0, "%s: rows [count, roundup(count, 128)) are not zero" % name
        rest = b.t[pad:]
        assert arena.unwritten(rest) == rest.numel(), "%s: rows behind roundup(count, 128) = %d were written" % (name, pad)
        return
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if b.dtype.is_floating_point:
        n = arena.unwritten(b)
        assert n == 0, "%s: %d of %d element(s) of the guarded result were never written (still 0xFF)" % (name, n, b.numel())
    same = torch.equal(bits(a), bits(b))
    if not same:
        af, bf_ = a.double().flatten(), b.double().flatten()
        nan_b, nan_a = int(torch.isnan(bf_).sum()), int(torch.isnan(af).sum())
        diff = int((bits(a) != bits(b)).sum())
        raise AssertionError("%s: the guarded, strided run is not bit-identical to the contiguous one (%d bytes differ; NaN in (a) %d, in (b) %d).  "
                             "Exact-size NaN-surrounded operands changed the result: a read outside an operand (past K, N or the last row), "
                             "a store that skipped an element, or a route that depends on ld." % (name, diff, nan_a, nan_b))


CASES = []


def case(id_, covers):
    def deco(fn):
        CASES.append(pytest.param(fn, covers, id=id_))
        return fn
    return deco


def run_case(fn, covers, monkeypatch):
    called = {}

    def counted(name, f):
        def g(*a, **k):
            called[name] = called.get(name, 0) + 1
            return f(*a, **k)
        return g
    res_a = fn(Ctx())
    torch.cuda.synchronize()
    arena = Arena(DEV)
    with guarded_ops(monkeypatch, arena, ops=ops), monkeypatch.context() as m:
        for name in covers:
            m.setattr(ops, name, counted(name, getattr(ops, name)))
        res_b = fn(Ctx(arena))
    arena.check()
    missing = [n for n in covers if n not in called]
    assert not missing, "the case says it covers %s but never called them" % missing
    assert res_a.keys() == res_b.keys()
    for k in res_a:
        compare(k, res_a[k], res_b[k], arena)


@pytest.mark.parametrize("fn,covers", CASES)
def test_guard_bands(fn, covers, monkeypatch):
    run_case(fn, covers, monkeypatch)


# ------------------------------------------------------------------------------------------------ completeness
# public callables of painter_amd.ops that enqueue nothing
EXCLUDED = {
    "stream": "host: the current stream's handle",
    "code": "host: dtype -> ABI code",
    "p": "host: data pointer or 0",
    "workspace": "host: the scratch allocator the harness replaces",
    "drop_skip": "knob accessor (16)",
    "decoder_rows": "knob accessor (17)",
    "gelu_aux_dtype": "host: dtype of the GELU side output",
    "gelu_aux_decode": "torch arithmetic for tests and tools, no kernel of the library",
    "gelu_aux_encode": "torch arithmetic for tests and tools, no kernel of the library",
    "decoder_live_ok": "host-only query",
    "padded_rows": "host arithmetic",
    "layernorm_bwd_workspace_bytes": "host-only size helper (held to the kernel by the layernorm_bwd defer case)",
    "attn_launch_counts": "host-side counters",
    "patch_cols_ok": "host-only query",
}


def test_every_kernel_enqueuing_function_of_ops_is_in_the_table():
    public = {n for n, f in vars(ops).items() if callable(f) and not n.startswith("_") and getattr(f, "__module__", None) == ops.__name__}
    covered = set()
    for c in CASES:
        covered |= set(c.values[1])
    assert not (covered & set(EXCLUDED)), covered & set(EXCLUDED)
    assert covered <= public and set(EXCLUDED) <= public, ((covered | set(EXCLUDED)) - public)
    assert public - covered - set(EXCLUDED) == set(), "entry points of painter_amd.ops without a guard-band case or a stated exclusion: %s" % sorted(public - covered - set(EXCLUDED))


# ------------------------------------------------------------------------------------------------ linear
def _linear_fwd(T, M, N, K):
    def fn(c):
        x, w, b = c.mat(gen((M, K), 1, 1.0, T)), c.inp(gen((N, K), 2, 0.05, T)), c.inp(gen((N,), 3))
        rps = 8
        rowscale = c.inp(gen(((M + rps - 1) // rps,), 5).abs() + 0.5)
        r = {}
        r["bias"] = ops.linear_fwd(x, w, b, EPI_BIAS, out=c.out((M, N), T))
        r["bias_f32"] = ops.linear_fwd(x, w, b, EPI_BIAS_F32, out=c.out((M, N), F32))
        act = c.buf((M, N), T, strided=True)
        aux = c.buf((M, N), ops.gelu_aux_dtype(T), strided=True, align=8)              # (shares ldo: elements of fp32, bytes of the 8-bit code -- rows of the code are 8-byte aligned where N % 16 == 8, as in (a))
        ops.linear_fwd(x, w, b, EPI_BIAS_GELU, out=act, out2=aux)
        r["gelu"], r["gelu_aux"] = act, aux
        r["gelu_pair"], r["gelu_pair_aux"] = ops.linear_gelu(x, w, b)                   # the wrapper: contiguous act / aux of its own
        r["resid"] = ops.linear_fwd(x, w, b, EPI_BIAS_RESID, out=c.out((M, N), F32), resid=c.mat(gen((M, N), 4)), rowscale=rowscale, rows_per_sample=rps)
        return r
    return fn


for T_ in BOTH:
    # (328, 264, 256), (500, 264, 256): the 256 x 256 kernel (bf16) with ragged 256-, 224- and half-tiles; the other two: the generic engine
    for s_ in [(328, 264, 256), (500, 264, 256), (200, 192, 128), (96, 64, 72)]:
        case("linear_fwd-%s-%dx%dx%d" % ((tname(T_),) + s_), ("linear_fwd", "linear_gelu"))(_linear_fwd(T_, *s_))


@case("linear_fwd-rowskip-bf16", ("linear_fwd",))
def _linear_fwd_rowskip(c):
    """tests/test_droppath_skip_gpu.py GEMM_SHAPES[2]: 4 samples of 640 rows (2.5 tiles), D = 256, hidden 1024; samples 1 and 2 dropped"""
    n, rps, D, hid = 4, 640, 256, 1024
    R = n * rps
    f = torch.full((n,), 1.25, dtype=F32)
    f[[1, 2]] = 0.0
    f = c.inp(f.to(DEV))
    old = ops.drop_skip(2)
    try:
        x = c.mat(gen((R, D), 31, 1.0, BF))
        r = {"qkv": ops.linear_fwd(x, c.inp(gen((3 * D, D), 11, 0.03, BF)), c.inp(gen((3 * D,), 12, 0.5)), EPI_BIAS, out=c.out((R, 3 * D), BF),
                                   rowskip=f, skip_rows_per_sample=rps)}
        act, aux = c.buf((R, hid), BF, strided=True), c.buf((R, hid), torch.uint8, strided=True)
        ops.linear_fwd(x, c.inp(gen((hid, D), 13, 0.03, BF)), c.inp(gen((hid,), 14, 0.5)), EPI_BIAS_GELU, out=act, out2=aux, rowskip=f, skip_rows_per_sample=rps)
        r["fc1"], r["fc1_aux"] = act, aux
        r["proj"] = ops.linear_fwd(x, c.inp(gen((D, D), 15, 0.03, BF)), c.inp(gen((D,), 16, 0.5)), EPI_BIAS_RESID, out=c.out((R, D), F32),
                                   resid=c.mat(gen((R, D), 19)), rowscale=f, rows_per_sample=rps, rowskip=f)
        return r
    finally:
        ops.drop_skip(old)


def _linear_pixshuf(T):
    def fn(c):
        B, Hp, Wp, P, C, K = 2, 8, 4, 16, 64, 256           # test_linear_strided_views_and_pixshuf
        x = c.mat(gen((B * Hp * Wp, K), 1, 1.0, T), ld=2 * K, off=K)
        return {"out": ops.linear_pixshuf(x, c.inp(gen((P * P * C, K), 2, 0.05, T)), c.inp(gen((P * P * C,), 3)), B, Hp, Wp, P, C)}
    return fn


for T_ in BOTH:
    case("linear_pixshuf-%s" % tname(T_), ("linear_pixshuf",))(_linear_pixshuf(T_))


def _gelu_aux(pre):
    """what linear_gelu hands to linear_dgrad: the pre-activation (fp32 build), the 8-bit code of gelu'(pre) (bf16 build)"""
    if pre.dtype == F32:
        return pre
    pg = pre.double().clone().requires_grad_(True)
    torch.nn.functional.gelu(pg).sum().backward()
    return ops.gelu_aux_encode(pg.grad)


def _linear_dgrad(T, M, N, K):
    def fn(c):
        dy, w = c.mat(gen((M, N), 6, 1.0, T)), c.inp(gen((N, K), 7, 0.05, T))
        aux = c.mat(_gelu_aux(gen((M, K), 9, 1.0, T)), align=8)                      # byte pitch (bf16 build) = the pitch of dx in elements
        r = {"plain": ops.linear_dgrad(dy, w, out=c.out((M, K), T))}
        r["gelu"] = ops.linear_dgrad(dy, w, gelu_aux=aux, out=c.out((M, K), T))
        cs, cs2 = c.buf((K,), F32), c.buf((K,), F32)
        r["plain_cs_dx"], r["plain_cs"] = ops.linear_dgrad(dy, w, out=c.out((M, K), T), colsum_out=cs), cs
        r["gelu_cs_dx"], r["gelu_cs"] = ops.linear_dgrad(dy, w, gelu_aux=aux, out=c.out((M, K), T), colsum_out=cs2), cs2
        return r
    return fn


for T_ in BOTH:
    for s_ in [(500, 256, 264), (96, 128, 136), (328, 264, 256)]:
        case("linear_dgrad-%s-%dx%dx%d" % ((tname(T_),) + s_), ("linear_dgrad",))(_linear_dgrad(T_, *s_))


def _linear_wgrad(T, M, N, K):
    def fn(c):
        dy, x = c.mat(gen((M, N), 1, 1.0, T)), c.mat(gen((M, K), 3, 1.0, T))
        return {"dw": ops.linear_wgrad(dy, x), "db": ops.colsum(dy)}
    return fn


for T_ in BOTH:
    # (512, 256, 256): bf16 the 256 x 256 kernel with 2 split-K slabs; (200, 192, 128): the generic engine
    for s_ in [(512, 256, 256), (200, 192, 128)]:
        case("linear_wgrad-%s-%dx%dx%d" % ((tname(T_),) + s_), ("linear_wgrad", "colsum"))(_linear_wgrad(T_, *s_))


@case("linear_wgrad-bf16-512x256x256-lddy-N+4", ("linear_wgrad",))
def _linear_wgrad_odd_pitch(c):
    """The route that depends on ld (csrc/gemm.hip, linear_wgrad_t):
        if (wgrad_fast(PA_BF16, M, N, K) && g256::ok(N, K, M, true, true, lddy, ldx)) -> 256 x 256 kernel, wgrad_fast_splits() = 2 slabs
        else                                                                          -> generic engine,   wgrad_splits()      = 8 slabs
    g256::ok refuses lddy % 8 != 0, so dy with a pitch of N + 4 takes the generic engine at a shape pa_linear_wgrad_workspace_bytes used to
    size for the fast route alone: 512 KiB asked, 2 MiB written.  Another K split and tile shape than (a): held to fp64 at the bf16 gate of
    test_linear_backward (1e-4: operands exact in bf16, fp32 accumulation) instead of to the bits."""
    M, N, K = 512, 256, 256
    dy0, x0 = gen((M, N), 1, 1.0, BF), gen((M, K), 3, 1.0, BF)
    ref = dy0.double().t() @ x0.double()
    dy = c.mat(dy0, ld=N + 4, off=0, align=8)
    assert not c.guarded or (dy.stride(0) == N + 4 and lib.pa_linear_wgrad_workspace_bytes(ops.code(BF), M, N, K) == 8 * N * K * 4)
    return {"dw": Gate(ops.linear_wgrad(dy, c.mat(x0)), ref, 1e-4)}


def _colsum(T, M, N):
    def fn(c):
        return {"sum": ops.colsum(c.mat(gen((M, N), 1, 1.0, T)))}
    return fn


for T_ in BOTH:
    for s_ in [(200, 192), (4100, 264)]:           # both chunk heights of the two-stage sum
        case("colsum-%s-%dx%d" % ((tname(T_),) + s_), ("colsum",))(_colsum(T_, *s_))


# ------------------------------------------------------------------------------------------------ layernorm
LN_SHAPES = [(33, 1280), (1003, 1024), (64, 128)]


def _ln_operands(c, T, R, D):
    x = c.mat(gen((R, D), 1, 2.0) + 0.3)
    return x, c.inp(1 + gen((D,), 2, 0.1)), c.inp(gen((D,), 3, 0.1))


def _layernorm_fwd(T, R, D):
    def fn(c):
        x, gamma, beta = _ln_operands(c, T, R, D)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6, T, out=c.out((R, D), T, ld=4 * D, off=D))      # the tap concat buffer's slice [:, D:2D]
        return {"y": y, "mean": mean, "rstd": rstd}
    return fn


def _layernorm_bwd(T, R, D, knob):
    def fn(c):
        old = lib.pa_debug_get(10)
        lib.pa_debug_set(10, knob)
        try:
            x, gamma, beta = _ln_operands(c, T, R, D)
            _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6, T)
            dy = c.mat(gen((R, D), 4, 1.0, T), ld=4 * D, off=D)                       # a slice of dconcat
            rps = 8
            dres, rowscale = c.mat(gen((R, D), 5)), c.inp(gen(((R + rps - 1) // rps,), 6).abs() + 0.5)
            r = {}
            dxT, cs = c.buf((R, D), T, strided=True), c.buf((D,), F32)
            r["dx"], r["gb"] = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres=dres, dx=c.buf((R, D), F32, strided=True), dxT=dxT, rowscale=rowscale,
                                                 rows_per_sample=rps, dxT_colsum=cs)
            r["dxT"], r["cs"] = dxT, cs
            # the deferred form: the partial rows stay in a caller-owned buffer of exactly pa_layernorm_bwd_workspace_bytes, finish() reduces them
            dxT2, cs2 = c.buf((R, D), T, strided=True), c.buf((D,), F32)
            ws = c.buf((ops.layernorm_bwd_workspace_bytes(R, D),), torch.uint8)
            r["defer_dx"], finish = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres=dres, dx=c.buf((R, D), F32, strided=True), dxT=dxT2, rowscale=rowscale,
                                                      rows_per_sample=rps, dxT_colsum=cs2, defer=True, ws=ws)
            r["defer_gb"] = finish()
            r["defer_dxT"], r["defer_cs"] = dxT2, cs2
            # without the T copy, without dres, scratch from the deferred form's own allocation
            r["bare_dx"], fin = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx=c.buf((R, D), F32, strided=True), defer=True)
            r["bare_gb"] = fin()
            return r
        finally:
            lib.pa_debug_set(10, old)
    return fn


for T_ in BOTH:
    for s_ in LN_SHAPES:
        case("layernorm_fwd-%s-%dx%d" % ((tname(T_),) + s_), ("layernorm_fwd",))(_layernorm_fwd(T_, *s_))
        for knob_ in (0, 1):
            case("layernorm_bwd-%s-%dx%d-knob10=%d" % ((tname(T_),) + s_ + (knob_,)), ("layernorm_bwd", "layernorm_fwd"))(_layernorm_bwd(T_, *s_, knob_))


# ------------------------------------------------------------------------------------------------ attention
def _relpos(T, Hp, Wp, hd):
    def fn(c):
        nb = 3
        hs = [c.inp(gen((2 * Hp - 1, hd), 10 + k, 0.2)) for k in range(nb)]
        ws = [c.inp(gen((2 * Wp - 1, hd), 50 + k, 0.2)) for k in range(nb)]
        tabs = c.inp(torch.tensor([t.data_ptr() for t in hs] + [t.data_ptr() for t in ws], dtype=torch.int64).to(DEV))
        r = {"rcat": ops.relpos_pack(hs[0], ws[0], Hp, Wp, T), "rcatT": ops.relpos_pack_t(hs[0], ws[0], Hp, Wp, T)}
        r["batch_rcat"], r["batch_rcatT"] = ops.relpos_pack_batch(tabs, nb, Hp, Wp, hd, T)
        return r
    return fn


for T_ in BOTH:
    for s_ in [(8, 4, 64), (8, 28, 64), (4, 32, 80)]:
        case("relpos_pack-%s-%dx%d-hd%d" % ((tname(T_),) + s_), ("relpos_pack", "relpos_pack_t", "relpos_pack_batch"))(_relpos(T_, *s_))


def _attn(T, B, H, Hp, Wp, hd, family, prep="fused", knob7=0):
    """family: index into attn_launch_counts() of the kernels both runs must have used (0 generic, 1 generation 2, 2 generation 3; None: only
    that (a) and (b) used the same).
    Operands: the unit Gaussians of test_attn_fwd."""
    def fn(c):
        L = Hp * Wp
        scale = hd ** -0.5
        old7 = lib.pa_debug_get(7)
        lib.pa_debug_set(7, knob7)
        try:
            qkv = c.mat(gen((B * L, 3 * H * hd), 1, 1.0, T))
            rel_h, rel_w = c.inp(gen((2 * Hp - 1, hd), 2, 0.2)), c.inp(gen((2 * Wp - 1, hd), 3, 0.2))
            dout = c.mat(gen((B * L, H * hd), 4, 1.0, T))
            rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T)
            c0 = ops.attn_launch_counts()
            out, lse, tables = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale, need_tables=True)
            out2, lse2 = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, scale)
            r = {"out": out, "lse": lse, "out_no_tables": out2, "lse_no_tables": lse2, "has_tables": tables is not None}
            o_in = c.mat(out)                                                       # the backward reads out and dout through their own pitches
            if prep == "fused" and knob7 == 0:
                r["dqkv"], r["drcat"] = ops.attn_bwd(qkv, rcat, rcatT, o_in, dout, lse, B, L, H, Hp, Wp, scale, tables=tables)
            else:
                r["dqkv"], dG = ops.attn_bwd_core(qkv, rcat, rcatT, o_in, dout, lse, B, L, H, Hp, Wp, scale, tables=tables, prep=prep)
                r["dG_is_partials"] = dG.dtype == torch.uint8
                r["drcat"] = ops.attn_bwd_relpos(dG, qkv, rcat.shape[0], B, L, H, Hp, Wp)
            c1 = ops.attn_launch_counts()
            r["family"] = tuple((c1[k][i] - c0[k][i]) > 0 for k in ("fwd", "bwd") for i in range(3))
            want = tuple(i == family for _ in ("fwd", "bwd") for i in range(3))
            assert family is None or r["family"] == want, (r["family"], want)
            return r
        finally:
            lib.pa_debug_set(7, old7)
    return fn


ATTN_COVERS = ("attn_fwd", "attn_bwd", "attn_bwd_core", "attn_bwd_relpos", "relpos_pack", "relpos_pack_t")
for T_ in BOTH:
    case("attn-%s-1x2x8x4-hd64" % tname(T_), ATTN_COVERS)(_attn(T_, 1, 2, 8, 4, 64, 0))                              # generic
    case("attn-%s-1x2x8x12-hd64" % tname(T_), ATTN_COVERS)(_attn(T_, 1, 2, 8, 12, 64, 1 if T_ == BF else 0))           # bf16: generation 2
    case("attn-%s-2x1x8x12-hd80" % tname(T_), ATTN_COVERS)(_attn(T_, 2, 1, 8, 12, 80, None))
    case("attn-%s-1x1x4x32-hd80" % tname(T_), ATTN_COVERS)(_attn(T_, 1, 1, 4, 32, 80, None))
case("attn-fp32-1x1x8x28-hd64", ATTN_COVERS)(_attn(F32, 1, 1, 8, 28, 64, 0))
ATTN3_COVERS = ("attn_fwd", "attn_bwd_core", "attn_bwd_relpos")
case("attn-bf16-1x1x8x28-hd64-gen3", ATTN_COVERS)(_attn(BF, 1, 1, 8, 28, 64, 2))                                        # generation 3: Delta in the dQ kernel, fused rel-pos sums
case("attn-bf16-1x1x8x28-hd64-gen3-prep-launch", ATTN3_COVERS)(_attn(BF, 1, 1, 8, 28, 64, 2, prep="launch"))
case("attn-bf16-1x1x8x28-hd64-gen3-relpos-dG", ATTN3_COVERS)(_attn(BF, 1, 1, 8, 28, 64, 2, knob7=1))                   # dG in HBM + the gather GEMM
case("attn-bf16-1x1x8x28-hd64-gen3-relpos-fused", ATTN3_COVERS)(_attn(BF, 1, 1, 8, 28, 64, 2, knob7=2))


# ------------------------------------------------------------------------------------------------ patch embedding
def _patch_embed(T, B, Hp, Wp, P, D):
    def fn(c):
        L = Hp * Wp
        imgs, tgts = c.inp(gen((B, 3, Hp * P, Wp * P), 1)), c.inp(gen((B, 3, Hp * P, Wp * P), 2))
        w, bias = c.inp(gen((D, 3, P, P), 3, 0.05)), c.inp(gen((D,), 4, 0.1))
        mask_token, seg_x, seg_y = c.inp(gen((D,), 5, 0.3)), c.inp(gen((D,), 6, 0.3)), c.inp(gen((D,), 7, 0.3))
        pos = c.inp(gen((L, D), 8, 0.2))
        tcls, tins = c.inp(gen((D,), 9, 0.3)), c.inp(gen((D,), 10, 0.3))
        seg_type = c.inp(torch.tensor([0.0, 1.0], device=DEV))
        mask = c.inp((torch.rand(B, L, generator=torch.Generator().manual_seed(11)) < 0.4).to(torch.uint8).to(DEV))
        r = {"wop": ops.patch_weight_pack(w, T, P)}
        kp = r["wop"].shape[1]
        assert kp == (3 * P * P + 7) // 8 * 8
        wop = c.mat(r["wop"])                                                          # the packed weight behind a pitch of its own (ldw); the pack itself has no ld
        for name, tok in (("painter", (None, None, None)), ("seggpt", (tcls, tins, seg_type))):
            r["tokens_" + name] = ops.patch_embed_fwd(T, imgs, tgts, wop, bias, mask_token, seg_x, seg_y, pos, mask, *tok, B, Hp, Wp, P, D)
        dpe = c.inp(gen((2 * B * L, D), 12, 1.0, T))
        r["dw"] = ops.patch_embed_wgrad(dpe, imgs, tgts, B, Hp, Wp, P, D)
        r["cols_ok"] = ops.patch_cols_ok(T, B, L, P, D)
        assert r["cols_ok"] == (T == BF and P == 16)
        if P % 8 == 0:
            cols = ops.patch_im2col(imgs, tgts, B, Hp, Wp, P)                           # (bf16 whatever T: the operand of the fast path)
            r["cols"] = cols
        if r["cols_ok"]:
            r["tokens_cols"] = ops.patch_embed_fwd_cols(cols, wop, bias, mask_token, seg_x, seg_y, pos, mask, tcls, tins, seg_type, B, L, D)
        r["dimgs"], r["dtgts"] = ops.patch_embed_dgrad(dpe, wop, B, Hp, Wp, P, D)
        add = c.inp(gen((B, 3, Hp * P, Wp * P), 13))
        r["dimgs_add"], r["dtgts_add"] = ops.patch_embed_dgrad(dpe, wop, B, Hp, Wp, P, D, addend=add, alpha=-1.0)
        r["only_imgs"], none = ops.patch_embed_dgrad(dpe, wop, B, Hp, Wp, P, D, want_tgts=False)
        none2, r["only_tgts"] = ops.patch_embed_dgrad(dpe, wop, B, Hp, Wp, P, D, want_imgs=False)
        assert none is None and none2 is None
        return r
    return fn


PATCH_COVERS = ("patch_weight_pack", "patch_embed_fwd", "patch_embed_wgrad", "patch_embed_dgrad")
for T_ in BOTH:
    for s_ in [(2, 8, 4, 16, 128), (2, 8, 4, 14, 160)]:
        case("patch_embed-%s-%dx%dx%d-P%d-D%d" % ((tname(T_),) + s_), PATCH_COVERS + (("patch_im2col",) if s_[3] == 16 else ()) + (("patch_embed_fwd_cols",) if T_ == BF and s_[3] == 16 else ()))(_patch_embed(T_, *s_))


# ------------------------------------------------------------------------------------------------ glue
def _glue(T):
    def fn(c):
        batch, L, D = 2, 32, 128
        R = batch * L
        r = {}
        x = c.inp(gen((2 * R, D), 1))
        r["merge_fwd"] = ops.merge_fwd(x, R, D)
        dm, rowscale = c.inp(gen((R, D), 2)), c.inp(gen((2 * batch,), 4).abs() + 0.5)
        r["merge_bwd_dx"], r["merge_bwd_dxT"] = ops.merge_bwd(T, dm, rowscale, L, R, D)
        r["merge_bwd_dx_noscale"], r["merge_bwd_dxT_noscale"] = ops.merge_bwd(T, dm, None, L, R, D)
        r["scale_cast"] = ops.scale_cast(T, x, rowscale, L)
        r["scale_cast_noscale"] = ops.scale_cast(T, x, None, L)
        r["cast_bf16"] = ops.cast_bf16(c.inp(gen((3 * D * D + 3,), 7)))              # no multiple of 4: the scalar tail
        a = c.inp(gen((R, D), 8))
        for group in (1, 2):
            r["ensemble_resid_%d" % group] = ops.ensemble_resid(dm, a, batch, group, L, D)
        for shared in (False, True):
            mask = c.inp((torch.rand((1 if shared else batch, L), generator=torch.Generator().manual_seed(9)) < 0.4).to(torch.uint8).to(DEV))
            r["tokens_bwd_dpe_%d" % shared], r["tokens_bwd_sums_%d" % shared] = ops.tokens_bwd(T, x, mask, batch, L, D)
        # abs-pos resize as a row-sparse operator: 14 x 14 source grid -> 8 x 4 tokens
        src, Hp, Wp = 14, 8, 4
        M = hostmath.abs_pos_operator(src, Hp, Wp)
        dev = lambda t: (c.inp(torch.from_numpy(t[0]).to(DEV)), c.inp(torch.from_numpy(t[1]).to(DEV)))
        fwd, bwd = dev(hostmath.sparse_rows(M)), dev(hostmath.sparse_rows(M.T))
        r["pos_fwd"] = ops.pos_fwd(fwd, c.inp(gen((src * src, D), 10)), Hp * Wp, D)
        dpe = c.buf((src * src, D), F32)
        ops.pos_bwd(bwd, c.inp(gen((Hp * Wp, D), 11)), c.inp(gen((Hp * Wp, D), 12)), dpe, src * src, D)
        r["pos_bwd"] = dpe
        return r
    return fn


GLUE_COVERS = ("pos_fwd", "pos_bwd", "tokens_bwd", "merge_fwd", "merge_bwd", "scale_cast", "cast_bf16", "ensemble_resid")
for T_ in BOTH:
    case("glue-%s" % tname(T_), GLUE_COVERS)(_glue(T_))


# ------------------------------------------------------------------------------------------------ decoder tail and 3 x 3 convolution
def _decoder_tail(T, B, Hi, Wi):
    def fn(c):
        P, Hp, Wp = 16, Hi // 16, Wi // 16
        x = c.inp(gen((B, Hi, Wi, 64), 1, 1.0, T))
        w3 = c.inp(gen((64, 64, 3, 3), 2, 0.05))
        b3, gamma, beta = c.inp(gen((64,), 3, 0.1)), c.inp(1.0 + gen((64,), 4, 0.1)), c.inp(gen((64,), 5, 0.1))
        w1, b1 = c.inp(gen((3, 64), 6, 0.1)), c.inp(gen((3,), 7, 0.1))
        r = {}
        r["w3r"], r["wf"] = ops.conv3x3_pack(w3, T)
        r["pred"], r["y3"] = ops.decoder_tail_fwd(x, r["w3r"], b3, gamma, beta, w1, b1, 1e-6, save_y3=True)
        r["pred_no_y3"], none = ops.decoder_tail_fwd(x, r["w3r"], b3, gamma, beta, w1, b1, 1e-6, save_y3=False)
        assert none is None
        dpred = c.inp(gen((B, 3, Hi, Wi), 8))
        r["dy3"], grads = ops.decoder_tail_bwd_pointwise(dpred, r["y3"], gamma, beta, w1, 1e-6)
        r["grads"] = grads[:323]                       # dgamma, dbeta, dw1, db1; the 324th float is padding
        dy = c.inp(gen((B, Hi, Wi, 64), 9, 1.0, T))
        r["dE"] = ops.conv3x3_dgrad_unshuffle(dy, r["wf"], B, Hp, Wp, P)
        r["dw"] = ops.conv3x3_wgrad(dy, x)
        try:                                           # knob 9: a cap on the weight-gradient workgroups, so that one walks many tiles
            assert lib.pa_debug_set(9, 1) == 0
            r["dw_cap1"] = ops.conv3x3_wgrad(dy, x)
        finally:
            lib.pa_debug_set(9, 0)
        return r
    return fn


TAIL_COVERS = ("conv3x3_pack", "decoder_tail_fwd", "decoder_tail_bwd_pointwise", "conv3x3_dgrad_unshuffle", "conv3x3_wgrad")
for T_ in BOTH:
    # Wi = 64: the bf16 tile kernels (csrc/conv64.h); Wi = 48: the generic route; fp32 is generic at both
    for s_ in [(2, 16, 64), (2, 16, 48)]:
        case("decoder_tail-%s-%dx%dx%d" % ((tname(T_),) + s_), TAIL_COVERS)(_decoder_tail(T_, *s_))


# ------------------------------------------------------------------------------------------------ live rows
def _live_rows(Hp, Wp):
    def fn(c):
        from tests.test_decoder_live_rows_gpu import batch_masks
        B, P, Kin = 2, 16, 256
        M, Hi, Wi, N = B * Hp * Wp, Hp * P, Wp * P, P * P * 64
        Mp = ops.padded_rows(M)
        assert ops.decoder_live_ok(BF, B, Hp, Wp, P, Kin)
        pred, tgts = c.inp(gen((B, 3, Hi, Wi), 1)), c.inp(gen((B, 3, Hi, Wi), 2))
        valid = c.inp((torch.rand((B, 3, Hi, Wi), generator=torch.Generator().manual_seed(3)) < 0.9).float().to(DEV))
        dloss, loss_out = c.inp(torch.full((1,), 1.5, device=DEV)), c.inp(torch.tensor([0.3, 41.0], device=DEV))
        y3 = c.inp(gen((B, Hi, Wi, 64), 4, 1.0, BF))
        gamma, beta, w1 = c.inp(gen((64,), 5).abs() + 0.5), c.inp(gen((64,), 6, 0.3)), c.inp(gen((3, 64), 7, 0.2))
        _, wf = ops.conv3x3_pack(c.inp(gen((64, 64, 3, 3), 8, 0.05)), BF)
        w = c.inp(gen((N, Kin), 9, 0.05, BF))                       # decoder_embed's weight [P*P*64, Kin]
        xin = gen((M, Kin), 10, 1.0, BF)                             # its input rows
        r = {}
        for name, mask in batch_masks(Hp, Wp, B).items():
            mask_u8 = c.inp(torch.from_numpy(mask.copy()).to(DEV))
            dpred = ops.loss_bwd(pred, tgts, valid, mask_u8, dloss, loss_out, P, "smoothl1")
            dy3, _ = ops.decoder_tail_bwd_pointwise(dpred, y3, gamma, beta, w1, 1e-6)
            rowmap, live, count = ops.live_rows(mask_u8, B, Hp, Wp)
            n = int(count.item())
            r[name + "/rowmap"], r[name + "/count"], r[name + "/live"] = rowmap, count, live[:n]
            dE = ops.conv3x3_dgrad_unshuffle_live(dy3, wf, rowmap, count, B, Hp, Wp, P)
            r[name + "/dE"] = Rows(dE, n)
            # data gradient: compact rows in (the NaN behind roundup(count, 128) with them), every row of dx out -- zeros where rowmap is -1
            r[name + "/dx"] = ops.linear_dgrad(c.mat(dE), w, out=c.out((M, Kin), BF), live=(live, rowmap, count))
            xg = ops.gather_rows(c.mat(xin), live, count, out=c.out((Mp, Kin), BF))
            r[name + "/gather"] = Rows(xg, n)
            r[name + "/dw"] = ops.linear_wgrad_live(c.mat(dE), xg, count)
            r[name + "/dw_via_wgrad"] = ops.linear_wgrad(dE, c.mat(xin), live=(live, count))
            r[name + "/db"] = ops.colsum_live(c.mat(dE), count)
        return r
    return fn


LIVE_COVERS = ("live_rows", "gather_rows", "conv3x3_dgrad_unshuffle_live", "linear_dgrad", "linear_wgrad", "linear_wgrad_live", "colsum_live", "loss_bwd")
for s_ in [(4, 4), (4, 3)]:             # 4 x 4: the conv tile kernel and its dead-tile exit; 4 x 3 (48 pixels wide): the gather engine
    case("live_rows-%dx%d" % s_, LIVE_COVERS)(_live_rows(*s_))


# ------------------------------------------------------------------------------------------------ loss and patchify
def _loss(kind):
    def fn(c):
        from oracle import painter_oracle as O
        B, Hi, Wi, P = 2, 32, 16, 16
        Hp, Wp = Hi // P, Wi // P
        g = torch.Generator().manual_seed(5)
        tgts = torch.randn(B, 3, Hi, Wi, generator=g)
        tgts[0] = (-torch.tensor(O.IMAGENET_MEAN) / torch.tensor(O.IMAGENET_STD))[:, None, None]     # a black picture: the ignore rule fires on sample 0
        pred = tgts + 0.02 * torch.randn(tgts.shape, generator=g)
        valid = torch.ones_like(tgts)
        valid[1, :, Hi // 4:Hi // 2, Wi // 8:Wi // 2] = 0.0
        mask = torch.rand(B, Hp * Wp, generator=g) < 0.5
        mask[:, 0] = True
        pd, td, vd = c.inp(pred.to(DEV)), c.inp(tgts.to(DEV)), c.inp(valid.to(DEV))
        r = {}
        for shared in (False, True):
            tag = "shared" if shared else "painter"
            m8 = c.inp((mask[:1] if shared else mask).to(torch.uint8).to(DEV))
            v = c.inp(valid.to(DEV))                                                        # (the rule writes into it)
            out = ops.loss_fwd(pd, td, v, m8, P, ignore_rule=True, eps_den=1e-2, kind=kind)
            r["loss_" + tag], r["valid_" + tag] = out, v
            dloss = c.inp(torch.tensor([0.75], device=DEV))
            r["loss_bwd_" + tag] = ops.loss_bwd(pd, td, v, m8, dloss, out, P, kind)
            dpatch = c.inp(gen((B, Hp * Wp, 3 * P * P), 6))
            r["pred_bwd_both_" + tag], r["pred_bwd_lossterm_" + tag] = ops.pred_bwd(pd, td, v, m8, dloss, out, dpatch, P, kind, want_loss_term=True)
            r["pred_bwd_loss_" + tag], none = ops.pred_bwd(pd, td, v, m8, dloss, out, None, P, kind)
            r["pred_bwd_patch_" + tag], none2 = ops.pred_bwd(pd, td, v, m8, None, out, dpatch, P, kind)
            assert none is None and none2 is None
        assert float(r["valid_painter"][0].abs().max()) == 0.0                                 # the rule fired, in place
        r["patchify"] = ops.patchify(pd, Hp, Wp, P)
        return r
    return fn


for kind_ in ("smoothl1", "l1", "l2", "l1l2"):
    case("loss-%s" % kind_, ("loss_fwd", "loss_bwd", "pred_bwd", "patchify"))(_loss(kind_))
