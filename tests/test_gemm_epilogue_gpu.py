"""rt_gemm_bf16 / rt_gemm_fp8: every epilogue term, batch stride, gate path and store path of csrc/gemm_bf16.hip's epilogue_tile against an
fp64 reference, judged PER ELEMENT, on guarded buffers (NaN where the kernel must not read, a sentinel where it must not write).

Reference (support_kernels.gemm_epilogue_ref): fp64 from the exact values the kernel reads — bf16 / e4m3 operands, fp32 gate, rowscale
and scales, all widened — in the header's order: (acc * a_scale * w_scale) + bias -> GELU-tanh for n >= gelu_from -> gate -> alpha ->
rowscale -> + res -> + add2. It also returns `mag`, the sum of the absolute values of every addend carried through the same scalings.

Bound, per element:
    fp32 output   |got - ref| <= (K + 16) * 2^-23 * mag + gelu_slack
    bf16 output   the same + 2^-8 |ref|                                   (support_kernels.check_bf16's convention)
K * 2^-23 * mag is the classical bound of K fp32 additions in any order with unit roundoff 2^-23 (it covers an MFMA that truncates), the
16 covers the epilogue's fewer than 16 fp32 operations. gelu_slack (GELU columns only) stands for the device exp2 / rcp inside
gelu_tanh_f, which cannot be derived here: see GELU_SLACK.

Shapes: the smallest that reach every path of the 256 x 256 tile with its 64- (bf16) or 128-element (e4m3) K-tile: M = 300 (one full
tile row + 44 ragged rows), K = three K-tiles (both LDS buffers, the loop and the drain), N = 264 (wide store, ragged last tile), 260
(narrow store: N % 8 != 0), 520 (a third tile column)."""
import ctypes

import pytest
import torch

from support_kernels import BF16, F32, NAN, SENT, check_bound, gelu_tanh_ref, gemm_epilogue_ref, same_bits, twice

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
# Worst |gelu_tanh_f(v) - gelu_fp64(v)| over the GELU columns (n >= 132) of the batched_all_terms, batched_rows_per_batch and
# flat_rows_per_batch data, every N, bf16 and e4m3 operands, fp32 output, v = the kernel's own fp32 pre-activation (a launch with the
# bias alone), measured on an MI355X by test_gelu_slack_measurement below (run it with -s; the figure is printed): MEASURED_GELU_ERR.
# The constant is 4x that.
# Measured 5.159e-07 (e4m3 operands, 2 x 200 x 264, max|v| 10.2; bf16 operands 5.147e-07) -> GELU_SLACK 2.064e-06.
MEASURED_GELU_ERR = 5.159e-07
GELU_SLACK = 4 * MEASURED_GELU_ERR
M_FULL, GELU_FROM, ALPHA = 300, 132, 0.75
OPS = ["bf16", "e4m3"]
OUTS = [BF16, F32]
ids_out = lambda dt: "out_bf16" if dt == BF16 else "out_f32"


def K_of(op):
    return 192 if op == "bf16" else 384


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


# ------------------------------------------------------------------------------------------------ data and guarded buffers
def _pad1d(vals, dtype, device, lead=4, tail=4):
    """A 1-D vector inside a longer NaN-filled one (the view starts `lead` elements in: 8 bytes for bf16, 16 for fp32)."""
    buf = torch.full((lead + vals.numel() + tail,), NAN, dtype=dtype)
    buf[lead : lead + vals.numel()] = vals.to(dtype)
    return buf.to(device)[lead : lead + vals.numel()]


def _pad3d(vals, ld, extra_rows, fill, dtype, device, col0=0):
    """[B, R, C] values as a view of a [B, R + extra_rows, ld] buffer filled with `fill` (padded row and batch strides)."""
    B, R, C = vals.shape
    buf = torch.full((B, R + extra_rows, ld), fill, dtype=torch.float32)
    buf[:, :R, col0 : col0 + C] = vals.float()
    buf = buf.to(dtype).to(device)
    return buf, buf[:, :R, col0 : col0 + C]


class Data:
    """One problem's true values on the CPU (exactly what the kernel will read) and their guarded device buffers."""

    def __init__(self, op, B, M, N, seed, gate_rows, rs_shape, device):
        K = K_of(op)
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        ru = lambda *s: torch.rand(*s, generator=g) * 1.5 + 0.25                      # [0.25, 1.75]
        self.op, self.B, self.M, self.N, self.K, self.dev = op, B, M, N, K, device
        a, w = rn(B, M, K), 0.1 * rn(N, K)
        if op == "e4m3":
            self.a_scale, self.w_scale = torch.rand(B * M, generator=g) + 0.5, torch.rand(N, generator=g) * 0.02 + 0.01
            self.a = (a / self.a_scale.view(B, M, 1)).to(FP8)                          # de-quantised: a ~ N(0,1), w ~ 0.1 N(0,1)
            self.w = (w / self.w_scale.view(N, 1)).to(FP8)
        else:
            self.a_scale = self.w_scale = None
            self.a, self.w = a.to(BF16), w.to(BF16)
        self.bias = rn(N).to(BF16)
        sign = torch.where(torch.rand(gate_rows, N, generator=g) < 0.5, -1.0, 1.0)
        self.gate = ru(gate_rows, N) * sign
        self.rowscale = ru(*rs_shape)
        self.res = {BF16: rn(B, M, N).to(BF16)}
        self.res[F32] = self.res[BF16].float() + rn(B, M, N) * 2.0 ** -12              # fp32 residual: not representable in bf16
        self.add2 = rn(B, M, N).to(BF16)
        # ---- device side: every operand a view of a larger NaN-filled buffer
        opdt = FP8 if op == "e4m3" else BF16
        _, self.d_a = _pad3d(self.a, K + 64, 5, NAN, opdt, device)                     # lda > K, rows behind M, padded strideA
        _, wv = _pad3d(self.w[None], K + 64, 5, NAN, opdt, device)                     # ldw > K, rows behind N
        self.d_w = wv[0]
        self.d_bias = _pad1d(self.bias, BF16, device)
        _, gv = _pad3d(self.gate[None], N + 24, 2, NAN, F32, device, col0=8)           # a [rows, N] view of a wider table
        self.d_gate = gv[0]
        if len(rs_shape) == 2:
            _, rv = _pad3d(self.rowscale[None], rs_shape[1] + 20, 1, NAN, F32, device)  # [B, rows], row stride > rows
            self.d_rowscale = rv[0]
        else:
            self.d_rowscale = _pad1d(self.rowscale, F32, device, tail=320)              # an index by m instead of m % rows lands in NaN, inside
        self.d_res = {dt: _pad3d(self.res[dt], N + 16, 2, NAN, dt, device)[1] for dt in (BF16, F32)}     # ldr != ldc, own strideR
        _, self.d_add2 = _pad3d(self.add2, N + 24, 1, NAN, BF16, device)                # own ld2 / stride2
        if op == "e4m3":
            self.d_a_scale, self.d_w_scale = _pad1d(self.a_scale, F32, device), _pad1d(self.w_scale, F32, device)

    def flat(self):
        """The 2-D form of a B = 1 problem's operand."""
        return self.d_a[0]

    def kwargs(self, terms, out_dtype, rows_per_batch=0, res=None):
        """(ops.LinearProblem keywords, gemm_epilogue_ref keywords) with the given subset of the seven terms switched on."""
        kw, rk = {}, {}
        if self.op == "e4m3":
            kw.update(a_scale=self.d_a_scale, w_scale=self.d_w_scale)
            rk.update(a_scale=self.a_scale, w_scale=self.w_scale)
        if "bias" in terms:
            kw["bias"], rk["bias"] = self.d_bias, self.bias
        if "gelu" in terms:
            kw["gelu_from"] = rk["gelu_from"] = GELU_FROM
        if "gate" in terms:
            kw["gate"], rk["gate"] = self.d_gate, self.gate
        if "alpha" in terms:
            kw["alpha"] = rk["alpha"] = ALPHA
        if "rowscale" in terms:
            kw["rowscale"], rk["rowscale"] = self.d_rowscale, self.rowscale
        if "res" in terms:
            kw["res"], rk["res"] = (self.d_res[out_dtype] if res is None else res), self.res[out_dtype]
        if "add2" in terms:
            kw["add2"], rk["add2"] = self.d_add2, self.add2
        if rows_per_batch:
            kw["rows_per_batch"] = rk["rows_per_batch"] = rows_per_batch
        return kw, rk


ALL = ("bias", "gelu", "gate", "alpha", "rowscale", "res", "add2")
_DATA = {}


def data(op, B, M, N, seed, gate_rows, rs_shape, device):
    key = (op, B, M, N, seed, gate_rows, tuple(rs_shape))
    if key not in _DATA:
        _DATA[key] = Data(op, B, M, N, seed, gate_rows, rs_shape, device)
    return _DATA[key]


def all_terms_data(op, N, device):
    """batched_all_terms: [3, 300, K], gate [3, N], rowscale [3, 300]; the three batch entries hold different data."""
    return data(op, 3, M_FULL, N, 100 + N, 3, (3, M_FULL), device)


_REF = {}


def reference(d, rk):
    """(ref, mag) of a problem, computed once per (data, keyword set) and shared."""
    key = (id(d), tuple(sorted((k, id(v) if isinstance(v, torch.Tensor) else v) for k, v in rk.items())))
    if key not in _REF:
        _REF[key] = gemm_epilogue_ref(d.a.float(), d.w.float(), **rk)
    return _REF[key]


def bound_of(ref, mag, K, out_dtype, gelu_from):
    b = (K + 16) * 2.0 ** -23 * mag
    if gelu_from is not None and gelu_from < ref.shape[-1]:
        b[..., max(gelu_from, 0):] += GELU_SLACK
    if out_dtype == BF16:
        b = b + 2.0 ** -8 * ref.abs()
    return b


def new_out(B, M, N, out_dtype, device, ldc=None, col0=0, init=None):
    """A sentinel-filled [B, M + 3, ldc] buffer and its [B, M, N] view at column col0 (`init`: values the view holds first)."""
    ldc = N + 8 if ldc is None else ldc
    return _pad3d(torch.full((B, M, N), SENT) if init is None else init, ldc, 3, SENT, out_dtype, device, col0=col0)


def guards_intact(buf, M, N, col0=0):
    """Everything of every batch entry of the guarded output outside [:M, col0 : col0 + N] still holds the sentinel."""
    m = torch.ones(buf.shape[1:], dtype=torch.bool, device=buf.device)
    m[:M, col0 : col0 + N] = False
    return all(same_bits(buf[b][m], torch.full_like(buf[b][m], SENT)) for b in range(buf.shape[0]))


def launch(ops, d, a_view, terms, out_dtype, rows_per_batch=0, ldc=None, col0=0, alias_res=False, batched_out=True):
    """One guarded launch through `twice`; returns (whole output buffer, its [B, M, N] part, reference keywords)."""
    B, M, N = d.B, d.M, d.N

    def run():
        buf, view = new_out(B, M, N, out_dtype, d.dev, ldc, col0, init=d.res[out_dtype] if alias_res else None)
        ov = view if batched_out else view[0]
        kw, _ = d.kwargs(terms, out_dtype, rows_per_batch, res=ov if alias_res else None)
        ops.linear(a_view, d.d_w, ov, **kw)
        torch.cuda.synchronize()
        return buf

    buf = twice(run)
    assert guards_intact(buf, M, N, col0), "wrote outside [:M, :N] of a batch entry"
    return buf, buf[:, :M, col0 : col0 + N], d.kwargs(terms, out_dtype, rows_per_batch)[1]


def run_and_check(what, ops, d, a_view, terms, out_dtype, **kw):
    buf, got, rk = launch(ops, d, a_view, terms, out_dtype, **kw)
    ref, mag = reference(d, rk)
    check_bound(what, got, ref, bound_of(ref, mag, d.K, out_dtype, rk.get("gelu_from")))
    return got


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", [264, 260, 520])
def test_batched_all_terms(ops, gpu, N, op, out_dtype):
    """a [3, 300, K] with a padded strideA, out with a padded strideC, res a different tensor (ldr != ldc, own strideR), add2 with its own
    ld2 / stride2, gate a [3, N] view of a wider table, rowscale [3, 300] with a row stride > 300, bias, alpha, gelu_from = 132."""
    d = all_terms_data(op, N, gpu)
    run_and_check(f"batched_all_terms {op} N={N} {ids_out(out_dtype)}", ops, d, d.d_a, ALL, out_dtype)


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", [264, 260])
def test_batched_rows_per_batch(ops, gpu, N, op, out_dtype):
    """a [2, 200, K] with rows_per_batch = 100: gate [4, N] (index bidx * (M / rpb) + m / rpb), one rowscale [100] shared."""
    d = data(op, 2, 200, N, 200 + N, 4, (100,), gpu)
    run_and_check(f"batched_rows_per_batch {op} N={N} {ids_out(out_dtype)}", ops, d, d.d_a, ALL, out_dtype, rows_per_batch=100)


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", [264, 520])
def test_flat_rows_per_batch(ops, gpu, N, op, out_dtype):
    """2-D a with M = 300 and rows_per_batch = 100 (both tile rows straddle gate rows), res aliasing out."""
    d = data(op, 1, M_FULL, N, 300 + N, 3, (100,), gpu)
    run_and_check(f"flat_rows_per_batch {op} N={N} {ids_out(out_dtype)}", ops, d, d.flat(), ALL, out_dtype, rows_per_batch=100,
                  alias_res=True, batched_out=False)


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
def test_narrow_store_by_alignment(ops, gpu, op, out_dtype):
    """N = 264 stored wide (ldc = N + 8, C 16-byte aligned), narrow because ldc % 8 == 4, and (bf16 output: an fp32 C must be 16-byte
    aligned) narrow because C is a column-offset view that is only 8-byte aligned: the same bits each time, and the fp64 bound."""
    N = 264
    d = all_terms_data(op, N, gpu)
    what = f"narrow_store {op} {ids_out(out_dtype)}"
    wide = run_and_check(what + " ldc=N+8", ops, d, d.d_a, ALL, out_dtype)
    by_ld = run_and_check(what + " ldc=N+4", ops, d, d.d_a, ALL, out_dtype, ldc=N + 4)
    assert same_bits(by_ld, wide)
    if out_dtype == BF16:
        by_ptr = run_and_check(what + " ldc=N+16, C + 8 bytes", ops, d, d.d_a, ALL, out_dtype, ldc=N + 16, col0=4)
        assert by_ptr.data_ptr() % 16 == 8
        assert same_bits(by_ptr, wide)


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
def test_one_term_at_a_time(ops, gpu, op, out_dtype):
    """The batched_all_terms data with exactly one of the seven terms enabled: pins which buffer each pointer reads."""
    d = all_terms_data(op, 264, gpu)
    for term in ALL:
        run_and_check(f"one_term {term} {op} {ids_out(out_dtype)}", ops, d, d.d_a, (term,), out_dtype)


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
def test_four_groups(ops, gpu, op, out_dtype):
    """RT_GEMM_MAX_GROUPS problems with different (M, N) and terms in one launch, the batch = 2 problem third: each result equals the
    same problem launched alone bit for bit, stays inside its own guarded buffer, and meets the fp64 bound."""
    from reptext_amd import native

    assert native.RT_GEMM_MAX_GROUPS == 4
    specs = [  # data, terms, rows_per_batch
        (data(op, 1, 300, 264, 41, 3, (100,), gpu), ("bias", "gelu", "gate", "res"), 100),
        (data(op, 1, 64, 520, 42, 1, (64,), gpu), ("bias", "alpha", "add2"), 0),
        (data(op, 2, 130, 264, 43, 2, (2, 130), gpu), ("bias", "gate", "rowscale", "res", "gelu"), 0),
        (data(op, 1, 257, 260, 44, 1, (257,), gpu), ("gelu", "alpha", "rowscale", "add2"), 0),
    ]

    def run(grouped):
        bufs, problems = [], []
        for d, terms, rpb in specs:
            buf, view = new_out(d.B, d.M, d.N, out_dtype, gpu)
            kw, _ = d.kwargs(terms, out_dtype, rpb)
            problems.append(ops.LinearProblem(d.d_a, d.d_w, view, **kw))
            bufs.append(buf)
        if grouped:
            ops.linear_grouped(problems)
        else:
            for p in problems:
                ops.linear_grouped([p])
        torch.cuda.synchronize()
        return bufs

    together = twice(lambda: run(True))
    alone = run(False)
    for i, ((d, terms, rpb), buf, ref_buf) in enumerate(zip(specs, together, alone)):
        assert guards_intact(buf, d.M, d.N), f"group {i} wrote outside its output"
        assert same_bits(buf, ref_buf), f"group {i} differs from the same problem launched alone"
        rk = d.kwargs(terms, out_dtype, rpb)[1]
        ref, mag = reference(d, rk)
        check_bound(f"four_groups[{i}] {d.B}x{d.M}x{d.N} {op} {ids_out(out_dtype)}", buf[:, : d.M, : d.N], ref,
                    bound_of(ref, mag, d.K, out_dtype, rk.get("gelu_from")))


@pytest.mark.parametrize("out_dtype", OUTS, ids=ids_out)
@pytest.mark.parametrize("op", OPS)
def test_unaligned_gelu_from(ops, gpu, op, out_dtype):
    """gelu_from = 130: the epilogue decides n >= gelu_from once per 4-column group, so columns 130 and 131 would stay un-activated. The C
    entry refuses it with RT_E_SHAPE, ops.linear raises, and the guarded output is untouched. (Were the call not refused, the fp64
    comparison below reports what the kernel made of those columns.)"""
    from reptext_amd import native

    d = all_terms_data(op, 264, gpu)
    buf, view = new_out(d.B, d.M, d.N, out_dtype, gpu)
    kw, rk = d.kwargs(("bias", "gelu"), out_dtype)
    grp = ops.LinearProblem(d.d_a, d.d_w, view, **kw).to_group()
    grp.gelu_from = 130
    lib = native.load()
    entry = lib.rt_gemm_fp8 if op == "e4m3" else lib.rt_gemm_bf16
    rc = entry(ctypes.pointer(grp), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc == 0:
        ref, mag = gemm_epilogue_ref(d.a.float(), d.w.float(), **dict(rk, gelu_from=130))
        check_bound(f"unaligned_gelu_from {op} {ids_out(out_dtype)}: accepted, columns 130..131", buf[:, : d.M, 130:132], ref[..., 130:132],
                    bound_of(ref, mag, d.K, out_dtype, 130)[..., 130:132])
    assert rc == -3, f"gelu_from = 130 returned {rc}, expected RT_E_SHAPE"
    with pytest.raises(ValueError, match="gelu_from"):
        ops.linear(d.d_a, d.d_w, view, **dict(kw, gelu_from=130))
    torch.cuda.synchronize()
    assert same_bits(buf, torch.full_like(buf, SENT)), "a refused call wrote to its output"


def test_gelu_slack_measurement(ops, gpu):
    """The figure behind GELU_SLACK: |gelu_tanh_f(v) - gelu_fp64(v)| with v the kernel's own fp32 value of acc + bias (a launch without the
    activation; launches are bitwise repeatable), so that nothing but the device exp2 / rcp and the final fp32 operations is in it.
    Prints the worst value over the GELU columns of the cases' data and asserts it is inside the constant."""
    worst = 0.0
    for op in OPS:
        for d in [all_terms_data(op, N, gpu) for N in (264, 260, 520)] + [data(op, 2, 200, N, 200 + N, 4, (100,), gpu) for N in (264, 260)] + \
                 [data(op, 1, M_FULL, N, 300 + N, 3, (100,), gpu) for N in (264, 520)]:
            _, pre, _ = launch(ops, d, d.d_a, ("bias",), F32)
            _, act, _ = launch(ops, d, d.d_a, ("bias", "gelu"), F32)
            assert same_bits(act[..., :GELU_FROM], pre[..., :GELU_FROM])
            e = float((act[..., GELU_FROM:].double() - gelu_tanh_ref(pre[..., GELU_FROM:])).abs().max())
            print(f"[gelu] {op} {d.B}x{d.M}x{d.N}: worst |gelu_tanh_f(v) - gelu_fp64(v)| {e:.3e}, max|v| {float(pre[..., GELU_FROM:].abs().max()):.2f}")
            worst = max(worst, e)
    print(f"[gelu] worst over all: {worst:.3e}  (MEASURED_GELU_ERR {MEASURED_GELU_ERR:.3e}, GELU_SLACK {GELU_SLACK:.3e})")
    assert worst <= GELU_SLACK
