"""CPU checks of the entry points added for the loop's small passes (rt_gemm_skinny_bf16, rt_layernorm_modulate_pair,
rt_add_rows_f32): struct layouts against the header, and argument validation that returns RT_E_* before any launch."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, ALIGN, SHAPE = -1, -2, -3


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from reptext_amd import native

    return native, native.load()


def test_struct_layouts_match_c(tmp_path):
    native, _ = _lib()
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "reptext_hip.h"
int main(){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rt_skinny_group), offsetof(rt_skinny_group, bias), offsetof(rt_skinny_group, C),
         offsetof(rt_skinny_group, ldw), offsetof(rt_skinny_group, ldc), offsetof(rt_skinny_group, N));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_ln_segment), offsetof(rt_ln_segment, out), offsetof(rt_ln_segment, scale),
         offsetof(rt_ln_segment, ldx), offsetof(rt_ln_segment, mod_ld), offsetof(rt_ln_segment, batch), offsetof(rt_ln_segment, rows_per_batch));
  return 0; }
'''
    src, exe = str(tmp_path / "_layout2.c"), str(tmp_path / "_layout2")
    open(src, "w").write(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    a, b = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    S, L = native.SkinnyGroup, native.LnSegment
    assert [int(x) for x in a.split()] == [ctypes.sizeof(S), S.bias.offset, S.C.offset, S.ldw.offset, S.ldc.offset, S.N.offset]
    assert [int(x) for x in b.split()] == [ctypes.sizeof(L), L.out.offset, L.scale.offset, L.ldx.offset, L.mod_ld.offset, L.batch.offset,
                                           L.rows_per_batch.offset]


def _skinny_group(native, **kw):
    g = native.SkinnyGroup()
    g.W, g.bias, g.C, g.ldw, g.ldc, g.N = 0x1000, 0x2000, 0x3000, 3072, 9216, 9216      # never dereferenced: every call below is rejected
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_skinny_gemm_rejects_bad_arguments():
    native, lib = _lib()
    call = lambda g, hi=0x4000, lo=0x5000, lda=3072, M=28, K=3072, n=1: lib.rt_gemm_skinny_bf16(hi, lo, lda, M, K, ctypes.pointer(g), n, None)
    ok = _skinny_group(native)
    assert call(ok, hi=None) == BADARG
    assert call(ok, lo=None) == BADARG
    assert lib.rt_gemm_skinny_bf16(0x4000, 0x5000, 3072, 28, 3072, None, 1, None) == BADARG
    assert call(ok, n=3) == BADARG
    assert call(ok, M=0) == BADARG
    assert call(ok, M=33) == SHAPE                              # more than two 16-row fragments
    assert call(ok, K=3072 + 64, lda=3072 + 64) == SHAPE        # K % 256
    assert call(ok, lda=3064) == SHAPE                          # lda < K
    assert call(ok, hi=0x4008) == ALIGN
    assert call(ok, lda=3076) == ALIGN
    assert call(_skinny_group(native, W=None)) == BADARG
    assert call(_skinny_group(native, C=None)) == BADARG
    assert call(_skinny_group(native, N=9224, ldc=9224)) == SHAPE   # N % 16
    assert call(_skinny_group(native, ldc=9000)) == SHAPE           # ldc < N
    assert call(_skinny_group(native, ldw=3000)) == SHAPE           # ldw < K
    assert call(_skinny_group(native, W=0x1008)) == ALIGN
    assert call(_skinny_group(native, C=0x3004)) == ALIGN
    assert call(_skinny_group(native, bias=0x2002)) == ALIGN


def test_layernorm_pair_and_add_rows_reject_bad_arguments():
    native, lib = _lib()

    def segs(**kw):
        a = (native.LnSegment * 2)()
        for g in a:
            g.x, g.out, g.shift, g.scale = 0x1000, 0x2000, 0x3000, 0x4000
            g.ldx = g.ldo = 3072
            g.mod_ld, g.batch, g.rows_per_batch = 18432, 1, 512
        for k, v in kw.items():
            setattr(a[1], k, v)
        return a

    call = lambda a, D=3072: lib.rt_layernorm_modulate_pair(a, 1, D, 1e-6, None)
    assert lib.rt_layernorm_modulate_pair(None, 1, 3072, 1e-6, None) == BADARG
    assert call(segs(x=None)) == BADARG
    assert call(segs(out=None)) == BADARG
    assert call(segs(rows_per_batch=0)) == BADARG
    assert call(segs(shift=None)) == BADARG                       # shift and scale come together
    assert call(segs(), D=3076) == SHAPE
    assert call(segs(), D=16384) == SHAPE
    assert call(segs(x=0x1008)) == ALIGN
    assert call(segs(ldo=3076)) == ALIGN
    assert call(segs(mod_ld=18433)) == ALIGN

    assert lib.rt_add_rows_f32(None, 0x1000, None, 28, 1, 3072, None) == BADARG
    assert lib.rt_add_rows_f32(0x1000, None, None, 28, 1, 3072, None) == BADARG
    assert lib.rt_add_rows_f32(0x1000, 0x2000, None, 0, 1, 3072, None) == BADARG
    assert lib.rt_add_rows_f32(0x1000, 0x2000, None, 28, 1, 3074, None) == SHAPE
    assert lib.rt_add_rows_f32(0x1004, 0x2000, None, 28, 1, 3072, None) == ALIGN
    assert lib.rt_add_rows_f32(0x1000, 0x2000, 0x3008, 28, 1, 3072, None) == ALIGN


def test_qk_norm_entries_reject_misaligned_norm_weights():
    """rt_qk_rmsnorm_rope and rt_attention_fp8_prep load all four norm weights as 16-byte vectors: the image weights always, the text
    weights when T > 0. A weight that is not 16-byte aligned is refused with RT_E_ALIGN before anything is queued; with T = 0 the text
    weights are not looked at. Made-up pointers, never dereferenced."""
    _, lib = _lib()
    buf, cos, sin, qk8, vt8 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    W = dict(wq_txt=0x1000, wk_txt=0x1100, wq_img=0x1200, wk_img=0x1300)

    def norm(T=8, **kw):
        w = dict(W, **kw)
        return lib.rt_qk_rmsnorm_rope(buf, 392, 392 * 16, 0, 128, w["wq_txt"], w["wk_txt"], w["wq_img"], w["wk_img"], cos, sin, 1, 16, T, 1, 1e-6, None)

    def prep(T=8, **kw):
        w = dict(W, **kw)
        return lib.rt_attention_fp8_prep(buf, 392, 392 * 16, 0, 128, 256, w["wq_txt"], w["wk_txt"], w["wq_img"], w["wk_img"], cos, sin, qk8, vt8,
                                         1, 16, T, 1, 1e-6, None)

    for call in (norm, prep):
        for name in W:
            assert call(**{name: W[name] + 8}) == ALIGN, (call.__name__, name)
            assert call(**{name: W[name] + 2}) == ALIGN, (call.__name__, name)
        assert call(wq_txt=None) == BADARG and call(wk_txt=None) == BADARG           # T > 0 needs them
        assert call(T=0, wq_img=W["wq_img"] + 8) == ALIGN and call(T=0, wk_img=W["wk_img"] + 8) == ALIGN
    # Only refusals are exercised: every call above returns before the launch. That T = 0 accepts text weights of any alignment (or
    # none) is what the T = 0 cases of test_token_passes_gpu.py and test_e4m3_producers_gpu.py run, with real buffers.


def test_rope_fields_layout_and_rejections(tmp_path):
    """rt_gemm_group's fused q/k fields: offsets against the header; all-zero = no fused step; bad descriptions are rejected."""
    native, lib = _lib()
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "reptext_hip.h"
int main(){ printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rt_gemm_group), offsetof(rt_gemm_group, rope_cos), offsetof(rt_gemm_group, rope_wk),
  offsetof(rt_gemm_group, rope_q0), offsetof(rt_gemm_group, rope_w), offsetof(rt_gemm_group, rope_pos0), offsetof(rt_gemm_group, rope_eps)); return 0; }
'''
    src, exe = str(tmp_path / "_layout3.c"), str(tmp_path / "_layout3")
    open(src, "w").write(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    G = native.GemmGroup
    assert [int(x) for x in out] == [ctypes.sizeof(G), G.rope_cos.offset, G.rope_wk.offset, G.rope_q0.offset, G.rope_w.offset, G.rope_pos0.offset,
                                     G.rope_eps.offset]

    def group(**kw):
        g = native.GemmGroup()
        g.A, g.W, g.C, g.bias = 0x10000, 0x20000, 0x30000, 0x40000
        g.M, g.N, g.K, g.batch = 512, 1536, 512, 1
        g.lda = g.ldw = 512
        g.ldc, g.gelu_from, g.alpha = 1536, 1536, 1.0
        g.rope_cos, g.rope_sin, g.rope_wq, g.rope_wk = 0x50000, 0x60000, 0x70000, 0x80000
        g.rope_q0, g.rope_k0, g.rope_w, g.rope_eps = 0, 512, 512, 1e-6
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    call = lambda g: lib.rt_gemm_bf16(ctypes.pointer(g), 1, None)
    assert call(group(rope_sin=None)) == BADARG
    assert call(group(rope_wq=None)) == BADARG
    assert call(group(rope_wk=None)) == BADARG
    assert call(group(out_f32=1)) == BADARG
    assert call(group(gate=0x90000)) == BADARG
    assert call(group(alpha=0.5)) == BADARG
    assert call(group(rope_q0=128)) == SHAPE                      # not tile-aligned
    assert call(group(rope_w=384)) == SHAPE
    assert call(group(rope_k0=256)) == SHAPE                      # overlaps q
    assert call(group(rope_k0=1280)) == SHAPE                     # runs past N
    assert call(group(gelu_from=768)) == SHAPE                    # GELU inside k
    assert call(group(rope_cos=0x50004)) == ALIGN
    assert call(group(rope_wk=0x80008)) == ALIGN
    assert call(group(ldc=1540)) == ALIGN
    assert lib.rt_gemm_fp8(ctypes.pointer(group(K=512)), 1, None) == BADARG


def test_gemm_rejects_gelu_from_inside_a_column_group():
    """The epilogue decides `n >= gelu_from` once per 4-column group of a lane: a first GELU column inside (0, N) that is no multiple
    of 4 is refused by both entries before anything is queued; <= 0 (all columns), >= N (none) and multiples of 4 are not."""
    native, lib = _lib()

    def group(**kw):
        g = native.GemmGroup()
        g.A, g.W, g.C = 0x10000, 0x20000, 0x30000                     # never dereferenced: every call below is rejected
        g.M, g.N, g.K, g.batch = 300, 264, 384, 1
        g.lda = g.ldw = 384
        g.ldc, g.alpha = 264, 1.0
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    for entry in (lib.rt_gemm_bf16, lib.rt_gemm_fp8):
        call = lambda g: entry(ctypes.pointer(g), 1, None)
        assert call(group(gelu_from=130)) == SHAPE
        assert call(group(gelu_from=1)) == SHAPE
        assert call(group(gelu_from=263)) == SHAPE
        # the accepted values must get past this rule: a LATER check stops them (C not 8-byte aligned), the rule itself stops 130
        assert call(group(gelu_from=130, C=0x30004)) == SHAPE
        for ok in (-3, 0, 132, 264, 265, 1000):
            assert call(group(gelu_from=ok, C=0x30004)) == ALIGN, ok

