"""CPU checks of the binding that native.py derives from include/reptext_hip.h: known answers written out from the header text, the
parser's strictness, native.call, and that the model files and ops.ip_attention reach the library through the same host checks."""
import ctypes as C

import pytest
import torch

I32, I64, F32, VP = C.c_int32, C.c_int64, C.c_float, C.c_void_p


def test_parser_known_answers():
    """argtypes typed here by hand from the prototypes in the header, against what the parser derived."""
    from reptext_amd import native

    P = C.POINTER
    want = {
        # (hi, lo, lda, M, K, const rt_skinny_group* groups, ngroups, stream): a struct pointer mid-list
        "rt_gemm_skinny_bf16": [VP, VP, I64, I32, I32, P(native.SkinnyGroup), I32, VP],
        # (q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, row_lo, row_hi, ws, ws_bytes, stream)
        "rt_attention_fwd_rows": [VP, VP, VP, VP, I64, I64, I64, I64, I32, I32, I32, F32, I32, I32, VP, I64, VP],
        # (q, ldq, stride_qb, wq, k, v, ldkv, stride_kvb, gate, stride_gb, o, ldo, stride_ob, o_f32, accumulate, B, N, H, n_ip,
        #  sm_scale, ip_scale, eps, stream)
        "rt_ip_attention_gated": [VP, I64, I64, VP, VP, VP, I64, I64, VP, I64, VP, I64, I64, I32, I32, I32, I32, I32, I32, F32, F32, F32, VP],
        # (ids, cos_out, sin_out, S, const int32_t* axes_dim /* host */, theta, stream)
        "rt_rope_table": [VP, VP, VP, I32, VP, F32, VP],
        # (const rt_ln_segment* segs, x_f32, D, eps, stream)
        "rt_layernorm_modulate_pair": [P(native.LnSegment), I32, I32, F32, VP],
        "rt_canny_ws_bytes": [I32, I32],
        "rt_version": [],
    }
    assert len(want["rt_ip_attention_gated"]) == 23
    for name, argtypes in want.items():
        assert native.SIGNATURES[name] == argtypes, name
    assert native.RESTYPES["rt_canny_ws_bytes"] is C.c_int64 and native.RESTYPES["rt_version"] is C.c_char_p
    assert native.RESTYPES["rt_gemm_skinny_bf16"] is C.c_int and native.RESTYPES["rt_attention_ws_bytes"] is C.c_int64
    assert (native.RT_GEMM_MAX_GROUPS, native.RT_LORA_MAX_TERMS, native.RT_ATTENTION_HD64_MAX_S, native.RT_ATTENTION_HD72_MAX_S) == (4, 8, 4096, 1024)
    assert (native.RT_OK, native.RT_E_BADARG, native.RT_E_ALIGN, native.RT_E_SHAPE) == (0, -1, -2, -3)
    lib = native.load()
    assert native.ABI_VERSION == native.RT_ABI_VERSION == lib.rt_abi_version()
    assert lib.rt_version() == b"reptext_hip abi%d gfx950" % native.ABI_VERSION
    assert lib.rt_gemm_skinny_bf16.argtypes == want["rt_gemm_skinny_bf16"] and lib.rt_canny_ws_bytes.restype is C.c_int64
    assert native.GemmGroup._fields_[:9] == [(n, VP) for n in ("A", "W", "C", "bias", "gate", "res", "add2", "rowscale")] + [("lda", I64)]
    assert native.LoraTerm._fields_ == [("B", VP), ("At", VP), ("ldb", I64), ("lda", I64), ("r_pad", I32), ("scale", F32)]


GOOD = """
/* a comment with a (parenthesis; and a semicolon */
#ifndef X_H
#define X_H
#include <stdint.h>
#define RT_LIMIT 7
#define RT_E_ODD (-9)   /* trailing comment */
typedef struct rt_pair { const void* p; float* f;   /* two pointers */
  int64_t lda, ldb;
  int32_t n; float s; } rt_pair;
int rt_first(const rt_pair* pairs /* host */, int32_t n,
             void* stream);
int64_t rt_second_bytes(void);
#endif
"""


def test_parser_reads_exactly_what_a_small_header_declares():
    from reptext_amd import native

    consts, structs, sigs, res = native.parse_header(GOOD)
    assert consts == {"RT_LIMIT": 7, "RT_E_ODD": -9}
    assert list(structs) == ["rt_pair"] and structs["rt_pair"].__name__ == "Pair"
    assert structs["rt_pair"]._fields_ == [("p", VP), ("f", VP), ("lda", I64), ("ldb", I64), ("n", I32), ("s", F32)]
    assert sigs == {"rt_first": [C.POINTER(structs["rt_pair"]), I32, VP], "rt_second_bytes": []}
    assert res == {"rt_first": C.c_int, "rt_second_bytes": C.c_int64}


@pytest.mark.parametrize("bad", [
    "int rt_f(double x, void* stream);",                                        # an unknown scalar type
    "typedef struct rt_s { double x; } rt_s;",
    "int rt_f(void (*cb)(int32_t), void* stream);",                            # a function-pointer argument
    "typedef struct rt_s { int32_t a : 3; int32_t b; } rt_s;",                 # a bit-field
    "typedef struct rt_s { int32_t a; int64_t b;\nint rt_f(void* stream);",     # an unterminated struct
    "int rt_f(int32_t n[3]);",                                                  # an array declarator
    "int rt_f(int32_t, void* stream);",                                         # an unnamed parameter
    "int rt_f(float** rows);",
    "int rt_f(const rt_unknown* g);",                                           # a struct the header does not define
    "double rt_f(void);",
    "#define RT_SCALE 1.5\nint rt_f(void);",                                    # a define that is no integer
    "#define RT_MAX(a, b) a\nint rt_f(void);",
    "#pragma pack(1)\nint rt_f(void);",
    "int rt_f(void)",                                                           # no terminating semicolon
    "int rt_f(void); static int x = 3;",
], ids=lambda s: s.splitlines()[0][:40])
def test_parser_raises_on_what_it_does_not_recognise(bad):
    from reptext_amd import native

    with pytest.raises(native.HeaderParseError):
        native.parse_header(bad)
    with pytest.raises(native.HeaderParseError):                                 # not skipped among valid declarations either
        native.parse_header(GOOD.replace("int64_t rt_second_bytes(void);", bad + "\nint64_t rt_second_bytes(void);"))


def test_missing_header_is_loud(tmp_path):
    from reptext_amd import native

    with pytest.raises(native.NativeLibraryMissing, match="no_such_header.h not found"):
        native.parse_header_file(str(tmp_path / "no_such_header.h"))
    assert native.parse_header_file(native.HEADER_PATH)[2].keys() == native.SIGNATURES.keys()


def test_call_raises_with_the_header_name_of_the_code():
    from reptext_amd import native

    with pytest.raises((AttributeError, KeyError)):
        native.call("rt_no_such_entry", None)
    with pytest.raises(native.NativeCallError, match="rt_euler_step failed: RT_E_BADARG") as e:
        native.call("rt_euler_step", None, None, 0.0, 10, None)
    assert e.value.code == -1
    g = native.GemmGroup()
    with pytest.raises(native.NativeCallError, match="RT_E_BADARG"):
        native.call("rt_gemm_bf16", C.pointer(g), 1, None)
    with pytest.raises(C.ArgumentError):                                         # typed: a float where the header says int64_t
        native.call("rt_euler_step", None, None, 0.0, 1.5, None)
    assert "hipError 98" in str(native.NativeCallError("rt_x", 98))


@pytest.fixture
def no_native_call(monkeypatch):
    from reptext_amd import native

    def refuse(name, *args):
        raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(native, "call", refuse)


def test_model_file_call_sites_refuse_cpu_tensors_on_the_host(no_native_call, monkeypatch):
    """The raw-pointer sites of encoder_common / mmdit go through ops._dev: a CPU tensor or a wrong dtype is an error before any entry
    point is reached."""
    from reptext_amd import encoder_common, mmdit, ops

    monkeypatch.setattr(ops, "_stream", lambda: 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encoder_common._quick_gelu(torch.zeros(64, dtype=torch.bfloat16))
    ws = type("W", (), dict(T=4, N=8, B=1, x=torch.zeros(1, 12, 64), xn=torch.zeros(1, 12, 64, dtype=torch.bfloat16)))()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mmdit.image_rows_bf16(ws)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # past the device check: the dtype check
    with pytest.raises(TypeError, match="expected torch.bfloat16"):
        encoder_common._quick_gelu(torch.zeros(64))
    ws.xn = torch.zeros(1, 12, 64, dtype=torch.float16)
    with pytest.raises(TypeError, match="expected torch.bfloat16"):
        mmdit.image_rows_bf16(ws)


def test_ip_attention_is_the_gated_op_without_a_gate(monkeypatch):
    """ops.ip_attention(...) and ops.ip_attention_gated(..., gate=None) make the same native call: rt_ip_attention_gated with a null gate,
    to which the C entry rt_ip_attention forwards. Host tensors stand in for device ones (the device check is what is patched out)."""
    from reptext_amd import native, ops

    calls = []
    monkeypatch.setattr(native, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, "_stream", lambda: 0x50)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    B, N, H, n = 2, 24, 2, 4
    d = H * 128
    qkv = torch.zeros(B, N, 3 * d, dtype=torch.bfloat16)
    wq = torch.zeros(128, dtype=torch.bfloat16)
    for kv, out in ((torch.zeros(B, n, 2 * d, dtype=torch.bfloat16), torch.zeros(B, N, d)),
                    (torch.zeros(1, n, 2 * d, dtype=torch.bfloat16), torch.zeros(B, N, d, dtype=torch.bfloat16))):
        calls.clear()
        q, k, v = qkv[..., :d], kv[..., :d], kv[..., d:]
        assert ops.ip_attention(q, wq, k, v, out, H, 0.6, True, 0.11, 1e-5) is out
        assert ops.ip_attention_gated(q, wq, k, v, out, H, 0.6, None, True, 0.11, 1e-5) is out
        assert ops.ip_attention_gated(q, wq, k, v, out, H, ip_scale=0.6, gate=None, accumulate=True, scale=0.11, eps=1e-5) is out
        assert len(calls) == 3 and calls[0] == calls[1] == calls[2]
        name, a = calls[0]
        o_f32, skvb = int(out.dtype == torch.float32), (kv.stride(0) if kv.shape[0] == B else 0)
        assert name == "rt_ip_attention_gated" and len(a) == len(native.SIGNATURES[name]) == 23
        assert a == (q.data_ptr(), 3 * d, N * 3 * d, wq.data_ptr(), k.data_ptr(), v.data_ptr(), 2 * d, skvb, None, 0,
                     out.data_ptr(), d, N * d, o_f32, 1, B, N, H, n, 0.11, 0.6, 1e-5, 0x50)
