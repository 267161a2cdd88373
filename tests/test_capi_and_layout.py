"""CPU checks of the boundary: the shared library loads without a GPU, exports every symbol include/reptext_hip.h
declares, the ctypes binding covers exactly that set, struct layouts agree, and the product never touches oracle/.
The binding itself (parser known answers, strictness, native.call) is tested in tests/test_native_binding_host.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "arabic-text-image-generation-reptext_amd")
HEADER = os.path.join(ROOT, "include", "reptext_hip.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    import __graft_entry__ as ge

    ge.build()
    from reptext_amd import native

    lib = native.load()
    assert lib.rt_version().startswith(b"reptext_hip")
    syms = header_symbols()
    assert len(syms) >= 24
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in reptext_hip.h but not exported"
    bound = set(native.SIGNATURES) | {"rt_version"}
    assert bound == set(syms), f"binding/header mismatch: {bound ^ set(syms)}"


def test_gemm_group_struct_layout_matches_c(tmp_path):
    """Compile a tiny host program against the header and compare sizeof and the offsetof of EVERY field of every struct with the
    ctypes classes the binding generates (the field list of the program comes from those classes)."""
    from reptext_amd import native

    assert set(native.STRUCTS) == {"rt_gemm_group", "rt_skinny_group", "rt_ln_segment", "rt_lora_term"}
    assert [native.STRUCTS[n] for n in sorted(native.STRUCTS)] == [native.GemmGroup, native.LnSegment, native.LoraTerm, native.SkinnyGroup]
    fields = [(c, f) for c, cls in native.STRUCTS.items() for f, _ in cls._fields_]
    assert len(fields) == 56 + 7 + 11 + 6                                       # counted in the header
    lines = [f'printf("%zu\\n", sizeof({c}));' for c in native.STRUCTS] + [f'printf("%zu\\n", offsetof({c}, {f}));' for c, f in fields]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "reptext_hip.h"\nint main(){\n' + "\n".join(lines) + "\nreturn 0; }\n"
    src, exe = str(tmp_path / "_layout.c"), str(tmp_path / "_layout")
    open(src, "w").write(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(cls) for cls in native.STRUCTS.values()] + [getattr(native.STRUCTS[c], f).offset for c, f in fields]
    assert out == want, [(cf, a, b) for cf, a, b in zip(list(native.STRUCTS) + fields, out, want) if a != b]
    G = native.GemmGroup
    assert (ctypes.sizeof(G), G.lda.offset, G.strideA.offset, G.M.offset, G.out_f32.offset, G.alpha.offset) == (360, 64, 112, 144, 168, 172)


def test_calls_are_rejected_not_crashed_without_gpu_memory():
    """Argument validation happens on the host before any launch: null pointers / bad shapes return RT_E_* codes."""
    from reptext_amd import native

    lib = native.load()
    g = native.GemmGroup()
    assert lib.rt_gemm_bf16(ctypes.pointer(g), 1, None) == -1            # RT_E_BADARG (null A/W/C)
    assert lib.rt_gemm_bf16(ctypes.pointer(g), 9, None) == -1            # too many groups
    assert lib.rt_euler_step(None, None, 0.0, 10, None) == -1
    assert lib.rt_layernorm_modulate(8, 8, 0, 0, 8, 8, 0, None, None, 0, 1, 1, 12, 1e-6, None) in (-2, -3)   # D % 8 != 0


def test_conv2d_rejects_a_misaligned_bias_or_res_whichever_kernel_serves_the_call():
    """rt_conv2d_nhwc: both of its kernels load 4 channels of bias and of res as one 8-byte word. A bias or res that is not 8-byte
    aligned is RT_E_ALIGN from the entry point itself, before anything is queued (null stream, fake pointers, no GPU) — for the calls
    the GEMM's convolution form takes and for those conv_nhwc_kernel takes (fp32 output, stride 2, upsample, Cout < 64, variant 0)."""
    from reptext_amd import native

    lib = native.load()
    X, W, Y, OK8, ODD = 0x10000, 0x20000, 0x30000, 0x40008, 0x40004
    #        Cout ks stride up out_f32
    calls = [(128, 3, 1, 0, 0), (260, 1, 1, 0, 0), (4, 3, 1, 0, 1), (128, 3, 2, 0, 0), (128, 3, 1, 1, 0), (32, 3, 1, 0, 0)]
    prev = lib.rt_conv2d_variant(-1)
    try:
        for mode in (1, 0):
            lib.rt_conv2d_variant(mode)
            for Cout, ks, stride, up, f32 in calls:
                shape = (2, 8, 8, 64, Cout, ks, stride, up, f32, None)
                assert lib.rt_conv2d_nhwc(X, W, ODD, None, Y, *shape) == native.RT_E_ALIGN, (mode, Cout, ks, stride, up, f32, "bias")
                assert lib.rt_conv2d_nhwc(X, W, None, ODD, Y, *shape) == native.RT_E_ALIGN, (mode, Cout, ks, stride, up, f32, "res")
                assert lib.rt_conv2d_nhwc(X, W, OK8, ODD + 2, Y, *shape) == native.RT_E_ALIGN, (mode, Cout, ks, stride, up, f32, "res + 2")
                assert lib.rt_conv2d_nhwc(X + 8, W, OK8, OK8, Y, *shape) == native.RT_E_ALIGN        # x / w / y keep their 16 bytes
            assert lib.rt_conv2d_nhwc(X, W, ODD, ODD, Y, 2, 8, 8, 64, 130, 3, 1, 0, 0, None) == native.RT_E_SHAPE   # the shape is judged first
            assert lib.rt_conv2d_nhwc(None, W, ODD, ODD, Y, 2, 8, 8, 64, 128, 3, 1, 0, 0, None) == native.RT_E_BADARG
    finally:
        lib.rt_conv2d_variant(prev)


def test_product_never_imports_the_oracle_and_has_no_cpu_fallback():
    bad = []
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "oracle." in txt and f.endswith(".py") and "import oracle" in txt:
                    bad.append(f)
    for f in ("controlnet_flux.py", "pipeline_flux_controlnet.py", "pipeline_flux_controlnet_inpaint.py", "reptext_amd.py"):
        p = os.path.join(ROOT, f)
        if os.path.exists(p) and re.search(r"^\s*(from|import)\s+oracle\b", open(p).read(), flags=re.M):
            bad.append(f)
    assert not bad, f"product files import the oracle: {bad}"


def test_ops_refuse_cpu_tensors():
    import torch

    import reptext_amd.ops as ops

    a = torch.zeros(64, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(a, a, a.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.euler_step_(a.clone(), a, 0.1)


def test_missing_library_is_loud(monkeypatch):
    from reptext_amd import native

    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "LIB_PATH", "/nonexistent/librt_reptext_hip.so")
    with pytest.raises(native.NativeLibraryMissing):
        native.load()


def test_attention_v3_code_object_keeps_out_of_the_asm_owned_registers():
    """csrc/attention_v3.hip names the accumulator registers a0..a191 literally (O and Q live there for a whole work item). The
    compiler must not have put anything of its own in them: no VGPR spill, no scratch, no compiler-generated v_accvgpr_* that
    names a0..a191 (tools/audit_v3_asm.py over the -S output of the same flags the Makefile builds with)."""
    import shutil
    import subprocess

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "audit_v3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "OK " in r.stdout


# (B, S, H) -> rt_attention_ws_bytes on a 256-CU device, recorded from the library as it was BEFORE the key-split geometry of
# csrc/attention.hip and csrc/attention_v3.hip moved into csrc/attention_split.h. The larger of the two kernels' needs: counters
# for 128-row items + two records per splitting workgroup (67 584-B records on 64 workgroups per XCD group in attention.hip,
# 135 168-B records on 32 in attention_v3: the same record bytes; S = 4500 is attention.hip's alone). 0: nothing splits.
ATTENTION_WS_BYTES_256CU = {
    (1, 4608, 24): 69209600,
    (3, 4608, 24): 207628544,
    (1, 4500, 24): 69209600,
    (1, 4608, 2): 69206528,
    (1, 4608, 4): 69206784,
    (1, 2304, 8): 69206784,
    (2, 2304, 7): 138413056,
    (1, 2048, 8): 69206528,
    (1, 9728, 24): 69213440,
    (1, 1536, 24): 69207296,
    (1, 768, 3): 0,
    (1, 1024, 24): 0,
    (1, 128, 1): 0,
    (1, 200, 2): 0,
    (0, 4608, 24): 0,
}


def test_attention_workspace_bytes_are_the_same_function_of_the_shape():
    """The split geometry (cut rule, counter region, records per workgroup) decides the workspace size; it is a function of
    (B, S, H, CU count) only. Without a device the CU query falls back to 256, the MI355X count."""
    import torch

    from reptext_amd import native

    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the recorded sizes are those of a 256-CU device")
    lib = native.load()
    got = {shape: lib.rt_attention_ws_bytes(*shape) for shape in ATTENTION_WS_BYTES_256CU}
    assert got == ATTENTION_WS_BYTES_256CU
