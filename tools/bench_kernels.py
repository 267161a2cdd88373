"""Kernel micro-benchmarks at the C2 shapes (1024², S=4608, d=3072). Run on the GPU box:
    python tools/bench_kernels.py [gemm|shapes|epilogue|fp8|attn|attn8|elem|passes|all]
Prints TFLOP/s from torch.cuda.Event timing on the current stream (same stream the kernels are enqueued on)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import reptext_amd.ops as ops

dev = torch.device("cuda:0")


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def bench_gemm():
    shapes = [(4608, 21504, 3072), (4608, 3072, 15360), (4096, 9216, 3072), (4096, 12288, 3072), (4096, 3072, 12288),
              (4096, 3072, 3072), (512, 9216, 3072), (512, 12288, 3072), (8192, 8192, 8192)]
    for M, N, K in shapes:
        a = torch.randn(M, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        b = torch.zeros(N, device=dev, dtype=torch.bfloat16)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        t = timeit(lambda: ops.linear(a, w, out, bias=b))
        print(f"gemm M={M} N={N} K={K}: {t*1e6:9.1f} us  {2*M*N*K/t/1e12:8.1f} TF/s", flush=True)
    # grouped: image + text stream
    T, Ni, d = 512, 4096, 3072
    x = torch.randn(T + Ni, d, device=dev).to(torch.bfloat16)
    wi = (torch.randn(3 * d, d, device=dev) * 0.02).to(torch.bfloat16)
    wt = (torch.randn(3 * d, d, device=dev) * 0.02).to(torch.bfloat16)
    out = torch.empty(T + Ni, 3 * d, device=dev, dtype=torch.bfloat16)
    t = timeit(lambda: ops.linear_grouped([ops.LinearProblem(x[T:], wi, out[T:]), ops.LinearProblem(x[:T], wt, out[:T])]))
    print(f"grouped qkv (4096+512)x9216x3072: {t*1e6:9.1f} us  {2*(T+Ni)*3*d*d/t/1e12:8.1f} TF/s", flush=True)


def bench_gemm_shapes():
    """rt_gemm_bf16 on the model's launches (single- and double-block projections with their epilogues), best of 3 x 10 calls."""
    T, Ni, d = 512, 4096, 3072
    x = torch.randn(T + Ni, 4 * d, device=dev).to(torch.bfloat16)
    x32 = torch.randn(T + Ni, d, device=dev)
    gate = torch.randn(1, d, device=dev)
    launches = []
    w_out = (torch.randn(d, 5 * d, device=dev) * 0.02).to(torch.bfloat16)
    a_out = torch.randn(T + Ni, 5 * d, device=dev).to(torch.bfloat16)
    launches.append(("single out 4608x3072x15360 f32", 2 * (T + Ni) * d * 5 * d, lambda: ops.linear(a_out, w_out, x32, gate=gate, res=x32)))
    w_f = (torch.randn(7 * d, d, device=dev) * 0.02).to(torch.bfloat16)
    o_f = torch.empty(T + Ni, 7 * d, device=dev, dtype=torch.bfloat16)
    launches.append(("single fused 4608x21504x3072", 2 * (T + Ni) * 7 * d * d, lambda: ops.linear(x[:, :d], w_f, o_f, gelu_from=3 * d)))
    for name, N, K, f32 in (("qkv", 3 * d, d, False), ("ff1", 4 * d, d, False), ("ff2", d, 4 * d, True), ("out", d, d, True)):
        wi = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        wt = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        o = x32 if f32 else torch.empty(T + Ni, N, device=dev, dtype=torch.bfloat16)
        def run(wi=wi, wt=wt, o=o, K=K, f32=f32):
            if f32:
                ops.linear_grouped([ops.LinearProblem(x[T:, :K], wi, o[T:], gate=gate, res=o[T:]), ops.LinearProblem(x[:T, :K], wt, o[:T], gate=gate, res=o[:T])])
            else:
                ops.linear_grouped([ops.LinearProblem(x[T:, :K], wi, o[T:]), ops.LinearProblem(x[:T, :K], wt, o[:T])])
        launches.append((f"double {name} (4096+512)x{N}x{K}", 2 * (T + Ni) * N * K, run))
    for name, fl, run in launches:
        t = min(timeit(run, iters=10, warm=2) for _ in range(3))
        print(f"{name:42s} {t*1e6:7.1f} us {fl/t/1e12:7.1f} TF/s", flush=True)


def bench_gemm_epilogue(rounds=10):
    """rt_gemm_bf16 on the bf16 loop's launches with rt_gemm_epilogue_variant 0 (general epilogue everywhere) and 1 (straight-line
    epilogue on interior tiles) alternating in one process: median and minimum over `rounds` rounds of 10 calls and the number of rounds
    in which variant 1 was the faster of the pair, one JSON line each. `python tools/bench_kernels.py epilogue [rounds]`."""
    import json
    import statistics
    from reptext_amd import native
    lib = native.load()
    T, Ni, d, H = 512, 4096, 3072, 24
    S = T + Ni
    P = ops.LinearProblem
    bf = lambda *s: (torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16)
    x = torch.randn(S, 5 * d, device=dev).to(torch.bfloat16)
    x32 = torch.randn(S, d, device=dev)
    gate = torch.randn(1, d, device=dev)
    inject = torch.randn(S, d, device=dev).to(torch.bfloat16)
    wn = [(1 + 0.1 * torch.randn(128, device=dev)).to(torch.bfloat16) for _ in range(2)]
    cos, sin = torch.randn(S, 128, device=dev), torch.randn(S, 128, device=dev)
    launches = []
    w7, b7, o7 = bf(7 * d, d), bf(7 * d), torch.empty(S, 7 * d, device=dev, dtype=torch.bfloat16)
    launches.append(("single fused 4608x21504x3072 bf16 plain+gelu", 2 * S * 7 * d * d, lambda: ops.linear(x[:, :d], w7, o7, bias=b7, gelu_from=3 * d)))
    rope = ops.QKRope(2 * d, 0, d, wn[0], wn[1], cos, sin)
    launches.append(("single fused 4608x21504x3072 rope+plain+gelu", 2 * S * 7 * d * d, lambda: ops.linear(x[:, :d], w7, o7, bias=b7, gelu_from=3 * d, rope=rope)))
    w5, b5 = bf(d, 5 * d), bf(d)
    launches.append(("single out 4608x3072x15360 f32 gate+res", 2 * S * d * 5 * d, lambda: ops.linear(x, w5, x32, bias=b5, gate=gate, res=x32)))
    for name, N, K, kind in (("qkv", 3 * d, d, "plain"), ("ff1", 4 * d, d, "gelu"), ("ff2", d, 4 * d, "f32+add2"), ("out", d, d, "f32")):
        wi, wt, bi, bt = bf(N, K), bf(N, K), bf(N), bf(N)
        o = x32 if kind.startswith("f32") else torch.empty(S, N, device=dev, dtype=torch.bfloat16)

        def run(wi=wi, wt=wt, bi=bi, bt=bt, o=o, K=K, kind=kind):
            if kind.startswith("f32"):
                ops.linear_grouped([P(x[T:, :K], wi, o[T:], bias=bi, gate=gate, res=o[T:], add2=inject[T:] if kind == "f32+add2" else None),
                                    P(x[:T, :K], wt, o[:T], bias=bt, gate=gate, res=o[:T])])
            else:
                gf = 0 if kind == "gelu" else None
                ops.linear_grouped([P(x[T:, :K], wi, o[T:], bias=bi, gelu_from=gf), P(x[:T, :K], wt, o[:T], bias=bt, gelu_from=gf)])

        launches.append((f"double {name} (4096+512)x{N}x{K} {kind}", 2 * S * N * K, run))
    prev = lib.rt_gemm_epilogue_variant(-1)
    try:
        for name, fl, run in launches:
            res = {0: [], 1: []}
            for _ in range(rounds):
                for var in (0, 1):
                    lib.rt_gemm_epilogue_variant(var)
                    res[var].append(timeit(run, iters=10, warm=2) * 1e6)
            m0, m1 = statistics.median(res[0]), statistics.median(res[1])
            print(json.dumps({"launch": name, "rounds": rounds, "general_us": {"median": round(m0, 1), "min": round(min(res[0]), 1)},
                              "fast_us": {"median": round(m1, 1), "min": round(min(res[1]), 1)}, "median_change_pct": round(100 * (m1 / m0 - 1), 2),
                              "rounds_fast_faster": sum(f < g for g, f in zip(res[0], res[1])), "fast_tflops": round(fl / m1 / 1e6, 1)}), flush=True)
    finally:
        lib.rt_gemm_epilogue_variant(prev)


def bench_gemm_fp8():
    FP8 = torch.float8_e4m3fn
    shapes = [(4608, 21504, 3072), (4096, 9216, 3072), (4096, 12288, 3072), (8192, 8192, 8192), (9728, 21504, 3072)]
    for M, N, K in shapes:
        a = torch.randn(M, K, device=dev).to(FP8)
        w = torch.randn(N, K, device=dev).to(FP8)
        sa = torch.rand(M, device=dev) + 0.5
        sw = torch.rand(N, device=dev) * 0.02
        b = torch.zeros(N, device=dev, dtype=torch.bfloat16)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        t = timeit(lambda: ops.linear(a, w, out, bias=b, a_scale=sa, w_scale=sw))
        print(f"gemm fp8 M={M} N={N} K={K}: {t*1e6:9.1f} us  {2*M*N*K/t/1e12:8.1f} TF/s", flush=True)
    x = torch.randn(1, 4608, 3072, device=dev)
    o8 = torch.empty(1, 4608, 3072, device=dev, dtype=FP8)
    rs = torch.empty(4608, device=dev)
    mod = torch.randn(1, 6144, device=dev)
    t = timeit(lambda: ops.layernorm_modulate_fp8(x, o8, rs, mod[:, :3072], mod[:, 3072:]))
    print(f"layernorm_mod_fp8 4608x3072 (f32 in): {t*1e6:8.1f} us", flush=True)


def bench_attn():
    """Interleaved A/B of the two attention kernels (variant 0 = attention.hip, 1 = attention_v3.hip where it applies)."""
    from reptext_amd import native
    lib = native.load()
    prev = lib.rt_attention_variant(-1)
    for B, S, H in [(1, 4608, 24), (1, 4096, 32), (4, 4608, 24), (1, 768, 24), (1, 9728, 24)]:
        d = H * 128
        qkv = torch.randn(B, S, 3 * d, device=dev).to(torch.bfloat16)
        out = torch.empty(B, S, d, device=dev, dtype=torch.bfloat16)
        res = {}
        for rnd in range(3):
            for var in (0, 2):
                lib.rt_attention_variant(var)
                res.setdefault(var, []).append(timeit(lambda: ops.attention(qkv[..., :d], qkv[..., d:2*d], qkv[..., 2*d:], out, H), iters=10, warm=2))
        fl = 4 * B * H * S * S * 128
        t0, t1 = min(res[0]), min(res[2])
        print(f"attn B={B} S={S} H={H}: attention.hip {t0*1e6:8.1f} us {fl/t0/1e12:7.1f} TF/s | v3 {t1*1e6:8.1f} us {fl/t1/1e12:7.1f} TF/s | {100*(t1/t0-1):+.1f} %", flush=True)
    lib.rt_attention_variant(prev)


def bench_attn_fp8():
    from reptext_amd import native
    FP8 = torch.float8_e4m3fn
    for B, S, H in [(1, 4608, 24), (1, 9728, 24)]:
        d = H * 128
        qkv = torch.randn(B, S, 3 * d, device=dev).to(torch.bfloat16)
        w = torch.ones(128, device=dev, dtype=torch.bfloat16)
        cos = torch.ones(S, 128, device=dev); sin = torch.zeros(S, 128, device=dev)
        qk8 = torch.empty(B, S, 2 * d, device=dev, dtype=FP8)
        vt8 = torch.empty(int(native.load().rt_attention_fp8_vt_bytes(B, S, H)), device=dev, dtype=FP8)
        out = torch.empty(B, S, d, device=dev, dtype=torch.bfloat16)
        tp = timeit(lambda: ops.attention_fp8_prep(qkv, 0, d, 2 * d, H, 512, w, w, w, w, cos, sin, qk8, vt8))
        t = timeit(lambda: ops.attention_fp8(qk8, vt8, out, H))
        print(f"attn fp8 B={B} S={S} H={H}: prep {tp*1e6:7.1f} us, kernel {t*1e6:9.1f} us  {4*B*H*S*S*128/t/1e12:8.1f} TF/s", flush=True)


def bench_elem():
    S, d = 4608, 3072
    x = torch.randn(1, S, d, device=dev).to(torch.bfloat16)
    out = torch.empty_like(x)
    mod = torch.randn(1, 2 * d, device=dev)
    t = timeit(lambda: ops.layernorm_modulate(x, out, mod[:, :d], mod[:, d:]))
    print(f"layernorm_mod {S}x{d}: {t*1e6:8.1f} us  {2*S*d*2/t/1e9:8.1f} GB/s", flush=True)
    w = (torch.randn(6 * d, d, device=dev) * 0.02).to(torch.bfloat16)
    temb = torch.randn(1, d, device=dev)
    y = torch.empty(1, 6 * d, device=dev)
    t = timeit(lambda: ops.gemv(temb, w, None, y, silu_in=True))
    print(f"adaLN gemv {6*d}x{d}: {t*1e6:8.1f} us  {6*d*d*2/t/1e9:8.1f} GB/s", flush=True)
    qkv = torch.randn(1, S, 3 * d, device=dev).to(torch.bfloat16)
    wn = torch.ones(128, device=dev, dtype=torch.bfloat16)
    cos = torch.randn(S, 128, device=dev); sin = torch.randn(S, 128, device=dev)
    t = timeit(lambda: ops.qk_rmsnorm_rope(qkv, 0, d, 24, 512, wn, wn, wn, wn, cos, sin))
    print(f"qk_rmsnorm_rope {S}x{2*d}: {t*1e6:8.1f} us  {2*S*2*d*2/t/1e9:8.1f} GB/s", flush=True)


def bench_loop_passes(rounds=5):
    """The loop's small passes, new form against the launches it replaces, alternating in one process. The adaLN weights rotate over
    enough distinct copies (> 256 MiB) that every launch streams them from HBM, as in the model (one weight per block)."""
    d, M = 3072, 28
    hi, lo = ops.silu_split(torch.randn(M, d, device=dev), apply_silu=True)
    mk = lambda n: ((torch.randn(n, d, device=dev) * 0.02).to(torch.bfloat16), torch.randn(n, device=dev).to(torch.bfloat16), torch.empty(M, n, device=dev))
    for name, N, ngrp, copies in (("adaLN table 28x9216x3072", 3 * d, 1, 6), ("adaLN table 28x18432x3072 x2", 6 * d, 2, 3)):
        sets = [[mk(N) for _ in range(ngrp)] for _ in range(copies)]
        it = [0]

        def pair():
            pr = sets[it[0] % copies]; it[0] += 1
            ops.linear_grouped([ops.LinearProblem(hi, w, o, bias=b) for w, b, o in pr])
            ops.linear_grouped([ops.LinearProblem(lo, w, o, res=o) for w, b, o in pr])

        def skinny():
            pr = sets[it[0] % copies]; it[0] += 1
            ops.linear_skinny(hi, lo, pr)

        for r in range(rounds):
            t0, t1 = timeit(pair, iters=copies * 4), timeit(skinny, iters=copies * 4)
            print(f"{name}: two launches {t0*1e6:7.1f} us | skinny {t1*1e6:7.1f} us  {ngrp*N*d*2/t1/1e9:7.0f} GB/s of W", flush=True)
        del sets
    T, Ni = 512, 4096
    x = torch.randn(1, T + Ni, d, device=dev)
    out = torch.empty(1, T + Ni, d, device=dev, dtype=torch.bfloat16)
    mi, mt = torch.randn(1, 6 * d, device=dev), torch.randn(1, 6 * d, device=dev)
    ch = lambda m, i: m[:, i * d : (i + 1) * d]

    def two():
        ops.layernorm_modulate(x[:, T:], out[:, T:], ch(mi, 0), ch(mi, 1))
        ops.layernorm_modulate(x[:, :T], out[:, :T], ch(mt, 0), ch(mt, 1))

    one = lambda: ops.layernorm_modulate_pair(x[:, T:], out[:, T:], ch(mi, 0), ch(mi, 1), x[:, :T], out[:, :T], ch(mt, 0), ch(mt, 1))
    for r in range(rounds):
        t0, t1 = timeit(two, iters=50), timeit(one, iters=50)
        print(f"layernorm_mod 4096+512 rows x {d} (f32 in): two launches {t0*1e6:6.1f} us | one launch {t1*1e6:6.1f} us", flush=True)


def bench_fused_qkv(rounds=5):
    """QKV launches with the q/k RMSNorm + RoPE fused into the epilogue (ops.QKRope) beside GEMM + qk_rmsnorm_rope, alternating."""
    d, T, Ni, H = 3072, 512, 4096, 24
    S = T + Ni
    x = torch.randn(1, S, d, device=dev).to(torch.bfloat16)
    wn = [(1 + 0.1 * torch.randn(128, device=dev)).to(torch.bfloat16) for _ in range(4)]
    cos, sin = torch.randn(S, 128, device=dev), torch.randn(S, 128, device=dev)
    P = ops.LinearProblem
    # single block: [k|v|q|mlp]
    w = (torch.randn(7 * d, d, device=dev) * 0.02).to(torch.bfloat16)
    b = torch.zeros(7 * d, device=dev, dtype=torch.bfloat16)
    big = torch.empty(1, S, 7 * d, device=dev, dtype=torch.bfloat16)

    def two_s():
        ops.linear(x, w, big, bias=b, gelu_from=3 * d)
        ops.qk_rmsnorm_rope(big, 2 * d, 0, H, 0, None, None, wn[0], wn[1], cos, sin)

    rope_s = ops.QKRope(2 * d, 0, d, wn[0], wn[1], cos, sin)
    one_s = lambda: ops.linear(x, w, big, bias=b, gelu_from=3 * d, rope=rope_s)
    # double block: image + text groups, [q|k|v]
    wi, wt = [(torch.randn(3 * d, d, device=dev) * 0.02).to(torch.bfloat16) for _ in range(2)]
    b3 = torch.zeros(3 * d, device=dev, dtype=torch.bfloat16)
    qkv = torch.empty(1, S, 3 * d, device=dev, dtype=torch.bfloat16)

    def two_d():
        ops.linear_grouped([P(x[:, T:], wi, qkv[:, T:], bias=b3), P(x[:, :T], wt, qkv[:, :T], bias=b3)])
        ops.qk_rmsnorm_rope(qkv, 0, d, H, T, wn[2], wn[3], wn[0], wn[1], cos, sin)

    ri, rt = ops.QKRope(0, d, d, wn[0], wn[1], cos, sin, pos0=T), ops.QKRope(0, d, d, wn[2], wn[3], cos, sin, pos0=0)
    one_d = lambda: ops.linear_grouped([P(x[:, T:], wi, qkv[:, T:], bias=b3, rope=ri), P(x[:, :T], wt, qkv[:, :T], bias=b3, rope=rt)])
    for r in range(rounds):
        t0, t1, t2, t3 = timeit(two_s), timeit(one_s), timeit(two_d), timeit(one_d)
        print(f"qkv single 4608x21504x3072: gemm + rope {t0*1e6:7.1f} us | fused {t1*1e6:7.1f} us   "
              f"double (4096+512)x9216x3072: gemm + rope {t2*1e6:7.1f} us | fused {t3*1e6:7.1f} us", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("gemm", "all"):
        bench_gemm()
    if what in ("shapes", "all"):
        bench_gemm_shapes()
    if what in ("epilogue", "all"):
        bench_gemm_epilogue(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    if what in ("fp8", "all"):
        bench_gemm_fp8()
    if what in ("attn", "all"):
        bench_attn()
    if what in ("attn8", "all"):
        bench_attn_fp8()
    if what in ("elem", "all"):
        bench_elem()
    if what in ("passes", "all"):
        bench_loop_passes()
        bench_fused_qkv()
