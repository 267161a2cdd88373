"""Where a GEMM tile's epilogue spends its time: instruction issue or the memory system draining. Run on the GPU box:
    make -C tools/gemm_stamps && python tools/gemm_stamps/report.py [out.json]
Drives libgemm_stamps.so (gemm_stamps.hip: the library's GEMM with s_memtime stamps per wave at the end of the K loop, behind the last
store and after s_waitcnt vmcnt(0)) on the bf16 loop's launches under rt_gemm_epilogue_variant 0 and 1, and prints per epilogue kind the
median over waves of issue (t1 - t0), drain (t2 - t1) and both, in microseconds (s_memtime ticks converted with the s_memrealtime pair
each wave records, 100 MHz), plus per workgroup the time from the first wave leaving the K loop to the last wave's end."""
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch  # noqa: E402
import reptext_amd.native as native  # noqa: E402
import reptext_amd.ops as ops  # noqa: E402

KINDS = {0: "general bf16 plain", 8: "general bf16 GELU", 1: "general f32", 2: "rope tile", 3: "straight bf16 plain", 4: "straight bf16 GELU"}
dev = torch.device("cuda:0")


def main():
    lib = C.CDLL(os.path.join(HERE, "libgemm_stamps.so"))
    lib.rt_gemm_bf16.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.rt_gemm_stamps_buffer.argtypes = [C.c_void_p]
    T, Ni, d = 512, 4096, 3072
    S = T + Ni
    P = ops.LinearProblem
    bf = lambda *s: (torch.randn(*s, device=dev) * 0.02).to(torch.bfloat16)
    x = torch.randn(S, d, device=dev).to(torch.bfloat16)
    x32 = torch.randn(S, d, device=dev)
    gate = torch.randn(1, d, device=dev)
    wn = [(1 + 0.1 * torch.randn(128, device=dev)).to(torch.bfloat16) for _ in range(2)]
    cos, sin = torch.randn(S, 128, device=dev), torch.randn(S, 128, device=dev)
    w7, b7, o7 = bf(7 * d, d), bf(7 * d), torch.empty(S, 7 * d, device=dev, dtype=torch.bfloat16)
    w4i, w4t, b4, o4 = bf(4 * d, d), bf(4 * d, d), bf(4 * d), torch.empty(S, 4 * d, device=dev, dtype=torch.bfloat16)
    w1i, w1t, b1 = bf(d, d), bf(d, d), bf(d)
    launches = [
        ("single fused 4608x21504x3072 (rope q/k | plain v | GELU mlp)",
         [P(x, w7, o7, bias=b7, gelu_from=3 * d, rope=ops.QKRope(2 * d, 0, d, wn[0], wn[1], cos, sin))]),
        ("double ff1 (4096+512)x12288x3072 GELU", [P(x[T:], w4i, o4[T:], bias=b4, gelu_from=0), P(x[:T], w4t, o4[:T], bias=b4, gelu_from=0)]),
        ("double out (4096+512)x3072x3072 f32 gate+res", [P(x[T:], w1i, x32[T:], bias=b1, gate=gate, res=x32[T:]), P(x[:T], w1t, x32[:T], bias=b1, gate=gate, res=x32[:T])]),
    ]
    stream = torch.cuda.current_stream().cuda_stream
    report = []
    for name, problems in launches:
        tiles = sum(-(-p.out.shape[-2] // 256) * -(-p.out.shape[-1] // 256) for p in problems)
        groups = (native.GemmGroup * len(problems))(*[p.to_group() for p in problems])
        for variant in (0, 1):
            lib.rt_gemm_epilogue_variant(variant)
            buf = torch.zeros(tiles * 8 * 8, dtype=torch.int64, device=dev)
            assert lib.rt_gemm_stamps_buffer(None) == 0
            for _ in range(3):                                                   # warm: clocks, caches
                assert lib.rt_gemm_bf16(groups, len(problems), stream) == 0
            assert lib.rt_gemm_stamps_buffer(buf.data_ptr()) == 0
            assert lib.rt_gemm_bf16(groups, len(problems), stream) == 0
            torch.cuda.synchronize()
            assert lib.rt_gemm_stamps_buffer(None) == 0
            s = buf.cpu().view(tiles, 8, 8).double()
            t0, t1, t2, kind, r0, r2 = (s[..., i] for i in range(6))
            us_per_tick = float(((r2 - r0).sum() / (t2 - t0).sum()) * 0.01)      # s_memrealtime: 10 ns per tick
            rows = {}
            for k in sorted(set(kind[:, 0].long().tolist())):
                m = kind[:, 0] == k
                med = lambda v: round(statistics.median((v[m].flatten() * us_per_tick).tolist()), 2)
                wg = ((t2[m].max(dim=1).values - t0[m].min(dim=1).values) * us_per_tick).tolist()
                rows[KINDS.get(int(k), str(int(k)))] = {"tiles": int(m.sum()), "issue_us": med(t1 - t0), "drain_us": med(t2 - t1), "wave_total_us": med(t2 - t0),
                                                        "workgroup_first_kloop_end_to_last_wave_end_us": round(statistics.median(wg), 2)}
            line = {"launch": name, "variant": variant, "memtime_ticks_per_us": round(1 / us_per_tick, 1), "kinds": rows}
            print(json.dumps(line), flush=True)
            report.append(line)
    if len(sys.argv) > 1:
        json.dump(report, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
