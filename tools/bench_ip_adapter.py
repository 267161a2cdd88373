"""IP-Adapter cost on the real-width stack (FLUX.1-dev 19+38 blocks + RepText tower, 1024², batch 1, random weights, captured loop):
  * rt_ip_attention alone at the block's shape (N = 4096 rows of the fused q|k|v buffer, H = 24) for n = 4 and n = 128 image-prompt
    tokens: time and share of its byte floor (q read once + o written once + K/V once, over 6.29 TB/s), on a rotating set of buffers
    larger than the 256 MB Infinity Cache. `--kernel-only` stops here (the form to run under `rocprofv3 --kernel-trace --stats`);
  * the adapter's per-call set-up (projection GEMM + LayerNorm + stacked K/V GEMM);
  * denoising-step time of the pipeline without embeds and with the adapter, alternated `--repeats` times, each from its captured
    graph.
`--layout instantx` measures the InstantX form instead (E = 1152, n = 128, a term in all 19 + 38 blocks): rt_ip_attention_gated at the
double-block shape (gated fp32 accumulate onto the residual rows) and at the single-block shape (S = 4608 rows at ldq = 7d, bf16 write)
plus the strided add, each against its byte floor; the six-launch set-up; and three alternated pipeline modes — without embeds, with
the adapter, and without embeds but with the fused q/k norm + RoPE epilogue switched off ("without_unfused"), which is what an active
adapter costs every block before its own kernels run.
Prints a table and one JSON line.  python tools/bench_ip_adapter.py [--layout xlabs|instantx] [--repeats 3] [--inference-steps 28] [--kernel-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops

COPY_TBS = 6.29
E = 768                                # CLIP ViT-L/14 projection width, what the XLabs adapter takes


def timed(fn, iters, warm=2):
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


def kernel_bench(dev, N=4096, H=24):
    d = H * 128
    res = {}
    print("rt_ip_attention, N = 4096, H = 24, q inside the fused q|k|v row, bf16 o      us    floor us   % of floor rate", flush=True)
    nbuf = 8                                                                    # 8 x (75 MB q|k|v + 25 MB o): every pass streams from HBM
    qkv = [torch.randn(1, N, 3 * d, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
    out = [torch.empty(1, N, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    wq = torch.ones(128, device=dev, dtype=torch.bfloat16)
    for n in (4, 128):
        k = (torch.randn(1, n, d, device=dev) * 1.5).to(torch.bfloat16)
        v = torch.randn(1, n, d, device=dev).to(torch.bfloat16)
        nbytes = 2 * N * d * 2 + 2 * n * d * 2
        floor = nbytes / (COPY_TBS * 1e12)
        # "packed": the same rows as one contiguous [N, d] tensor (nothing between the heads' segments of consecutive rows)
        for label, qs in (("", [t[..., :d] for t in qkv]), ("_packed_q", [t.view(-1)[: N * d].view(1, N, d) for t in qkv])):
            i = [0]

            def one():
                j = i[0] % nbuf
                ops.ip_attention(qs[j], wq, k, v, out[j], H, ip_scale=0.7)
                i[0] += 1
            t = sorted(timed(one, 5 * nbuf, warm=nbuf) for _ in range(3))[1]       # median of three
            res[f"n{n}{label}"] = {"us": round(t * 1e6, 2), "bytes": nbytes, "floor_us": round(floor * 1e6, 2), "share_of_floor_rate": round(floor / t, 3)}
            print(f"n = {n:3d} {label or '(fused row)':12s}                                                 {t * 1e6:8.1f}  {floor * 1e6:8.1f}   {100 * floor / t:5.1f} %", flush=True)
    return res


def kernel_bench_instantx(dev, N=4096, T=512, H=24, n=128):
    d, S = H * 128, T + N
    res = {}
    nbuf = 4                                                                    # 4 x (198 MB big + 28 MB term + 57 MB residual): HBM every pass
    big = [torch.randn(1, S, 7 * d, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
    term = [torch.empty(1, S, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    qkv = [b.view(-1)[: N * 3 * d].view(1, N, 3 * d) for b in big]
    x = [torch.randn(1, S, d, device=dev) for _ in range(nbuf)]
    wq = torch.ones(128, device=dev, dtype=torch.bfloat16)
    k = torch.nn.functional.normalize(torch.randn(1, n, H, 128, device=dev), dim=-1).mul(128 ** 0.5).reshape(1, n, d).to(torch.bfloat16)
    v = torch.randn(1, n, d, device=dev).to(torch.bfloat16)
    table = torch.randn(1, 6 * d, device=dev)
    kvb = 2 * n * d * 2
    cases = {
        "double_gated_f32_accumulate": (N * d * (2 + 4 + 4) + kvb, lambda j: ops.ip_attention_gated(qkv[j][..., :d], wq, k, v, x[j][:, T:], H, ip_scale=0.7,
                                                                                                  gate=table[:, 2 * d : 3 * d], accumulate=True)),
        "single_bf16_write": (S * d * (2 + 2) + kvb, lambda j: ops.ip_attention_gated(big[j][..., 2 * d : 3 * d], wq, k, v, term[j], H, ip_scale=0.7)),
        "single_strided_add": (S * d * (2 + 2 + 2), lambda j: ops.add_bf16_(big[j][..., 2 * d : 3 * d], term[j])),
    }
    print(f"InstantX form, n = {n}, H = {H}                                   us    floor us   % of floor rate", flush=True)
    for name, (nbytes, fn) in cases.items():
        i = [0]

        def one():
            fn(i[0] % nbuf)
            i[0] += 1
        t = sorted(timed(one, 5 * nbuf, warm=nbuf) for _ in range(3))[1]
        floor = nbytes / (COPY_TBS * 1e12)
        res[name] = {"us": round(t * 1e6, 2), "bytes": nbytes, "floor_us": round(floor * 1e6, 2), "share_of_floor_rate": round(floor / t, 3)}
        print(f"{name:40s}                     {t * 1e6:8.1f}  {floor * 1e6:8.1f}   {100 * floor / t:5.1f} %", flush=True)
    return res


def adapter_sd_instantx(tr, n, dev, seed, Ee=1152):
    g = torch.Generator(device=dev).manual_seed(seed)
    C, d, L = tr.config.joint_attention_dim, tr.inner_dim, tr.config.num_layers + tr.config.num_single_layers
    r = lambda *s, std: (torch.randn(*s, generator=g, device=dev) * std).to(torch.bfloat16)
    sd = {"image_proj.proj.0.weight": r(2 * Ee, Ee, std=Ee ** -0.5), "image_proj.proj.0.bias": r(2 * Ee, std=0.02),
          "image_proj.proj.2.weight": r(n * C, 2 * Ee, std=(2 * Ee) ** -0.5), "image_proj.proj.2.bias": r(n * C, std=0.02),
          "image_proj.norm.weight": torch.ones(C, device=dev, dtype=torch.bfloat16), "image_proj.norm.bias": r(C, std=0.02)}
    for j in range(L):
        sd[f"ip_adapter.{j}.to_k_ip.weight"], sd[f"ip_adapter.{j}.to_v_ip.weight"] = r(d, C, std=0.025), r(d, C, std=0.015)
    return sd


def adapter_sd(tr, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    C, d, L = tr.config.joint_attention_dim, tr.inner_dim, tr.config.num_layers
    r = lambda *s, std: (torch.randn(*s, generator=g, device=dev) * std).to(torch.bfloat16)
    sd = {"image_proj.proj.weight": r(n * C, E, std=E ** -0.5), "image_proj.proj.bias": r(n * C, std=0.02),
          "image_proj.norm.weight": torch.ones(C, device=dev, dtype=torch.bfloat16), "image_proj.norm.bias": r(C, std=0.02)}
    for i in range(L):
        sd[f"ip_adapter.{i}.to_k_ip.weight"], sd[f"ip_adapter.{i}.to_k_ip.bias"] = r(d, C, std=0.025), r(d, std=0.02)
        sd[f"ip_adapter.{i}.to_v_ip.weight"], sd[f"ip_adapter.{i}.to_v_ip.bias"] = r(d, C, std=0.015), r(d, std=0.02)
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inference-steps", type=int, default=28)
    ap.add_argument("--tokens", type=int, nargs="+", default=None, help="default: 4 128 (xlabs), 128 (instantx)")
    ap.add_argument("--layout", choices=("xlabs", "instantx"), default="xlabs")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ip_adapter.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    instantx = args.layout == "instantx"
    args.tokens = args.tokens or ([128] if instantx else [4, 128])
    Ew = 1152 if instantx else E
    result = {"tool": "bench_ip_adapter", "layout": args.layout, "device": torch.cuda.get_device_name(0),
              "kernel": kernel_bench_instantx(dev) if instantx else kernel_bench(dev)}
    if args.kernel_only:
        print(json.dumps(result), flush=True)
        return

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    bf16 = torch.bfloat16
    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**reptext_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=1)
    pipe = P.FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    H = W = 1024
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(1, N, 1, device=dev, dtype=bf16)
    mask[:, 1000:2000] = 1.0
    kw = dict(prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768), height=H, width=W, num_inference_steps=steps, guidance_scale=3.5,
              control_image=[r(1, N, 128)], controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30, latents=r(1, N, 64),
              output_type="latent")
    pipe._region_masks = lambda control_mask, device, dtype: [mask]            # a fixed regional mask, no PIL round trip
    emb = r(1, 1, Ew)
    import reptext_amd.mmdit as mmdit

    def run(mode):
        fused = mmdit.FUSED_QK_ROPE
        mmdit.FUSED_QK_ROPE = fused and mode != "without_unfused"               # part of the graph key: this mode has its own graph
        try:
            pipe(**kw, **({"ip_adapter_image_embeds": emb} if mode == "with" else {}))
        finally:
            mmdit.FUSED_QK_ROPE = fused

    # the pipeline keeps two captured graphs: modes are alternated in pairs, each pair with the graph cache to itself
    pairs = (("without", "with"), ("without", "without_unfused")) if instantx else (("without", "with"),)
    result["pipeline"] = {}
    for n in args.tokens:
        pipe.load_ip_adapter((adapter_sd_instantx if instantx else adapter_sd)(tr, n, dev, seed=10 + n))
        setup = timed(lambda: tr._ip_adapter.prepare(emb), 10)
        print(f"n = {n}: per-call set-up (projection(s) + LayerNorm + K/V GEMM [+ GELU, K norm]) {setup * 1e3:.3f} ms", flush=True)
        entry = result["pipeline"][f"n{n}"] = {"setup_ms": round(setup * 1e3, 3), "pairs": []}
        for modes in pairs:
            pipe.__dict__.get("_graph_cache", {}).clear()                       # the adapter is part of the key: drop the last one's graphs
            for m in modes:                                                     # eager, then capture
                run(m)
                run(m)
            torch.cuda.synchronize()
            res = {m: [] for m in modes}
            for _ in range(args.repeats):
                for m in modes:
                    res[m].append(timed(lambda: run(m), 1, warm=0) / steps * 1e3)
            graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
            entry["pairs"].append({"graphs": graphs, "ms_per_step": {m: [round(t, 3) for t in v] for m, v in res.items()}})
            for m in modes:
                print(f"  ms per denoising step, {m:15s}: " + "  ".join(f"{t:.3f}" for t in res[m]) + f"   ({graphs} captured graphs)", flush=True)
        pipe.unload_ip_adapter()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
