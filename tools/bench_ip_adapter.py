"""IP-Adapter cost on the real-width stack (FLUX.1-dev 19+38 blocks + RepText tower, 1024², batch 1, random weights, captured loop):
  * rt_ip_attention alone at the block's shape (N = 4096 rows of the fused q|k|v buffer, H = 24) for n = 4 and n = 128 image-prompt
    tokens: time and share of its byte floor (q read once + o written once + K/V once, over 6.29 TB/s), on a rotating set of buffers
    larger than the 256 MB Infinity Cache. `--kernel-only` stops here (the form to run under `rocprofv3 --kernel-trace --stats`);
  * the adapter's per-call set-up (projection GEMM + LayerNorm + stacked K/V GEMM);
  * denoising-step time of the pipeline without embeds and with the adapter, alternated `--repeats` times, each from its captured
    graph.
Prints a table and one JSON line.  python tools/bench_ip_adapter.py [--repeats 3] [--inference-steps 28] [--kernel-only]"""
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
    ap.add_argument("--tokens", type=int, nargs="+", default=[4, 128])
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ip_adapter.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_ip_adapter", "device": torch.cuda.get_device_name(0), "kernel": kernel_bench(dev)}
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
    emb = r(1, 1, E)

    def run(mode):
        pipe(**kw, **({} if mode == "without" else {"ip_adapter_image_embeds": emb}))

    modes = ("without", "with")
    result["pipeline"] = {}
    for n in args.tokens:
        pipe.load_ip_adapter(adapter_sd(tr, n, dev, seed=10 + n))
        pipe.__dict__.get("_graph_cache", {}).clear()                           # the adapter is part of the key: drop the last one's graphs
        setup = timed(lambda: tr._ip_adapter.prepare(emb), 10)
        for m in modes:                                                         # eager, then capture
            run(m)
            run(m)
        torch.cuda.synchronize()
        res = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m in modes:
                res[m].append(timed(lambda: run(m), 1, warm=0) / steps * 1e3)
        graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
        result["pipeline"][f"n{n}"] = {"setup_ms": round(setup * 1e3, 3), "graphs": graphs, "ms_per_step": {m: [round(t, 3) for t in v] for m, v in res.items()}}
        print(f"n = {n}: per-call set-up (projection + LayerNorm + K/V GEMM) {setup * 1e3:.3f} ms; {graphs} captured graphs", flush=True)
        for m in modes:
            print(f"  ms per denoising step, {m:15s}: " + "  ".join(f"{t:.3f}" for t in res[m]), flush=True)
        pipe.unload_ip_adapter()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
