"""Cost of perturbed-attention guidance (pag_scale / pag_applied_layers, rt_attention_fwd_keyed_self) on an MI355X.

Pipeline: 1024 x 1024, FLUX.1-dev depth (19 + 38) + RepText tower, random weights, one masked text line, the captured loop. ms per
denoising step over alternated rounds in ONE process: the plain call / the true-CFG call with a negative prompt / PAG with 1, 4 and 19
applied double blocks. A PAG step is expected to cost the CFG step plus, per applied block, the difference between the self launch and
the default kernel at B = 2: compare against the CFG call and the kernel figures of the same process, never across processes.

Kernel: S = 4608 (T = 512, N = 4096), H = 24, B = 2 with the tables of perturbed_attention_tables: the self launch, rt_attention_fwd_keyed
with the same tables, and the dense launch (whichever kernel serves it by default).
Prints a table and one JSON line.  python tools/bench_pag.py [--repeats 3] [--inference-steps 8] [--kernel-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops

T, N, H = 512, 4096, 24


def kernel_bench(dev, rounds=3, iters=100):
    from reptext_amd.pipeline import perturbed_attention_tables

    S, d, B = T + N, H * 128, 2
    qkv = torch.randn(B, S, 3 * d, device=dev).to(torch.bfloat16)
    q, k, v = (qkv[..., i * d : (i + 1) * d] for i in range(3))
    out = torch.empty(B, S, d, device=dev, dtype=torch.bfloat16)
    kc = ops.KeyClasses(*perturbed_attention_tables(T, N, 1)).to(dev)
    cases = {"dense": lambda: ops.attention(q, k, v, out, H), "keyed": lambda: ops.attention(q, k, v, out, H, groups=kc),
             "keyed_self": lambda: ops.attention(q, k, v, out, H, groups=kc, self_key=True)}
    for fn in cases.values():
        for _ in range(iters):                                             # a window long enough for the clocks to settle
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in cases}
    for _ in range(rounds):                                                # alternated: every round times each case once
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / iters * 1e3, 1))
    print(f"attention at B = {B}, S = {S}, H = {H}, us per launch over {rounds} alternated rounds of {iters}", flush=True)
    for name, us in res.items():
        print(f"  {name:12s} " + "  ".join(f"{u:7.1f}" for u in us), flush=True)
    return {"B": B, "S": S, "H": H, "us": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inference-steps", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pag.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_pag", "device": torch.cuda.get_device_name(0), "kernel": kernel_bench(dev, rounds=args.repeats)}
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
    steps = args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(64, 64)
    mask[16:24, 8:56] = 1.0
    kw = dict(prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768), height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5,
              control_image=[r(1, N, 128)], control_mask=[mask.reshape(1, N, 1).to(dev, bf16)], controlnet_conditioning_scale=1.0,
              controlnet_conditioning_step=30, latents=r(1, N, 64), output_type="latent")
    doubles = lambda n: [f"transformer_blocks.{i}" for i in range(n)]
    modes = {"plain": {}, "true_cfg": dict(true_cfg_scale=4.0, negative_prompt_embeds=r(1, T, 4096), negative_pooled_prompt_embeds=r(1, 768))}
    for n in (1, 4, 19):
        modes[f"pag_{n}_double"] = dict(pag_scale=3.0, pag_applied_layers=doubles(n))
    P.GRAPH_CACHE_MAX = max(P.GRAPH_CACHE_MAX, len(modes))                 # every mode keeps its graph: the rounds alternate between them
    run = lambda m: pipe(**kw, **modes[m])
    for m in modes:                                                        # eager, then capture
        run(m)
        run(m)
    torch.cuda.synchronize()
    res = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(m)
            e1.record()
            torch.cuda.synchronize()
            res[m].append(round(e0.elapsed_time(e1) / steps, 3))
    graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
    result["pipeline"] = {"shape": "1024x1024, one masked text line, batch 1, T = 512", "steps": steps, "graphs": graphs, "ms_per_step": res}
    for m in modes:
        print(f"  ms per denoising step, {m:14s}: " + "  ".join(f"{t:.3f}" for t in res[m]) + f"   ({graphs} captured graphs)", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
