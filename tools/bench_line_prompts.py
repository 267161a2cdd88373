"""Cost of per-line prompts (region-masked joint attention) on the real-width stack (FLUX.1-dev 19+38 blocks + RepText tower, 1024²,
batch 1, random weights, captured loop):
  * the kernel alone at S = 512 + 2·128 + 4096 = 4864, H = 24, alternated in one process: rt_attention_fwd_grouped with every bit set,
    with the real table of two line prompts, and the dense launch under rt_attention_variant(0) (csrc/attention.hip, the kernel the
    grouped launch instantiates) and under variant 1 (the default: attention_v3 takes S % 256 == 0). `--kernel-only` stops here;
  * ms per denoising step of the plain call at T = 512, of a plain DENSE call at T = 512 + 2·128 (the longer text stream without a mask)
    and of the call with two line prompts of 128 tokens, each from its captured graph, alternated in pairs (the pipeline keeps two graphs).
By counting, the line prompts cost 4864² / 4608² = 1.11 x the attention FLOPs plus the loss of attention_v3 at this S, and the longer
text stream in every GEMM of the text rows.
`--isolation` measures region isolation (control_prompt_isolation=True, rt_attention_fwd_keyed) instead: the kernel cases are the grouped
launch with the real table, the keyed launch with the tables of line_prompt_classes for the same two boxes (16 of the 64 image-row
tiles hold two classes), the keyed launch with a class per group (every tile of one class) and with every key of every tile of
another class than its neighbour (every tile mixed); the pipeline pair is the call with line prompts without and with isolation.
`--scale` measures a strength per line prompt (control_prompt_scale, rt_attention_fwd_grouped_biased / rt_attention_fwd_keyed_biased)
instead: the kernel cases are the grouped and the keyed launch with the real tables, each without a bias and with the table of scales
(2.0, 0.5) — 4 of the 76 key tiles carry a bias —; the pipeline pairs are the call with line prompts without and with the keyword, under
the grouped rule and under isolation.
Prints a table and one JSON line.  python tools/bench_line_prompts.py [--repeats 3] [--inference-steps 28] [--kernel-only] [--isolation | --scale]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops
from reptext_amd import native

T0, L, R, N, H = 512, 128, 2, 4096, 24


def two_boxes(dev, dtype):
    """Token masks [1, N, 1] of two text lines on the 64 x 64 grid: rows 16..23 and 36..43, columns 8..55."""
    out = []
    for r0 in (16, 36):
        m = torch.zeros(64, 64)
        m[r0 : r0 + 8, 8:56] = 1.0
        out.append(m.reshape(1, N, 1).to(dev, dtype))
    return out


def kernel_bench(dev, rounds=3, iters=10, isolation=False, scale=False):
    from reptext_amd.pipeline import line_prompt_bias, line_prompt_classes, line_prompt_groups

    S, d = T0 + R * L + N, H * 128
    qkv = torch.randn(1, S, 3 * d, device=dev).to(torch.bfloat16)
    q, k, v = (qkv[..., i * d : (i + 1) * d] for i in range(3))
    out = torch.empty(1, S, d, device=dev, dtype=torch.bfloat16)
    ends, real = line_prompt_groups(T0, L, [m.cpu() for m in two_boxes("cpu", torch.float32)], N)
    full = torch.full_like(real, (1 << len(ends)) - 1)
    lib = native.load()

    def dense(mode):
        def run():
            prev = lib.rt_attention_variant(mode)
            try:
                ops.attention(q, k, v, out, H)
            finally:
                lib.rt_attention_variant(prev)
        return run

    grouped = lambda table: (lambda g: lambda: ops.attention(q, k, v, out, H, groups=g))(ops.KeyGroups(ends, table.to(dev)))
    cases = {"grouped_all_bits": grouped(full), "grouped_real_table": grouped(real), "dense_variant0": dense(0), "dense_variant1": dense(1)}
    if isolation:
        boxes = [m.cpu() for m in two_boxes("cpu", torch.float32)]
        keyed = lambda vis, cls: (lambda g: lambda: ops.attention(q, k, v, out, H, groups=g))(ops.KeyClasses(vis, cls).to(dev))
        j = torch.arange(S)
        per_group = torch.bucketize(j, torch.tensor(ends), right=True).to(torch.uint8)[None]
        cases = {"grouped_real_table": grouped(real), "keyed_real_tables": keyed(*line_prompt_classes(T0, L, boxes, N)),
                 "keyed_class_per_group": keyed(real, per_group), "keyed_every_tile_mixed": keyed(torch.full_like(real, 3), (j % 2).to(torch.uint8)[None])}
    if scale:
        boxes = [m.cpu() for m in two_boxes("cpu", torch.float32)]
        bias = line_prompt_bias([2.0, 0.5], [True, True]).to(dev)
        kg, kc = ops.KeyGroups(ends, real.to(dev)), ops.KeyClasses(*line_prompt_classes(T0, L, boxes, N)).to(dev)
        launch = lambda g, kb: lambda: ops.attention(q, k, v, out, H, groups=g, key_bias=kb)
        cases = {"grouped_real_table": launch(kg, None), "grouped_biased": launch(kg, bias), "keyed_real_tables": launch(kc, None),
                 "keyed_biased": launch(kc, bias)}
    for fn in cases.values():
        for _ in range(iters if isolation or scale else 1):                      # isolation: a window long enough for the clocks to settle
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in cases}
    for _ in range(rounds):                                            # alternated: every round times each case once
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / iters * 1e3, 1))
    print(f"attention at S = {S}, H = {H}, us per launch over {rounds} alternated rounds of {iters}", flush=True)
    for name, us in res.items():
        print(f"  {name:20s} " + "  ".join(f"{u:7.1f}" for u in us), flush=True)
    return {"S": S, "H": H, "us": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inference-steps", type=int, default=28)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--isolation", action="store_true")
    ap.add_argument("--scale", action="store_true")
    args = ap.parse_args()
    if args.isolation and args.scale:
        raise SystemExit("--isolation and --scale are two measurements: give one")
    if not torch.cuda.is_available():
        raise SystemExit("bench_line_prompts.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_line_prompts", "device": torch.cuda.get_device_name(0), "kernel": kernel_bench(dev, iters=200 if args.isolation or args.scale else 10, isolation=args.isolation, scale=args.scale)}
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
    masks = two_boxes(dev, bf16)
    kw = dict(pooled_prompt_embeds=r(1, 768), height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5,
              control_image=[r(1, N, 128), r(1, N, 128)], control_mask=masks, controlnet_conditioning_scale=1.0,
              controlnet_conditioning_step=30, latents=r(1, N, 64), output_type="latent")
    base, long_prompt, lines = r(1, T0, 4096), r(1, T0 + R * L, 4096), [r(1, L, 4096) for _ in range(R)]
    modes = {"plain_T512": dict(prompt_embeds=base), "dense_T768": dict(prompt_embeds=long_prompt),
             "line_prompts": dict(prompt_embeds=base, control_prompt_embeds=lines, control_prompt_max_sequence_length=L)}
    modes["line_isolation"] = dict(modes["line_prompts"], control_prompt_isolation=True)
    modes["line_scale"] = dict(modes["line_prompts"], control_prompt_scale=[2.0, 0.5])
    modes["line_isolation_scale"] = dict(modes["line_isolation"], control_prompt_scale=[2.0, 0.5])
    run = lambda m: pipe(**kw, **modes[m])
    result["pipeline"] = {"shape": "1024x1024, two text lines, batch 1", "steps": steps, "pairs": []}
    pairs = (("plain_T512", "line_prompts"), ("dense_T768", "line_prompts"))
    if args.isolation:
        pairs = (("line_prompts", "line_isolation"),)
    if args.scale:
        pairs = (("line_prompts", "line_scale"), ("line_isolation", "line_isolation_scale"))
    for pair in pairs:
        pipe.__dict__.get("_graph_cache", {}).clear()                   # the pipeline keeps two graphs: each pair has the cache to itself
        for m in pair:                                                  # eager, then capture
            run(m)
            run(m)
        torch.cuda.synchronize()
        res = {m: [] for m in pair}
        for _ in range(args.repeats):
            for m in pair:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(m)
                e1.record()
                torch.cuda.synchronize()
                res[m].append(round(e0.elapsed_time(e1) / steps, 3))
        graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
        result["pipeline"]["pairs"].append({"graphs": graphs, "ms_per_step": res})
        for m in pair:
            print(f"  ms per denoising step, {m:20s}: " + "  ".join(f"{t:.3f}" for t in res[m]) + f"   ({graphs} captured graphs)", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
