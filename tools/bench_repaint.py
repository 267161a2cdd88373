"""What rendering text into an existing image costs, per denoising step and per call, on the real-width stack: FLUX.1-dev 19+38 blocks
+ the RepText tower (6 double blocks), 1024², one masked text line, random weights. Four modes, alternated `--repeats` times in one
process:
  (a) plain ......... the text-to-image call (the flagship call), captured loop,
  (b) repaint_1.0 ... FluxControlNetRepaintPipeline at strength 1.0: every step, each with the blend, captured loop,
  (c) repaint_0.6 ... the same at strength 0.6: the last int-rounded 60 % of the steps, captured loop,
  (d) inpaint ....... the inpaint flow (config C4): a second 6-block tower and true CFG at internal batch 2; its loop is eager by decision.
The expectation to confirm or refute: a repaint step costs what a plain step costs (the blend rides in the step's kernel), so (b) equals
(a) per call and (c) is about 0.6 × (a). Every figure is kept with the mode that ran before it; the order is reversed every other repeat.
Prints a table and one JSON line.  python tools/bench_repaint.py [--repeats 3] [--inference-steps 28] [--out profiles/repaint_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("plain", "repaint_1.0", "repaint_0.6", "inpaint")


def timed_call(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inference-steps", type=int, default=28)
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'repaint'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_repaint.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline, repaint_t_start
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    cfg_c = reptext_controlnet_config()
    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**cfg_c, device=dev, dtype=bf16).random_init_(seed=1)
    cni = FluxControlNetModel(**dict(cfg_c, extra_condition_channels=4), device=dev, dtype=bf16).random_init_(seed=2)
    pipe = FluxControlNetRepaintPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    inpaint = InpaintPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn, cni)
    P.GRAPH_CACHE_MAX = 3                                                      # one captured loop per captured mode, none evicted
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(1, N, 1, device=dev, dtype=bf16)
    mask[:, 1000:2000] = 1.0                                                   # a window of 1008 of 4096 rows
    for p in (pipe, inpaint):
        p.set_progress_bar_config(disable=True)
        p._region_masks = lambda control_mask, device, dtype: [mask]           # a fixed regional mask, no PIL round trip
    base = dict(height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5, controlnet_conditioning_scale=1.0,
                controlnet_conditioning_step=30, control_mask=[0], output_type="latent", prompt_embeds=r(1, T, 4096),
                pooled_prompt_embeds=r(1, 768), control_image=[r(1, N, 128)], latents=r(1, N, 64))
    repaint = dict(base, image=r(1, N, 64).float(), mask_image=mask.float().expand(1, N, 64).contiguous())
    inp = dict(base, negative_prompt_embeds=r(1, T, 4096), negative_pooled_prompt_embeds=r(1, 768), true_guidance_scale=2.0,
               control_image_inpaint=r(1, N, 68), controlnet_conditioning_scale_inpaint=1.0)
    calls = {"plain": lambda: P.FluxControlNetPipeline.__call__(pipe, **base),
             "repaint_1.0": lambda: pipe(**repaint, strength=1.0),
             "repaint_0.6": lambda: pipe(**repaint, strength=0.6),
             "inpaint": lambda: inpaint(**inp)}
    ran = {"plain": steps, "repaint_1.0": steps - repaint_t_start(steps, 1.0), "repaint_0.6": steps - repaint_t_start(steps, 0.6), "inpaint": steps}
    result = {"tool": "bench_repaint", "device": torch.cuda.get_device_name(0), "inference_steps": steps, "steps_run": ran,
              "shape": "1024x1024, T = 512, full depth, one masked text line; plain and repaint captured, inpaint eager with a second tower"}
    for m in MODES:                                                            # remember, capture, replay once
        for _ in range(3 if m != "inpaint" else 1):
            calls[m]()
    res, ran_after = {m: [] for m in MODES}, {m: [] for m in MODES}
    for k in range(args.repeats):
        order = MODES if k % 2 == 0 else MODES[::-1]
        for j, m in enumerate(order):
            res[m].append(timed_call(calls[m]))
            ran_after[m].append(order[j - 1])
    med = lambda v: sorted(v)[len(v) // 2]
    result["ms_per_call"] = {m: [round(t, 2) for t in v] for m, v in res.items()}
    result["ms_per_step"] = {m: [round(t / ran[m], 3) for t in v] for m, v in res.items()}
    result["spread_ms_per_step"] = {m: round((max(v) - min(v)) / ran[m], 3) for m, v in res.items()}
    result["ran_after"] = ran_after
    result["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
    result["median_call_over_plain"] = {m: round(med(res[m]) / med(res["plain"]), 3) for m in MODES}
    result["median_step_over_plain"] = {m: round(med(res[m]) / ran[m] / (med(res["plain"]) / steps), 3) for m in MODES}
    print("ms per denoising step that runs (ms per call)", flush=True)
    for m in MODES:
        print(f"  {m:11s} [{ran[m]:2d} steps]: " + "  ".join(f"{t / ran[m]:.3f} ({t:.1f}, after {p})" for t, p in zip(res[m], ran_after[m]))
              + f"   spread {result['spread_ms_per_step'][m]:.3f}", flush=True)
    print(f"  per call / plain: {result['median_call_over_plain']}; per step / plain: {result['median_step_over_plain']}", flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["repaint"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
