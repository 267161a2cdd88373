"""What a negative prompt (true CFG: true_cfg_scale > 1, conditioning batch 2B against latents of batch B) costs per denoising step on
the real-width stack: FLUX.1-dev 19+38 blocks + the RepText tower (6 double blocks), 1024², one masked text line, random weights,
captured loop. Three modes, alternated `--repeats` times in one process:
  (a) plain_b1 .. the plain call at batch 1 (the flagship call),
  (b) plain_b2 .. the plain call at batch 2,
  (c) cfg_b1 .... the CFG call at batch 1: internal batch 2, [negative, positive].
The expectation to confirm or refute: (c) costs what (b) costs — the same launches at the same batch, minus one batch entry of the
x_embedder input and plus the mix inside the step's kernel. The two batch-2 modes swap places from one repeat to the next, and every
figure is kept with the mode that ran before it, so that a difference that follows the position in the sequence (clocks after 4 s of
batch-2 load against after 2 s of batch-1 load) can be told from one that follows the mode.
Prints a table and one JSON line.  python tools/bench_true_cfg.py [--repeats 3] [--inference-steps 28] [--out profiles/true_cfg_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("plain_b1", "plain_b2", "cfg_b1")


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
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'true_cfg'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_true_cfg.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**reptext_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=1)
    pipe = P.FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    P.GRAPH_CACHE_MAX = len(MODES)                                             # one captured loop per mode, none evicted while they alternate
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(1, N, 1, device=dev, dtype=bf16)
    mask[:, 1000:2000] = 1.0                                                   # a window of 1008 of 4096 rows, shared by the batch
    pipe._region_masks = lambda control_mask, device, dtype: [mask]            # a fixed regional mask, no PIL round trip
    fixed = dict(height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5, controlnet_conditioning_scale=1.0,
                 controlnet_conditioning_step=30, control_mask=[0], output_type="latent")
    inputs = lambda B: dict(fixed, prompt_embeds=r(B, T, 4096), pooled_prompt_embeds=r(B, 768), control_image=[r(B, N, 128)], latents=r(B, N, 64))
    calls = {"plain_b1": inputs(1), "plain_b2": inputs(2),
             "cfg_b1": dict(inputs(1), negative_prompt_embeds=r(1, T, 4096), negative_pooled_prompt_embeds=r(1, 768), true_cfg_scale=3.5)}
    result = {"tool": "bench_true_cfg", "device": torch.cuda.get_device_name(0),
              "shape": "1024x1024, T = 512, full depth, one masked text line, captured loop", "inference_steps": steps}
    for m in MODES:                                                            # remember, capture, replay once
        for _ in range(3):
            pipe(**calls[m])
    res, ran_after = {m: [] for m in MODES}, {m: [] for m in MODES}
    for k in range(args.repeats):
        order = MODES if k % 2 == 0 else (MODES[0], MODES[2], MODES[1])
        for j, m in enumerate(order):
            res[m].append(timed_call(lambda: pipe(**calls[m])) / steps)
            ran_after[m].append(order[j - 1])
    entry = result["ms_per_step"] = {m: [round(t, 3) for t in v] for m, v in res.items()}
    entry["ran_after"] = ran_after
    entry["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    entry["cfg_b1_minus_plain_b2"] = round(med["cfg_b1"] - med["plain_b2"], 3)
    entry["cfg_b1_over_plain_b1"] = round(med["cfg_b1"] / med["plain_b1"], 3)
    entry["spread"] = {m: round(max(v) - min(v), 3) for m, v in res.items()}
    print("captured loop, ms per denoising step", flush=True)
    for m in MODES:
        print(f"  {m:9s}: " + "  ".join(f"{t:.3f} (after {p})" for t, p in zip(res[m], ran_after[m])) + f"   spread {entry['spread'][m]:.3f}", flush=True)
    print(f"  CFG at batch 1 minus plain at batch 2: {entry['cfg_b1_minus_plain_b2']:+.3f} ms per step (medians); CFG / plain batch 1 = "
          f"{entry['cfg_b1_over_plain_b1']:.3f}", flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["true_cfg"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
