"""What the second ControlNet (pipe.controlnet_union, Union-Pro-2.0 shape) costs per denoising step on the real-width stack: FLUX.1-dev
19+38 blocks + the RepText tower (6 double blocks), 1024², batch 1, random weights. Three modes, alternated `--repeats` times:
  (a) one_line ........ one masked text line (the flagship call),
  (b) line_and_union .. the same plus the union tower on every step,
  (c) two_lines ....... two masked text lines (what one more evaluation of a 6-block tower costs today),
first with the eager loop, then each from its captured hipGraph. (b) - (a) against (c) - (a) is the figure: both add one tower evaluation
per step; the union tower's is unmasked (full-row zero-linears, no windowed last block).
Prints a table and one JSON line.  python tools/bench_union.py [--repeats 3] [--inference-steps 28] [--out profiles/union_tower_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("one_line", "line_and_union", "two_lines")


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
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'union_tower'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_union.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config, union_pro2_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**reptext_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=1)
    pipe = P.FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.controlnet_union = FluxControlNetModel(**union_pro2_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=2)
    pipe.set_progress_bar_config(disable=True)
    P.GRAPH_CACHE_MAX = len(MODES)                                             # one captured loop per mode, none evicted while they alternate
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    masks = [torch.zeros(1, N, 1, device=dev, dtype=bf16) for _ in range(2)]
    masks[0][:, 1000:2000] = 1.0                                               # both lines inside rows 1000..2400: a window of 1408 of 4096 rows
    masks[1][:, 1400:2400] = 1.0
    pipe._region_masks = lambda control_mask, device, dtype: list(masks[: len(control_mask)])      # fixed regional masks, no PIL round trip
    base = dict(prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768), height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5,
                controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30, latents=r(1, N, 64), output_type="latent")
    h1, h2, hu = r(1, N, 128), r(1, N, 128), r(1, N, 64)
    calls = {"one_line": dict(base, control_image=[h1], control_mask=[0]),
             "line_and_union": dict(base, control_image=[h1], control_mask=[0], control_image_union=hu, controlnet_conditioning_scale_union=0.7),
             "two_lines": dict(base, control_image=[h1, h2], control_mask=[0, 1])}
    result = {"tool": "bench_union", "device": torch.cuda.get_device_name(0), "shape": "1024x1024, batch 1, T = 512, full depth",
              "inference_steps": steps, "ms_per_step": {}}
    for loop in ("eager", "captured"):
        pipe.capture_graphs = loop == "captured"
        for m in MODES:                                                        # warm (and for the captured loop: remember, then capture)
            pipe(**calls[m])
            pipe(**calls[m])
        res = {m: [] for m in MODES}
        for _ in range(args.repeats):
            for m in MODES:
                res[m].append(timed_call(lambda: pipe(**calls[m])) / steps)
        entry = result["ms_per_step"][loop] = {m: [round(t, 3) for t in v] for m, v in res.items()}
        if loop == "captured":
            entry["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
        med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
        spread = max(max(v) - min(v) for v in res.values())
        entry["union_minus_one_line"] = round(med["line_and_union"] - med["one_line"], 3)
        entry["second_line_minus_one_line"] = round(med["two_lines"] - med["one_line"], 3)
        entry["largest_spread_of_a_mode"] = round(spread, 3)
        print(f"{loop} loop, ms per denoising step", flush=True)
        for m in MODES:
            print(f"  {m:15s}: " + "  ".join(f"{t:.3f}" for t in res[m]), flush=True)
        print(f"  union tower: +{entry['union_minus_one_line']:.3f}   second text line: +{entry['second_line_minus_one_line']:.3f}   "
              f"(medians; largest spread of a mode {spread:.3f})", flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["union_tower"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
