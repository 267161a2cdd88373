"""What a guider on a true-CFG call (``pipe.guider``: a guidance interval, projected guidance) costs or saves per call on the real-width
stack: FLUX.1-dev 19+38 blocks + the RepText tower (6 double blocks), 1024², one masked text line, random weights, captured 28-step
loop. Four modes, alternated `--repeats` times in one process, the order reversed every other repeat:
  (a) plain ....... the plain call at batch 1 (no negative prompt),
  (b) cfg ......... true CFG on all steps (internal batch 2),
  (c) interval .... true CFG with the guidance interval (0, 0.5): 14 steps at batch 2, 14 on the positive half at batch 1,
  (d) projected ... true CFG on all steps with projected guidance (eta = 0, momentum -0.5, a norm threshold): two launches per step
                    in place of one.
The expectations to confirm or refute, all from this run's own figures: ms_per_call(interval) = g·ms_step(cfg) + (n − g)·ms_step(plain),
and ms_step(projected) = ms_step(cfg) up to the spread (the pair moves a few MB beside a 135 ms step). Every figure is kept with the mode
that ran before it.
Prints a table and one JSON line.  python tools/bench_guidance.py [--repeats 3] [--inference-steps 28] [--out profiles/guidance_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("plain", "cfg", "interval", "projected")


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
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'guidance'")
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("bench_guidance.py alternates its modes at least three times")
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.guidance import TrueCFGGuider, guided_steps
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
    mask[:, 1000:2000] = 1.0                                                   # a window of 1008 of 4096 rows
    pipe._region_masks = lambda control_mask, device, dtype: [mask]            # a fixed regional mask, no PIL round trip
    plain = dict(height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5, controlnet_conditioning_scale=1.0,
                 controlnet_conditioning_step=30, control_mask=[0], output_type="latent", prompt_embeds=r(1, T, 4096),
                 pooled_prompt_embeds=r(1, 768), control_image=[r(1, N, 128)], latents=r(1, N, 64))
    cfg = dict(plain, negative_prompt_embeds=r(1, T, 4096), negative_pooled_prompt_embeds=r(1, 768), true_cfg_scale=3.5)
    interval = TrueCFGGuider(stop=0.5)
    guiders = {"plain": None, "cfg": None, "interval": interval, "projected": TrueCFGGuider(eta=0.0, momentum=-0.5, norm_threshold=10.0)}
    calls = {"plain": plain, "cfg": cfg, "interval": cfg, "projected": cfg}

    def run(m):
        pipe.guider = guiders[m]
        return pipe(**calls[m])

    result = {"tool": "bench_guidance", "device": torch.cuda.get_device_name(0),
              "shape": "1024x1024, T = 512, full depth, one masked text line, batch 1, captured loop", "inference_steps": steps}
    for m in MODES:                                                            # remember, capture, replay once
        for _ in range(3):
            run(m)
    res, ran_after = {m: [] for m in MODES}, {m: [] for m in MODES}
    for k in range(args.repeats):
        order = MODES if k % 2 == 0 else MODES[::-1]
        for j, m in enumerate(order):
            res[m].append(timed_call(lambda: run(m)))
            ran_after[m].append(order[j - 1])
    n, gsteps = steps, len(guided_steps(steps, interval))
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    entry = result["ms_per_call"] = {m: [round(t, 2) for t in v] for m, v in res.items()}
    result["ms_per_step"] = {m: [round(t / n, 3) for t in v] for m, v in res.items()}
    entry["ran_after"] = ran_after
    entry["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
    entry["spread"] = {m: round(max(v) - min(v), 2) for m, v in res.items()}
    predicted = gsteps * med["cfg"] / n + (n - gsteps) * med["plain"] / n
    entry["interval_guided_steps"] = gsteps
    entry["interval_predicted"] = round(predicted, 2)
    entry["interval_minus_predicted"] = round(med["interval"] - predicted, 2)
    entry["interval_over_cfg"] = round(med["interval"] / med["cfg"], 4)
    entry["projected_minus_cfg"] = round(med["projected"] - med["cfg"], 2)
    entry["projected_minus_cfg_per_step"] = round((med["projected"] - med["cfg"]) / n, 4)
    print("captured loop, ms per call (ms per step)", flush=True)
    for m in MODES:
        print(f"  {m:9s}: " + "  ".join(f"{t:.2f} ({t / n:.3f}, after {p})" for t, p in zip(res[m], ran_after[m])) + f"   spread {entry['spread'][m]:.2f}",
              flush=True)
    print(f"  interval (0, 0.5): {gsteps} of {n} steps guided; predicted from this run's plain and cfg medians {predicted:.2f} ms per call, measured "
          f"{med['interval']:.2f} ({entry['interval_minus_predicted']:+.2f}); interval / cfg = {entry['interval_over_cfg']:.4f}", flush=True)
    print(f"  projected minus cfg: {entry['projected_minus_cfg']:+.2f} ms per call = {entry['projected_minus_cfg_per_step']:+.4f} ms per step (two launches "
          f"per step in place of one)", flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["guidance"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
