"""What stochastic sampling (the scheduler's ``stochastic_sampling``) costs per denoising step on the real-width stack: FLUX.1-dev 19+38
blocks + the RepText tower (6 double blocks), 1024², one masked text line, random weights, the captured loop.
  (a) ms per step: the Euler scheduler against the same scheduler with the switch on at `--inference-steps`, alternated `--repeats`
      times in one process, every figure kept with the mode that ran before it, the order reversed every other repeat. The expectation
      from counting: 65 k Philox calls of ten rounds and four transcendentals per group of four, beside a ~68 ms step — nothing should
      show per step.
  (b) the step kernel alone at the same state size (1 x 4096 x 64): the Euler instantiation against the stochastic one (eta = 1 and
      eta = 0.5), a captured graph of `--kernel-iters` launches between two events, alternated `--repeats` times.
Asserts nothing. Prints a table and one JSON line.
python tools/bench_stochastic.py [--repeats 3] [--inference-steps 28] [--out profiles/stochastic_bench.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("euler", "stochastic")


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
    ap.add_argument("--kernel-iters", type=int, default=500)
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'stochastic'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stochastic.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd import ops
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**reptext_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=1)
    schedulers = {"euler": FlowMatchEulerDiscreteScheduler(), "stochastic": FlowMatchEulerDiscreteScheduler(stochastic_sampling=True)}
    pipe = P.FluxControlNetPipeline(schedulers["euler"], None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    P.GRAPH_CACHE_MAX = 2                                                      # one captured loop per mode, none evicted
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(1, N, 1, device=dev, dtype=bf16)
    mask[:, 1000:2000] = 1.0                                                   # a window of 1008 of 4096 rows
    pipe._region_masks = lambda control_mask, device, dtype: [mask]            # a fixed regional mask, no PIL round trip
    base = dict(height=1024, width=1024, guidance_scale=3.5, controlnet_conditioning_scale=1.0, controlnet_conditioning_step=10 ** 6,
                control_mask=[0], output_type="latent", prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768),
                control_image=[r(1, N, 128)], latents=r(1, N, 64), num_inference_steps=steps)
    seeds = iter(range(1000, 10 ** 6))

    def call(mode):
        pipe.scheduler = schedulers[mode]
        pipe(**base, generator=torch.Generator().manual_seed(next(seeds)))     # another seed every call: the same graph replays

    result = {"tool": "bench_stochastic", "device": torch.cuda.get_device_name(0), "inference_steps": steps,
              "shape": "1024x1024, T = 512, full depth, one masked text line, random weights, captured loop"}
    for m in MODES:                                                            # remember, capture, replay once
        for _ in range(3):
            call(m)
    res, ran_after = {m: [] for m in MODES}, {m: [] for m in MODES}
    for k in range(args.repeats):
        order = MODES if k % 2 == 0 else MODES[::-1]
        for j, m in enumerate(order):
            res[m].append(timed_call(lambda: call(m)))
            ran_after[m].append(order[j - 1])
    med = lambda v: sorted(v)[len(v) // 2]
    result["ms_per_call"] = {m: [round(t, 2) for t in v] for m, v in res.items()}
    result["ms_per_step"] = {m: [round(t / steps, 3) for t in v] for m, v in res.items()}
    result["spread_ms_per_step"] = {m: round((max(v) - min(v)) / steps, 3) for m, v in res.items()}
    result["ran_after"] = ran_after
    result["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
    result["median_step_stochastic_over_euler"] = round(med(res["stochastic"]) / med(res["euler"]), 4)
    print("ms per denoising step (ms per call)", flush=True)
    for m in MODES:
        print(f"  {m:10s}: " + "  ".join(f"{t / steps:.3f} ({t:.1f}, after {p})" for t, p in zip(res[m], ran_after[m]))
              + f"   spread {result['spread_ms_per_step'][m]:.3f}", flush=True)

    # (b) the kernel alone; the state is reset by nothing: the timing does not depend on its values (finite: sigma_next < 1 contracts)
    x32, xb, v = torch.randn(1, N, 64, device=dev), torch.zeros(1, N, 64, device=dev, dtype=bf16), r(1, N, 64)
    rng = torch.tensor([[42, 0]], dtype=torch.int64, device=dev)
    kernels = {"euler": lambda: ops.euler_step_f32_(x32, v, -1e-6, xb),
               "stochastic eta=1": lambda: ops.stochastic_step_f32_(x32, v, ops.StochasticArgs(rng, 0.5, 1.0, 0.0, 3), 0.45, xb),
               "stochastic eta=0.5": lambda: ops.stochastic_step_f32_(x32, v, ops.StochasticArgs(rng, 0.5, 0.5, math.sqrt(0.75), 3), 0.45, xb)}
    us, graphs = {k: [] for k in kernels}, {}
    for name, fn in kernels.items():                                           # a graph of back-to-back launches: no host enqueue in the figure
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.kernel_iters):
                fn()
        graphs[name].replay()
    for k in range(args.repeats):
        for name in (list(kernels) if k % 2 == 0 else list(kernels)[::-1]):
            us[name].append(timed_call(graphs[name].replay) * 1e3 / args.kernel_iters)
    result["kernel_us_per_launch_back_to_back"] = {k: [round(t, 2) for t in v] for k, v in us.items()}
    result["kernel_note"] = f"a captured graph of {args.kernel_iters} launches on one stream between two events: launch gaps included, host enqueue not"
    print("step kernel alone, us per launch (back to back in a graph)", flush=True)
    for name, v in us.items():
        print(f"  {name:18s}: " + "  ".join(f"{t:.2f}" for t in v), flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["stochastic"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
