"""What the second-order multistep scheduler costs per denoising step, and what it buys per step count, on the real-width stack: FLUX.1-dev
19+38 blocks + the RepText tower (6 double blocks), 1024², one masked text line, random weights, the captured loop.
  (a) ms per step: the Euler scheduler against FlowMatchMultistepScheduler at `--inference-steps`, alternated `--repeats` times in one
      process, every figure kept with the mode that ran before it, the order reversed every other repeat. The expectation to confirm or
      refute: equal — the step kernel gains one fp32 read and one fp32 write of the state (1 MB each) beside a ~70 ms step.
  (b) rel-L2 of the final fp32 latents of each solver at 14, 20 and 28 steps against a 112-step multistep run of the same call.
      RANDOM WEIGHTS: the figures say how the two rules converge on this velocity field, nothing about image quality with a checkpoint.
Asserts nothing. Prints a table and one JSON line.
python tools/bench_solver.py [--repeats 3] [--inference-steps 28] [--out profiles/multistep_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("euler", "multistep")
ERROR_STEPS, REFERENCE_STEPS = (14, 20, 28), 112


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
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'solver'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver.py measures on an MI355X; no GPU is visible")
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16

    import reptext_amd.pipeline as P
    from reptext_amd.config import flux_dev_transformer_config, reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**flux_dev_transformer_config(), device=dev, dtype=bf16).random_init_(seed=0)
    cn = FluxControlNetModel(**reptext_controlnet_config(), device=dev, dtype=bf16).random_init_(seed=1)
    schedulers = {"euler": FlowMatchEulerDiscreteScheduler(), "multistep": FlowMatchMultistepScheduler()}
    pipe = P.FluxControlNetPipeline(schedulers["euler"], None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    P.GRAPH_CACHE_MAX = 2                                                      # one captured loop per solver, none evicted
    N, T, steps = 4096, 512, args.inference_steps
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)
    mask = torch.zeros(1, N, 1, device=dev, dtype=bf16)
    mask[:, 1000:2000] = 1.0                                                   # a window of 1008 of 4096 rows
    pipe._region_masks = lambda control_mask, device, dtype: [mask]            # a fixed regional mask, no PIL round trip
    # the tower is on at every step of every run: the runs differ in the grid and the rule alone
    base = dict(height=1024, width=1024, guidance_scale=3.5, controlnet_conditioning_scale=1.0, controlnet_conditioning_step=10 ** 6,
                control_mask=[0], output_type="latent", prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768),
                control_image=[r(1, N, 128)], latents=r(1, N, 64))

    def call(mode, n):
        pipe.scheduler = schedulers[mode]
        pipe(**base, num_inference_steps=n)
        return pipe._master_latents

    result = {"tool": "bench_solver", "device": torch.cuda.get_device_name(0), "inference_steps": steps,
              "shape": "1024x1024, T = 512, full depth, one masked text line, random weights, captured loop"}
    # (a) the step's cost
    for m in MODES:                                                            # remember, capture, replay once
        for _ in range(3):
            call(m, steps)
    res, ran_after = {m: [] for m in MODES}, {m: [] for m in MODES}
    for k in range(args.repeats):
        order = MODES if k % 2 == 0 else MODES[::-1]
        for j, m in enumerate(order):
            res[m].append(timed_call(lambda: call(m, steps)))
            ran_after[m].append(order[j - 1])
    med = lambda v: sorted(v)[len(v) // 2]
    result["ms_per_call"] = {m: [round(t, 2) for t in v] for m, v in res.items()}
    result["ms_per_step"] = {m: [round(t / steps, 3) for t in v] for m, v in res.items()}
    result["spread_ms_per_step"] = {m: round((max(v) - min(v)) / steps, 3) for m, v in res.items()}
    result["ran_after"] = ran_after
    result["graphs"] = sum(isinstance(v, dict) for v in pipe._graph_cache.values())
    result["median_step_multistep_over_euler"] = round(med(res["multistep"]) / med(res["euler"]), 4)
    print("ms per denoising step (ms per call)", flush=True)
    for m in MODES:
        print(f"  {m:9s}: " + "  ".join(f"{t / steps:.3f} ({t:.1f}, after {p})" for t, p in zip(res[m], ran_after[m]))
              + f"   spread {result['spread_ms_per_step'][m]:.3f}", flush=True)
    # (b) the error per step count; every one of these calls is the first of its signature and runs the eager loop
    pipe.capture_graphs = False
    ref = call("multistep", REFERENCE_STEPS).double()
    rel = lambda x: float((x.double() - ref).norm() / ref.norm())
    result["reference"] = f"{REFERENCE_STEPS}-step multistep run of the same call, fp32 state"
    result["rel_l2_vs_reference"] = {m: {str(n): rel(call(m, n)) for n in ERROR_STEPS} for m in MODES}
    result["note"] = "random weights: convergence of the two rules on this velocity field; nothing measured about image quality with real checkpoints"
    print(f"rel-L2 of the final latents against the {REFERENCE_STEPS}-step multistep run (random weights)", flush=True)
    for m in MODES:
        print(f"  {m:9s}: " + "  ".join(f"{n} steps {result['rel_l2_vs_reference'][m][str(n)]:.3e}" for n in ERROR_STEPS), flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["solver"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
