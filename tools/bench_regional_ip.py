"""Cost of regional image prompts on the real-width stack, InstantX layout (a term in all 19 + 38 blocks, n = 128).

  * rt_ip_attention_rows alone at the double-block shape (N = 4096 rows of the fused q|k|v buffer, gated fp32 accumulate) and at the
    single-block shape (S = 4608 rows at ldq = 7d, bf16 write), H = 24, n = 4 and 128, with four tables: none (rt_ip_attention_gated),
    all ones, a text box (rows 24..39 x columns 16..31 of the 64 x 64 token grid: 1/16 of the rows as 16 runs of 16 contiguous image
    rows, one run per 64-row image line, so the box lies in 16 tiles of 4 workgroups, not in one block) and an empty one. The count
    each is to be compared to: rows touched x bytes per row (q read + o read/write) + K/V of the workgroups that stage, over the copy
    rate, and the launch floor for the empty table. The variants are alternated, `--repeats` rounds, every round reported.
  * ms per denoising step from the captured loop (1024^2, batch 1, random weights), alternated in pairs (the pipeline keeps two
    graphs): plain | global image prompt, global | the same with a mask, global | global plus two line image prompts.
Prints tables and one JSON line.  python tools/bench_regional_ip.py [--repeats 3] [--inference-steps 28] [--kernel-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import reptext_amd.ops as ops
from bench_ip_adapter import COPY_TBS, adapter_sd_instantx, timed

GRID = 64                                # 64 x 64 image tokens at 1024^2
BOX = (24, 40, 16, 32)                   # token rows, token columns: 16 x 16 = 256 = 1/16 of the 4096 image rows


def box_table(T, dev):
    m = torch.zeros(GRID, GRID, device=dev)
    m[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 1.0
    return torch.cat([torch.zeros(T, device=dev), m.reshape(-1)]).reshape(1, -1)


def expected_bytes(w, rows_per_wg, row_bytes, kv_bytes, H):
    """Rows touched x bytes per row, in whole 16-row tiles, plus K/V once per (head, workgroup that stages)."""
    if w is None:
        n = -(-row_bytes[1] // rows_per_wg)
        return row_bytes[1] * row_bytes[0] + kv_bytes, n
    on = (w[0] != 0).cpu()
    R = on.numel()
    pad = (-R) % rows_per_wg
    on = torch.cat([on, torch.zeros(pad, dtype=torch.bool)])
    tiles = int(on.reshape(-1, 16).any(dim=1).sum())
    wgs = int(on.reshape(-1, rows_per_wg).any(dim=1).sum())
    return tiles * 16 * row_bytes[0] + (kv_bytes if wgs else 0), wgs


def kernel_bench(dev, repeats, N=4096, T=512, H=24):
    d, S = H * 128, T + N
    nbuf = 4
    big = [torch.randn(1, S, 7 * d, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
    term = [torch.empty(1, S, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
    qkv = [b.view(-1)[: N * 3 * d].view(1, N, 3 * d) for b in big]
    x = [torch.randn(1, S, d, device=dev) for _ in range(nbuf)]
    wq = torch.ones(128, device=dev, dtype=torch.bfloat16)
    gate = torch.randn(1, 6 * d, device=dev)[:, 2 * d : 3 * d]
    res = {}
    for n in (4, 128):
        k = torch.nn.functional.normalize(torch.randn(1, n, H, 128, device=dev), dim=-1).mul(128 ** 0.5).reshape(1, n, d).to(torch.bfloat16)
        v = torch.randn(1, n, d, device=dev).to(torch.bfloat16)
        wg = 256 if n > 96 else 128
        kvb = 2 * n * d * 2
        shapes = {
            "double_gated_f32_accumulate": (N, 0, (d * (2 + 4 + 4), N), lambda j, w: ops.ip_attention_gated(
                qkv[j][..., :d], wq, k, v, x[j][:, T:], H, ip_scale=0.7, gate=gate, accumulate=True, row_weights=w)),
            "single_bf16_write": (S, T, (d * (2 + 2), S), lambda j, w: ops.ip_attention_gated(
                big[j][..., 2 * d : 3 * d], wq, k, v, term[j], H, ip_scale=0.7, row_weights=w)),
        }
        for shape, (R, Tt, row_bytes, fn) in shapes.items():
            tables = {"unweighted": None, "ones": torch.ones(1, R, device=dev), "box_1_16": box_table(Tt, dev), "empty": torch.zeros(1, R, device=dev)}
            runs = {name: [] for name in tables}
            for _ in range(repeats):                                        # alternate the variants; every round is reported
                for name, w in tables.items():
                    i = [0]

                    def one():
                        fn(i[0] % nbuf, w)
                        i[0] += 1
                    runs[name].append(timed(one, 5 * nbuf, warm=nbuf) * 1e6)
            print(f"n = {n:3d} {shape:30s}  us per launch (rounds)          expected bytes -> us at {COPY_TBS} TB/s    workgroups that stage", flush=True)
            for name, w in tables.items():
                nbytes, wgs = expected_bytes(w, wg, row_bytes, kvb, H)
                # write mode still writes the zeros of the rows worth nothing: o bytes of every row
                if w is not None and shape == "single_bf16_write":
                    nbytes += int((w[0] == 0).sum()) * d * 2 if name != "ones" else 0
                floor = nbytes / (COPY_TBS * 1e12) * 1e6
                res[f"n{n}_{shape}_{name}"] = {"us": [round(t, 2) for t in runs[name]], "expected_bytes": nbytes, "expected_us": round(floor, 2),
                                               "staging_workgroups_per_head": wgs}
                print(f"    {name:12s} " + "  ".join(f"{t:7.1f}" for t in runs[name]) + f"      {nbytes:12d} -> {floor:6.1f}      {wgs}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inference-steps", type=int, default=28)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regional_ip.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_regional_ip", "device": torch.cuda.get_device_name(0), "kernel": kernel_bench(dev, args.repeats)}
    if not args.kernel_only:
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
        pipe.load_ip_adapter(adapter_sd_instantx(tr, 128, dev, seed=138))
        N, T, steps = 4096, 512, args.inference_steps
        g = torch.Generator().manual_seed(1)
        r = lambda *s: torch.randn(*s, generator=g).to(dev, bf16)

        def token_box(r0, r1, c0, c1):
            m = torch.zeros(GRID, GRID, device=dev, dtype=bf16)
            m[r0:r1, c0:c1] = 1.0
            return m.reshape(1, N, 1)

        kw = dict(prompt_embeds=r(1, T, 4096), pooled_prompt_embeds=r(1, 768), height=1024, width=1024, num_inference_steps=steps, guidance_scale=3.5,
                  control_image=[r(1, N, 128), r(1, N, 128)], control_mask=[token_box(*BOX), token_box(44, 52, 8, 56)],
                  controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30, latents=r(1, N, 64), output_type="latent")
        emb, l1, l2 = r(1, 1, 1152), r(1, 1152), r(1, 1152)
        left = torch.zeros(GRID, GRID, device=dev, dtype=bf16)
        left[:, : GRID // 2] = 1.0
        modes = {"plain": {}, "global": dict(ip_adapter_image_embeds=emb),
                 "global_masked": dict(ip_adapter_image_embeds=emb, ip_adapter_mask=left.reshape(1, N, 1)),
                 "global_two_lines": dict(ip_adapter_image_embeds=emb, control_ip_adapter_image_embeds=[l1, l2])}
        result["pipeline"] = []
        for pair in (("plain", "global"), ("global", "global_masked"), ("global", "global_two_lines")):
            pipe.__dict__.get("_graph_cache", {}).clear()
            for m in pair:                                                  # eager, then capture
                pipe(**kw, **modes[m])
                pipe(**kw, **modes[m])
            torch.cuda.synchronize()
            res = {m: [] for m in pair}
            for _ in range(args.repeats):
                for m in pair:
                    res[m].append(timed(lambda: pipe(**kw, **modes[m]), 1, warm=0) / steps * 1e3)
            graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
            result["pipeline"].append({"graphs": graphs, "ms_per_step": {m: [round(t, 3) for t in v] for m, v in res.items()}})
            for m in pair:
                print(f"  ms per denoising step, {m:18s}: " + "  ".join(f"{t:.3f}" for t in res[m]) + f"   ({graphs} captured graphs)", flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
