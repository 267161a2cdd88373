"""LoRA merge cost on the real-width transformer (19+38 blocks, d = 3072, random weights), rank-64 adapter on every block linear:
  * rt_lora_merge_bf16 per shape: time, GB/s (W0 read + W write; factors excluded) and share of the 6.3 TB/s copy rate, with a
    rotating set of weights larger than the 256 MB Infinity Cache so every pass streams from HBM;
  * the whole-model merge (every targeted module re-merged from W0) = the cost of switching the per-call scale, also under
    enable_fp8_linears('ln') where the merged rows are requantised into the e4m3 plans;
  * transformer s/step at 1024² (T = 512, N = 4096) with the adapter active and with it unloaded, alternating runs.
python tools/bench_lora.py [--steps 3]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops

COPY_TBS = 6.3


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


def per_shape(dev, r=64):
    print("shape (N x K), r = 64, out of place        us      GB/s   % of 6.3 TB/s", flush=True)
    for N, K in [(3072, 3072), (9216, 3072), (12288, 3072), (18432, 3072), (3072, 12288), (3072, 15360)]:
        nbuf = max(2, (768 << 20) // (2 * N * K * 2) + 1)
        w0 = [torch.randn(N, K, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        w = [torch.empty_like(x) for x in w0]
        B = (torch.randn(N, r, device=dev) * 0.02).to(torch.bfloat16)
        At = (torch.randn(K, r, device=dev) * 0.02).to(torch.bfloat16)
        i = [0]

        def one():
            j = i[0] % nbuf
            ops.lora_merge_(w[j], w0[j], [(B, At, 0.5)])
            i[0] += 1
        t = timed(one, 4 * nbuf)
        gbs = 4.0 * N * K / t / 1e9
        print(f"{N:6d} x {K:6d}                        {t * 1e6:8.1f}  {gbs:8.0f}   {100 * gbs / (COPY_TBS * 1e3):5.1f} %", flush=True)
        del w0, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    per_shape(dev)

    from reptext_amd.modules import Lin
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(num_layers=19, num_single_layers=38, guidance_embeds=True, device=dev, dtype=torch.bfloat16).random_init_(1)
    g = torch.Generator(device=dev).manual_seed(2)
    sd, elems = {}, 0
    for name, m in tr.named_modules():
        if isinstance(m, Lin) and name.startswith(("transformer_blocks.", "single_transformer_blocks.")):
            sd[f"transformer.{name}.lora_A.weight"] = (torch.randn(64, m.in_features, generator=g, device=dev) / m.in_features ** 0.5).to(torch.bfloat16)
            sd[f"transformer.{name}.lora_B.weight"] = (torch.randn(m.out_features, 64, generator=g, device=dev) * 0.01).to(torch.bfloat16)
            elems += m.in_features * m.out_features
    t0 = time.perf_counter()
    tr.load_lora_adapter(sd, adapter_name="a")
    torch.cuda.synchronize()
    print(f"load_lora_adapter (pad factors, W0 copies, first merge) of {len(sd) // 2} modules: {time.perf_counter() - t0:.2f} s; "
          f"W0 copies {elems * 2 / 1e9:.1f} GB", flush=True)
    scales = iter([0.5, 1.0] * 100)
    t = timed(lambda: tr._lora.sync(next(scales)), 6)
    print(f"whole-model merge (= switching the call scale): {t * 1e3:.2f} ms for {elems / 1e9:.2f} G elements, "
          f"{4.0 * elems / t / 1e9:.0f} GB/s ({100 * 4.0 * elems / t / (COPY_TBS * 1e12):.1f} % of 6.3 TB/s)", flush=True)
    t_noop = timed(lambda: tr._lora.sync(1.0), 20)
    print(f"sync with an unchanged scale (host check only): {t_noop * 1e6:.0f} us", flush=True)
    tr.enable_fp8_linears("ln")
    t8 = timed(lambda: tr._lora.sync(next(scales)), 6)
    print(f"whole-model merge under enable_fp8_linears('ln') (+ requantising {len(tr._fp8_rows())} modules' e4m3 rows): "
          f"{t8 * 1e3:.2f} ms", flush=True)
    tr.enable_fp8_linears(False)

    T, N = 512, 4096
    x = torch.randn(1, N, 64, device=dev).to(torch.bfloat16)
    kw = dict(encoder_hidden_states=torch.randn(1, T, 4096, device=dev).to(torch.bfloat16),
              pooled_projections=torch.randn(1, 768, device=dev).to(torch.bfloat16), timestep=torch.full((1,), 0.5, device=dev),
              img_ids=torch.zeros(N, 3, device=dev), txt_ids=torch.zeros(T, 3, device=dev), guidance=torch.full((1,), 3.5, device=dev),
              return_dict=False)
    step = lambda: tr(hidden_states=x, **kw)
    res = {"with adapter": [], "without": []}
    for rep in range(3):
        for which in ("with adapter", "without"):
            if which == "without":
                tr.unload_lora()
            elif getattr(tr, "_lora", None) is None:
                tr.load_lora_adapter(sd, adapter_name="a")
            res[which].append(timed(step, args.steps, warm=1))
    for k, v in res.items():
        print(f"transformer step at 1024² {k:13s}: " + "  ".join(f"{t:.4f}" for t in v) + " s", flush=True)


if __name__ == "__main__":
    main()
