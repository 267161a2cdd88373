"""CLIP vision encoder cost at the ViT-L/14 shape (24 layers, d = 1024, 16 heads, 257 tokens, random weights), B = 1 and B = 4:
  * the encoder as shipped: one rt_attention_hd64 launch per layer;
  * the same forward with attention routed through text_encoders._attention_heads, the per-(batch, head) GEMM -> softmax ->
    transpose -> GEMM chain that was the only head-dim-64 attention before, with the tokens padded to 320;
  three alternating timed runs each after warm-up, and the two outputs compared;
  * rt_attention_hd64 alone at (B = 1, S = 257, H = 16) and (B = 4, ...), on a rotating set of buffers; `--kernel-only` stops here
    (the form to run under `rocprofv3 --kernel-trace --stats`; RT_HD64_WAVES = 1 | 2 | 4 forces the workgroup size for an A/B).
Prints a table and one JSON line.  python tools/bench_image_encoder.py [--repeats 3] [--layers 24] [--kernel-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops
from reptext_amd import text_encoders as te
from reptext_amd.image_encoder import CLIPVisionModelWithProjection


class AssembledAttention(CLIPVisionModelWithProjection):
    """The same model with its attention as text_encoders.CLIPTextModel runs it: tokens padded to a multiple of 64, one GEMM ->
    rt_softmax_rows_bias -> rt_transpose_bf16 -> GEMM chain per (batch, head)."""

    def _padded_tokens(self, S):
        return (S + 63) // 64 * 64

    def _attention(self, qkv, att, S):
        d, H, Tp = self.config.hidden_size, self.config.num_attention_heads, qkv.shape[1]
        key = (Tp, str(qkv.device))
        if getattr(self, "_scratch_key", None) != key:
            dev = qkv.device
            self._scratch = (torch.empty(Tp, Tp, device=dev, dtype=torch.float32), torch.zeros(Tp, Tp, device=dev, dtype=torch.bfloat16),
                             torch.empty(64, Tp, device=dev, dtype=torch.bfloat16))
            self._scratch_key = key
        te._attention_heads(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], att, H, None, 64 ** -0.5, S, Tp, self._scratch)


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


def kernel_bench(dev, S=257, H=16):
    d = H * 64
    res = {"RT_HD64_WAVES": os.environ.get("RT_HD64_WAVES", "")}
    nbuf = 8
    for B in (1, 4):
        qkv = [torch.randn(B, S, 3 * d, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        out = [torch.empty(B, S, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
        i = [0]

        def one():
            j = i[0] % nbuf
            ops.attention_hd64(qkv[j][..., :d], qkv[j][..., d:2 * d], qkv[j][..., 2 * d:], out[j], H)
            i[0] += 1
        t = sorted(timed(one, 25 * nbuf, warm=nbuf) for _ in range(3))[1]           # median of three; back-to-back launches
        res[f"B{B}"] = {"us": round(t * 1e6, 2)}
        print(f"rt_attention_hd64 B = {B}, S = {S}, H = {H}: {t * 1e6:7.2f} us per launch (back to back)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_encoder.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_image_encoder", "device": torch.cuda.get_device_name(0), "layers": args.layers, "kernel": kernel_bench(dev)}
    if args.kernel_only:
        print(json.dumps(result), flush=True)
        return
    cfg = dict(hidden_size=1024, intermediate_size=4096, projection_dim=768, num_hidden_layers=args.layers, num_attention_heads=16,
               image_size=224, patch_size=14)
    fused = CLIPVisionModelWithProjection(**cfg, device=dev, dtype=torch.bfloat16).random_init_(seed=0)
    g = torch.Generator(device=dev).manual_seed(0)
    assembled = AssembledAttention(**cfg, device=dev, dtype=torch.bfloat16)
    assembled.load_state_dict(fused.state_dict(), strict=True)
    models = {"fused": fused, "assembled": assembled}
    result["encoder"] = {}
    for B in (1, 4):
        pix = torch.randn(B, 3, 224, 224, device=dev, generator=g)
        outs = {m: model(pix).image_embeds.float() for m, model in models.items()}      # also the warm-up (plans, allocator)
        diff = float((outs["fused"] - outs["assembled"]).norm() / outs["assembled"].norm())
        res = {m: [] for m in models}
        for _ in range(args.repeats):
            for m, model in models.items():
                res[m].append(timed(lambda: model(pix), args.iters, warm=1) * 1e3)
        result["encoder"][f"B{B}"] = {"ms": {m: [round(t, 3) for t in v] for m, v in res.items()}, "image_embeds_rel_l2_between_them": round(diff, 5)}
        for m in models:
            print(f"B = {B} encoder, {m:9s} attention: ms per image batch " + "  ".join(f"{t:8.3f}" for t in res[m]), flush=True)
        print(f"B = {B}: image_embeds of the two differ by rel-L2 {diff:.2e}", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
