"""CLIP vision encoder cost at the ViT-L/14 shape (24 layers, d = 1024, 16 heads, 257 tokens, random weights), B = 1 and B = 4:
  * the encoder as shipped: one rt_attention_hd64 launch per layer;
  * the same forward with attention routed through encoder_common._attention_heads, the per-(batch, head) GEMM -> softmax ->
    transpose -> GEMM chain that was the only head-dim-64 attention before, with the tokens padded to 320;
  three alternating timed runs each after warm-up, and the two outputs compared;
  * rt_attention_hd64 alone at (B = 1, S = 257, H = 16) and (B = 4, ...), on a rotating set of buffers; `--kernel-only` stops here
    (the form to run under `rocprofv3 --kernel-trace --stats`; RT_HD64_WAVES = 1 | 2 | 4 forces the workgroup size for an A/B).
`--siglip` measures the SigLIP-so400m encoder instead (27 layers, d = 1152, 16 heads of 72, 729 tokens from a 384 x 384 image, random
weights), B = 1 and B = 4: ms per forward, three timed runs each, and rt_attention_hd72 alone at the self-attention shape (Sq = Sk =
729) and at the pooling call (Sq = 1, one probe row shared by the batch). There is no earlier form to compare against.
Prints a table and one JSON line.  python tools/bench_image_encoder.py [--siglip] [--repeats 3] [--layers 24 | 27] [--kernel-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import reptext_amd.ops as ops
from reptext_amd.encoder_common import _AssembledAttention
from reptext_amd.image_encoder import CLIPVisionModelWithProjection


class AssembledAttention(_AssembledAttention, CLIPVisionModelWithProjection):
    """The same model with its attention as text_encoders.CLIPTextModel runs it, without a mask: tokens padded to a multiple of 64, one
    GEMM -> rt_softmax_rows_bias -> rt_transpose_bf16 -> GEMM chain per (batch, head)."""


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


def kernel_bench(dev, hd, S, H=16):
    """rt_attention_hd<hd> alone on a rotating set of buffers, B = 1 and 4: the self-attention call, and for 72 the pooling call too."""
    d, env = H * hd, f"RT_HD{hd}_WAVES"
    attention = ops.attention_hd64 if hd == 64 else ops.attention_hd72
    res = {env: os.environ.get(env, "")}
    nbuf = 8
    for B in (1, 4):
        qkv = [torch.randn(B, S, 3 * d, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        out = [torch.empty(B, S, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
        pooled = [torch.empty(B, 1, d, device=dev, dtype=torch.bfloat16) for _ in range(nbuf)]
        i = [0]

        def self_attention():
            j = i[0] % nbuf
            attention(qkv[j][..., :d], qkv[j][..., d:2 * d], qkv[j][..., 2 * d:], out[j], H)
            i[0] += 1

        def pooling():
            j = i[0] % nbuf
            attention(qkv[j][:1, :1, :d], qkv[j][..., d:2 * d], qkv[j][..., 2 * d:], pooled[j], H)
            i[0] += 1
        res[f"B{B}"] = {}
        for name, fn in (("self", self_attention), ("pooling", pooling))[:1 if hd == 64 else 2]:
            t = sorted(timed(fn, 25 * nbuf, warm=nbuf) for _ in range(3))[1]         # median of three; back-to-back launches
            res[f"B{B}"]["us" if hd == 64 else name + "_us"] = round(t * 1e6, 2)
            print(f"rt_attention_hd{hd} B = {B}, Sk = {S}, H = {H}, {name:7s}: {t * 1e6:7.2f} us per launch (back to back)", flush=True)
    return res


def main_siglip(args, dev):
    from reptext_amd.image_encoder import SiglipVisionModel

    layers = args.layers if args.layers is not None else 27
    result = {"tool": "bench_image_encoder", "encoder_model": "siglip-so400m-patch14-384 shape, random weights",
              "device": torch.cuda.get_device_name(0), "layers": layers, "kernel": kernel_bench(dev, 72, 729)}
    if args.kernel_only:
        print(json.dumps(result), flush=True)
        return
    model = SiglipVisionModel(num_hidden_layers=layers, device=dev, dtype=torch.bfloat16).random_init_(seed=0)
    g = torch.Generator(device=dev).manual_seed(0)
    result["encoder"] = {}
    for B in (1, 4):
        pix = torch.randn(B, 3, 384, 384, device=dev, generator=g)
        pooled = model(pix).pooler_output                                            # also the warm-up (plans, allocator)
        assert bool(torch.isfinite(pooled.float()).all())
        ms = [timed(lambda: model(pix), args.iters, warm=1) * 1e3 for _ in range(args.repeats)]
        result["encoder"][f"B{B}"] = {"ms": [round(t, 3) for t in ms]}
        print(f"B = {B} SigLIP encoder: ms per forward " + "  ".join(f"{t:8.3f}" for t in ms), flush=True)
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="default: 24 (CLIP ViT-L/14), 27 (--siglip)")
    ap.add_argument("--siglip", action="store_true", help="the SigLIP-so400m encoder (rt_attention_hd72) instead of CLIP ViT-L/14")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_encoder.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    if args.siglip:
        return main_siglip(args, dev)
    args.layers = 24 if args.layers is None else args.layers
    result = {"tool": "bench_image_encoder", "device": torch.cuda.get_device_name(0), "layers": args.layers, "kernel": kernel_bench(dev, 64, 257)}
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
