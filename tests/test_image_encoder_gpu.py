"""GPU tests of the CLIP vision encoder path: rt_attention_hd64 against fp64, against the per-head assembled attention it
replaces and against a CPU emulation of its roundings, rt_patchify_nchw against its definition,
reptext_amd.image_encoder.CLIPVisionModelWithProjection against the REAL transformers class with shared random weights (as
tests/test_text_encoders_gpu.py pins T5 and CLIP-text), and the pipeline's ``ip_adapter_image=`` against
``ip_adapter_image_embeds=``."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402
import small_head_attention as sha  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------------ the kernel
# (B, S, H): a single key, a partial key tile, an exact tile, a tile plus one, the real token count (257), five whole tiles - all
# small enough for one wave per workgroup - and the two smallest 16-head shapes at which the host picks 2 and 4 waves per workgroup
# (>= 256 workgroups of 32 / 64 rows), with a last workgroup whose waves past the first have no row
KERNEL_CASES = [(1, 1, 1), (1, 17, 2), (2, 64, 1), (1, 65, 3), (2, 257, 2), (1, 320, 1), (1, 513, 16), (2, 513, 16)]
SCALE = 64 ** -0.5


def _assembled(gpu, buf, B, S, H):
    """The earlier way: text_encoders._attention_heads (GEMM -> softmax -> transpose -> GEMM per head) on the inputs padded to 64.
    ``buf`` is the harness's guarded buffer; its [B,S,3·64H] interior is what is copied."""
    from reptext_amd import text_encoders as te

    d = H * 64
    Tp = (S + 63) // 64 * 64
    pad = torch.zeros(B, Tp, 3 * d, device=gpu, dtype=torch.bfloat16)
    pad[:, :S] = buf[:, :S, :3 * d].to(gpu)
    out = torch.zeros(B, Tp, d, device=gpu, dtype=torch.bfloat16)
    scratch = (torch.empty(Tp, Tp, device=gpu, dtype=torch.float32), torch.zeros(Tp, Tp, device=gpu, dtype=torch.bfloat16),
               torch.empty(64, Tp, device=gpu, dtype=torch.bfloat16))
    te._attention_heads(pad[..., :d], pad[..., d:2 * d], pad[..., 2 * d:], out, H, None, SCALE, S, Tp, scratch)
    torch.cuda.synchronize()
    return out[:, :S].cpu()


@pytest.mark.parametrize("B, S, H", KERNEL_CASES)
def test_attention_hd64_vs_fp64_and_the_assembled_path(gpu, B, S, H):
    """rel-L2 against fp64 from the same bf16 values, bounded by 1.5 x the error of the assembled per-head path on the same inputs
    (both round P and the output to bf16; they differ in summation order and in whether P is rounded before or after normalisation)
    and by 1.5 x the error of a CPU emulation of the kernel's roundings, the yardstick and margin rt_attention_hd72 is held to. With
    one key the output is v, bit for bit. The harness (tests/small_head_attention.py) surrounds the inputs with NaN rows and columns
    and requires the same bits from two default launches and from RT_HD64_WAVES = 1, 2, 4.
    Measured on an MI355X, fused / assembled / emulation: (1,1,1) 0 / 0 / 0; (1,17,2) 2.024e-3 / 2.429e-3 / 2.024e-3; (2,64,1) 2.051e-3 /
    2.287e-3 / 2.051e-3; (1,65,3) 2.115e-3 / 2.353e-3 / 2.118e-3; (2,257,2) 2.134e-3 / 2.327e-3 / 2.174e-3; (1,320,1) 2.212e-3 / 2.421e-3 /
    2.262e-3; (1,513,16) 2.190e-3 / 2.350e-3 / 2.234e-3; (2,513,16) 2.188e-3 / 2.344e-3 / 2.234e-3."""
    buf, ref, emu, _ = sha.case(64, B, S, S, H, False, 1.0)
    out = sha.fused(gpu, 64, buf, B, S, S, H, False)
    err_f, err_e = rel_l2(out.float(), ref), rel_l2(emu.float(), ref)
    err_a = rel_l2(_assembled(gpu, buf, B, S, H).float(), ref)
    print(f"attention_hd64 B={B} S={S} H={H}: rel-L2 vs fp64 fused {err_f:.3e}, assembled {err_a:.3e}, emulation {err_e:.3e}")
    if S == 1:
        assert sha.is_v(out, buf, 64, B, S, H)
    assert err_f <= 1.5 * err_a, (err_f, err_a)
    assert err_f <= 1.5 * err_e, (err_f, err_e)


@pytest.mark.parametrize("B, S, H", [(1, 65, 3), (2, 257, 2)])
def test_attention_hd64_large_scores(gpu, B, S, H):
    """q scaled so that the largest scale·score exceeds 100: fp32 exp overflows at 88.7 unless the row maximum is subtracted.
    Same two bounds, finite outputs. Measured, fused / assembled / emulation: (1,65,3) 9.456e-4 / 1.150e-3 / 9.456e-4 at a largest
    scale·score of 216; (2,257,2) 9.178e-4 / 1.152e-3 / 9.239e-4 at 243."""
    buf, ref, emu, smax = sha.case(64, B, S, S, H, False, 48.0)
    assert smax > 100.0, smax
    err_f, err_e = rel_l2(sha.fused(gpu, 64, buf, B, S, S, H, False).float(), ref), rel_l2(emu.float(), ref)
    err_a = rel_l2(_assembled(gpu, buf, B, S, H).float(), ref)
    print(f"attention_hd64 large scores B={B} S={S} H={H} (max scale*score {smax:.0f}): rel-L2 vs fp64 fused {err_f:.3e}, assembled {err_a:.3e}, "
          f"emulation {err_e:.3e}")
    assert err_f <= 1.5 * err_a, (err_f, err_a)
    assert err_f <= 1.5 * err_e, (err_f, err_e)


def test_attention_hd64_wrapper_refuses_what_the_kernel_cannot_take(gpu):
    from reptext_amd import native, ops

    buf = torch.zeros(1, 16, 384, device=gpu, dtype=torch.bfloat16)
    o = torch.zeros(1, 16, 128, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="share shape and strides"):
        ops.attention_hd64(buf[..., :128], buf[..., 128:256], buf[:, :8, 256:], o, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_hd64(buf.cpu()[..., :128], buf.cpu()[..., 128:256], buf.cpu()[..., 256:], o, 2)
    big = torch.zeros(1, native.RT_ATTENTION_HD64_MAX_S + 1, 192, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rows"):
        ops.attention_hd64(big[..., :64], big[..., 64:128], big[..., 128:], torch.zeros_like(big[..., :64]), 1)
    torch.cuda.synchronize()
    assert not o.any()


@pytest.mark.parametrize("B, G, p, dtype", [(2, 4, 14, torch.float32), (1, 5, 14, torch.bfloat16), (1, 4, 16, torch.float32)])
def test_patchify_is_the_unfolded_convolution_input(gpu, B, G, p, dtype):
    """Exact: the kernel only moves values and rounds fp32 to bf16. 3p² = 588 -> Kp 640 (zero tail), 768 -> 768 (none)."""
    from reptext_amd import ops

    x = torch.randn(B, 3, G * p, G * p, generator=torch.Generator().manual_seed(G * p)).to(dtype)
    out = ops.patchify_nchw(x.to(gpu), p).cpu()
    k = 3 * p * p
    Kp = (k + 63) // 64 * 64
    want = torch.nn.functional.unfold(x.float(), kernel_size=p, stride=p).transpose(1, 2).to(torch.bfloat16)     # [B, G², 3p²], (c, dy, dx) order
    assert out.shape == (B, G * G, Kp) and out.dtype == torch.bfloat16
    assert torch.equal(out[..., :k], want) and not out[..., k:].any()


# ------------------------------------------------------------------------------------------------------------------ the model
def _hf_vision(cfg_kw, seed):
    """transformers' CLIPVisionModelWithProjection in fp32 on the CPU, every weight rounded to bf16 and given an exercised range:
    LayerNorm weights 1 + 0.2·randn and biases 0.1·randn as in test_text_encoders_gpu.py; the Linear / patch weights at
    1/sqrt(fan-in) and the embeddings at unit scale, so that attention and MLP outputs are as large as the stream they are added to
    (the default init leaves them two orders below it, where no error of theirs would show)."""
    from transformers import CLIPVisionConfig
    from transformers import CLIPVisionModelWithProjection as HF

    torch.manual_seed(seed)
    hf = HF(CLIPVisionConfig(**cfg_kw)).eval()
    bf = lambda t: t.to(torch.bfloat16).float()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(bf(1.0 + 0.2 * torch.randn_like(p)))
            elif n.endswith("bias"):
                p.copy_(bf(0.1 * torch.randn_like(p)))
            elif "embedding" in n and p.dim() <= 2:
                p.copy_(bf(torch.randn_like(p)))
            else:
                p.copy_(bf(torch.randn_like(p) * (p[0].numel() ** -0.5)))
    return hf


VIT_TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, image_size=56, patch_size=14, projection_dim=64)
MODEL_CASES = {
    "a": (VIT_TINY, 1),                                                          # 17 tokens, K 588 -> 640
    "b": (dict(VIT_TINY, image_size=70), 2),                                     # 26 tokens, batch 2
    "c": (dict(VIT_TINY, image_size=64, patch_size=16), 1),                      # K = 768: no padding
    "d": (dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16, image_size=224, patch_size=14,
               projection_dim=768), 1),                                          # ViT-L/14 width, the real S = 257
}


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_vision_model_vs_transformers(gpu, name):
    """image_embeds and last_hidden_state rel-L2 < 1e-2 against transformers in fp32: the project's bound for bf16 storage between
    stages against an fp32 run (tests/test_text_encoders_gpu.py). Measured (image_embeds / last_hidden_state): (a) 3.9e-3 / 4.0e-3,
    (b) 4.1e-3 / 3.9e-3, (c) 4.3e-3 / 3.5e-3, (d) 3.8e-3 / 3.2e-3."""
    from reptext_amd.image_encoder import CLIPVisionModelWithProjection

    cfg_kw, B = MODEL_CASES[name]
    hf = _hf_vision(cfg_kw, seed=ord(name))
    pix = torch.randn(B, 3, cfg_kw["image_size"], cfg_kw["image_size"], generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).float()
    with torch.no_grad():
        r = hf(pixel_values=pix)
    mine = CLIPVisionModelWithProjection(**cfg_kw, layer_norm_eps=hf.config.layer_norm_eps, device=gpu, dtype=torch.bfloat16)
    mine.load_state_dict(hf.state_dict(), strict=True)
    o = mine(pix.to(gpu))
    S = (cfg_kw["image_size"] // cfg_kw["patch_size"]) ** 2 + 1
    assert o.image_embeds.shape == (B, cfg_kw["projection_dim"]) and o.image_embeds.dtype == torch.bfloat16
    assert o.last_hidden_state.shape == (B, S, cfg_kw["hidden_size"]) and o.last_hidden_state.dtype == torch.bfloat16
    assert o[0] is o.image_embeds and o[1] is o.last_hidden_state
    e_e, e_h = rel_l2(o.image_embeds.float().cpu(), r.image_embeds), rel_l2(o.last_hidden_state.float().cpu(), r.last_hidden_state)
    print(f"CLIP vision ({name}) B={B} S={S}: image_embeds {e_e:.3e}, last_hidden_state {e_h:.3e} vs transformers fp32")
    assert e_e < 1e-2 and e_h < 1e-2
    # bf16 pixel_values are the same values here (pix is bf16-representable): the same bits
    o16 = mine(pix.to(gpu, torch.bfloat16))
    assert torch.equal(o16.image_embeds, o.image_embeds) and torch.equal(o16.last_hidden_state, o.last_hidden_state)


# ------------------------------------------------------------------------------------------------------------------ the pipeline
E = 64


def _tiny_encoder(gpu, seed):
    from reptext_amd.image_encoder import CLIPVisionModelWithProjection

    return CLIPVisionModelWithProjection(**dict(VIT_TINY, num_hidden_layers=2, projection_dim=E), device=gpu, dtype=torch.bfloat16).random_init_(seed)


def _photo(seed, w=90, h=70):
    from PIL import Image

    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))


def test_pipeline_image_prompt_is_the_embeds_path(gpu):
    from test_ip_adapter_gpu import SMALL_T, _pipe, _pipe_inputs

    from reptext_amd.image_encoder import clip_preprocess

    pipe, _, _ = _pipe(gpu, 401)
    kw, _ = _pipe_inputs(gpu, 402, steps=2)
    pipe.load_ip_adapter(ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=E, seed=403))
    pipe.set_ip_adapter_scale([1.0, -0.7])
    img1, img2 = _photo(1), _photo(2)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):   # no encoder: today's refusal
        pipe(**kw, ip_adapter_image=img1)
    pipe.image_encoder = _tiny_encoder(gpu, 404)
    pipe.capture_graphs = False
    base = pipe(**kw).images.clone()
    emb1 = pipe.encode_image(img1, gpu)
    assert emb1.shape == (1, E) and emb1.dtype == torch.bfloat16 and emb1.is_cuda
    assert pipe.encode_image(img1, gpu, num_images_per_prompt=3).shape == (3, E)
    via_embeds = pipe(**kw, ip_adapter_image_embeds=emb1).images.clone()
    via_image = pipe(**kw, ip_adapter_image=img1).images.clone()
    assert torch.equal(via_image, via_embeds) and not torch.equal(via_image, base)
    other = pipe(**kw, ip_adapter_image=[img2]).images.clone()
    assert not torch.equal(other, via_image)
    # a tensor is taken as pixel_values
    assert torch.equal(pipe(**kw, ip_adapter_image=clip_preprocess(img1, size=56)).images, via_image)
    # a feature extractor, when set, replaces clip_preprocess
    seen = []

    class Extractor:
        def __call__(self, images=None, return_tensors=None):
            seen.append(return_tensors)
            return type("Batch", (), {"pixel_values": clip_preprocess(img2, size=56)})()

    pipe.feature_extractor = Extractor()
    assert torch.equal(pipe(**kw, ip_adapter_image=img1).images, other) and seen == ["pt"]
    pipe.feature_extractor = None
    # the captured loop: the embedding is the same static input as before
    pipe.capture_graphs = True
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    assert torch.equal(pipe(**kw, ip_adapter_image=img1).images, via_image)    # first sight: eager
    assert torch.equal(pipe(**kw, ip_adapter_image=img1).images, via_image)    # captured + replayed
    n_before = len(calls)
    assert torch.equal(pipe(**kw, ip_adapter_image=img1).images, via_image)    # replay only
    assert torch.equal(pipe(**kw, ip_adapter_image=img2).images, other)        # another image: new values of the same static input
    assert len(calls) == n_before
    pipe._denoise_eager = orig
    assert_no_call_state(pipe)
    # scale 0 short-circuits after the encoder; no adapter is still the embeds path's error
    pipe.set_ip_adapter_scale(0.0)
    assert torch.equal(pipe(**kw, ip_adapter_image=img1).images, base)
    pipe.unload_ip_adapter()
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(**kw, ip_adapter_image=img1)
    pipe.image_encoder = None
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        pipe(**kw, ip_adapter_image=img1)


def test_pipeline_image_prompt_with_two_images_per_prompt(gpu):
    """num_images_per_prompt = 2 from one prompt and one image: two latents, both moved by the image prompt."""
    from test_ip_adapter_gpu import SMALL_T

    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.text_encoders import CLIPTextModel, T5EncoderModel
    from reptext_amd.transformer import FluxTransformer2DModel

    from oracle import flux_oracle as orc

    class Tok:
        def __init__(self, vocab, length, eos):
            self.vocab, self.model_max_length, self.eos = vocab, length, eos

        def __call__(self, prompt, padding=None, max_length=None, truncation=None, return_tensors=None, **kw):
            n = max_length or self.model_max_length
            ids = torch.zeros(len(prompt), n, dtype=torch.long)
            for i, p in enumerate(prompt):
                toks = [(ord(ch) % (self.vocab - 2)) + 1 for ch in p][: n - 1]
                ids[i, : len(toks)] = torch.tensor(toks)
                ids[i, len(toks)] = self.eos
            return type("Enc", (), {"input_ids": ids})()

    t5 = T5EncoderModel(vocab_size=512, d_model=256, d_kv=64, d_ff=640, num_layers=1, num_heads=4, device=gpu, dtype=torch.bfloat16)
    clip = CLIPTextModel(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1, eos_token_id=999,
                         device=gpu, dtype=torch.bfloat16)
    g = torch.Generator(device=gpu).manual_seed(0)
    for m in (t5, clip):
        for p in m.parameters():
            p.data.copy_(0.05 * torch.randn(p.shape, device=gpu, generator=g))
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(orc.init_mmdit_params(SMALL_T, 411))
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, clip, Tok(1000, 77, 999), t5, Tok(512, 512, 1), tr, None)
    pipe.set_progress_bar_config(disable=True)
    pipe.capture_graphs = False
    pipe.load_ip_adapter(ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=E, seed=412))
    pipe.image_encoder = _tiny_encoder(gpu, 413)
    kw = dict(prompt="a sign", height=256, width=256, num_inference_steps=2, guidance_scale=3.5, max_sequence_length=64,
              num_images_per_prompt=2, output_type="latent")
    gen = lambda: torch.Generator(device="cpu").manual_seed(7)
    plain = pipe(**kw, generator=gen()).images
    out = pipe(**kw, generator=gen(), ip_adapter_image=_photo(3)).images
    assert out.shape == plain.shape and out.shape[0] == 2 and torch.isfinite(out.float()).all()
    assert not torch.equal(out[0], plain[0]) and not torch.equal(out[1], plain[1])
    assert torch.equal(out, pipe(**kw, generator=gen(), ip_adapter_image_embeds=pipe.encode_image(_photo(3), gpu)).images)
