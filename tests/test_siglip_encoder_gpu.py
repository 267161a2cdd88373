"""GPU tests of the SigLIP vision encoder path: rt_attention_hd72 against fp64 with the error of a CPU emulation of its roundings as
the yardstick, reptext_amd.image_encoder.SiglipVisionModel against the REAL transformers class with shared random weights, and
the pipeline's ``ip_adapter_image=`` with the InstantX adapter against ``ip_adapter_image_embeds=``."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantx_reference as ixr  # noqa: E402
import small_head_attention as sha  # noqa: E402
from instantx_reference import SMALL_T, rel_l2  # noqa: E402

# ------------------------------------------------------------------------------------------------------------------ the kernel
# (B, Sq, Sk, H, shared q). Self-attention: a single key, a partial key tile, an exact tile, a tile plus one, the real token count
# (729), five whole tiles, and the two smallest 16-head shapes at which the host picks 2 and 4 waves per workgroup, with a last
# workgroup whose waves past the first have no row. Rectangular: one query row over an exact tile and a tile plus one, a few rows
# over a partial tile, and the pooling call (one probe row shared by the batch: stride_qb = 0).
SELF_CASES = [(1, 1, 1, 1), (1, 17, 17, 2), (2, 64, 64, 1), (1, 65, 65, 3), (2, 729, 729, 2), (1, 320, 320, 1), (1, 513, 513, 16), (2, 513, 513, 16)]
RECT_CASES = [(1, 1, 64, 2), (1, 1, 65, 2), (3, 5, 17, 2)]
KERNEL_CASES = [c + (False,) for c in SELF_CASES + RECT_CASES] + [(2, 1, 729, 16, True)]


@pytest.mark.parametrize("B, Sq, Sk, H, shared", KERNEL_CASES)
def test_attention_hd72_vs_fp64_and_the_emulated_roundings(gpu, B, Sq, Sk, H, shared):
    """rel-L2 against fp64 from the same bf16 values, bounded by 1.5 x the error of a CPU emulation of the kernel's roundings on the
    same inputs (the margin rt_attention_hd64 is held to; the harness is tests/small_head_attention.py). With one key the output is v, bit for bit.
    Measured on an MI355X, kernel / emulation (B, Sq, Sk, H): (1,1,1,1) 0 / 0; (1,17,17,2) 2.052e-3 / 2.052e-3; (2,64,64,1) 2.123e-3 /
    2.122e-3; (1,65,65,3) 2.103e-3 / 2.100e-3; (2,729,729,2) 2.205e-3 / 2.245e-3; (1,320,320,1) 2.178e-3 / 2.215e-3; (1,513,513,16)
    2.200e-3 / 2.245e-3; (2,513,513,16) 2.180e-3 / 2.226e-3; (1,1,64,2) 1.779e-3 / 1.779e-3; (1,1,65,2) 2.490e-3 / 2.490e-3; (3,5,17,2)
    1.892e-3 / 1.892e-3; the pooling call (2,1,729,16) 2.178e-3 / 2.225e-3. Within one key tile the two agree to the last digit shown;
    over several tiles the kernel's running rescale orders the sums differently from the emulation's single pass."""
    buf, ref, emu, _ = sha.case(72, B, Sq, Sk, H, shared, 1.0)
    out = sha.fused(gpu, 72, buf, B, Sq, Sk, H, shared)
    err_k, err_e = rel_l2(out.float(), ref), rel_l2(emu.float(), ref)
    print(f"attention_hd72 B={B} Sq={Sq} Sk={Sk} H={H}: rel-L2 vs fp64 kernel {err_k:.3e}, emulation {err_e:.3e}")
    if Sk == 1:
        assert sha.is_v(out, buf, 72, B, Sq, H)
    assert err_k <= 1.5 * err_e, (err_k, err_e)


@pytest.mark.parametrize("B, S, H", [(1, 65, 3), (2, 257, 2)])
def test_attention_hd72_large_scores(gpu, B, S, H):
    """q scaled so that the largest scale·score exceeds 100: fp32 exp overflows at 88.7 unless the row maximum is subtracted.
    Same bound, finite outputs. Measured, kernel / emulation: (1,65,3) 8.284e-4 / 8.284e-4 at a largest scale·score of 203; (2,257,2)
    9.531e-4 / 9.593e-4 at 227."""
    buf, ref, emu, smax = sha.case(72, B, S, S, H, False, 48.0)
    assert smax > 100.0, smax
    err_k, err_e = rel_l2(sha.fused(gpu, 72, buf, B, S, S, H, False).float(), ref), rel_l2(emu.float(), ref)
    print(f"attention_hd72 large scores B={B} S={S} H={H} (max scale*score {smax:.0f}): rel-L2 vs fp64 kernel {err_k:.3e}, emulation {err_e:.3e}")
    assert err_k <= 1.5 * err_e, (err_k, err_e)


def test_attention_hd72_wrapper_refuses_what_the_kernel_cannot_take(gpu):
    from reptext_amd import native, ops

    buf = torch.zeros(2, 16, 432, device=gpu, dtype=torch.bfloat16)
    o = torch.zeros(2, 16, 144, device=gpu, dtype=torch.bfloat16)
    q, k, v = buf[..., :144], buf[..., 144:288], buf[..., 288:]
    with pytest.raises(ValueError, match="share shape and strides"):
        ops.attention_hd72(q, k, buf[:, :8, 288:], o, 2)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.attention_hd72(q, k, v, o[..., :128], 2)                             # not 72·H wide
    with pytest.raises(ValueError, match="q must be"):
        ops.attention_hd72(q[:, :8], k, v, o, 2)                                 # out rows != query rows
    with pytest.raises(ValueError, match="q must be"):
        ops.attention_hd72(torch.zeros(3, 16, 144, device=gpu, dtype=torch.bfloat16), k, v, o, 2)       # a batch that is neither 1 nor B
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_hd72(q.cpu(), k.cpu(), v.cpu(), o, 2)
    big = torch.zeros(1, native.RT_ATTENTION_HD72_MAX_S + 1, 216, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rows"):
        ops.attention_hd72(big[..., :72], big[..., 72:144], big[..., 144:], torch.zeros_like(big[..., :72]), 1)
    with pytest.raises(ValueError, match="rows"):
        ops.attention_hd72(big[:, :1, :72], big[..., 72:144], big[..., 144:], torch.zeros_like(big[:, :1, :72]), 1)   # too many keys
    torch.cuda.synchronize()
    assert not o.any()


# ------------------------------------------------------------------------------------------------------------------ the model
def _hf_siglip(cfg_kw, seed):
    """transformers' SiglipVisionModel in fp32 on the CPU, every weight rounded to bf16 and given an exercised range: LayerNorm weights
    1 + 0.1·randn, biases 0.1·randn, matrices at 1/sqrt(fan-in), the positions and the probe at unit scale (the default init leaves
    attention and MLP two orders below the stream, where no error of theirs would show)."""
    from transformers import SiglipVisionConfig
    from transformers import SiglipVisionModel as HF

    torch.manual_seed(seed)
    hf = HF(SiglipVisionConfig(**cfg_kw)).eval()
    bf = lambda t: t.to(torch.bfloat16).float()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(bf(1.0 + 0.1 * torch.randn_like(p)))
            elif n.endswith("bias"):
                p.copy_(bf(0.1 * torch.randn_like(p)))
            elif "position_embedding" in n or "probe" in n:
                p.copy_(bf(torch.randn_like(p)))
            else:
                p.copy_(bf(torch.randn_like(p) * (p[0].numel() ** -0.5)))
    return hf


SIG_TINY = dict(hidden_size=576, intermediate_size=592, num_hidden_layers=2, num_attention_heads=8, image_size=56, patch_size=14)
MODEL_CASES = {
    "a": (SIG_TINY, 1),                                                          # 16 tokens, K 588 -> 640, F 592 -> 640
    "b": (dict(SIG_TINY, image_size=74), 2),                                     # 74 = 5·14 + 4: 25 tokens from the top-left 70 x 70, batch 2
    "c": (dict(SIG_TINY, image_size=64, patch_size=16), 1),                      # K = 768: no padding
    "d": (dict(hidden_size=1152, intermediate_size=4304, num_hidden_layers=2, num_attention_heads=16, image_size=384, patch_size=14), 1),
}                                                                                # so400m width, the real S = 729 from 378 of 384 pixels


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_siglip_vision_model_vs_transformers(gpu, name):
    """pooler_output and last_hidden_state rel-L2 < 1e-2 against transformers in fp32: the project's bound for bf16 storage between
    stages against an fp32 run (tests/test_image_encoder_gpu.py). Measured (pooler_output / last_hidden_state): (a) 4.6e-3 / 2.6e-3,
    (b) 4.3e-3 / 2.5e-3, (c) 4.2e-3 / 2.6e-3, (d) 3.2e-3 / 2.2e-3."""
    from reptext_amd.image_encoder import SiglipVisionModel

    cfg_kw, B = MODEL_CASES[name]
    hf = _hf_siglip(cfg_kw, seed=ord(name))
    pix = torch.randn(B, 3, cfg_kw["image_size"], cfg_kw["image_size"], generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).float()
    with torch.no_grad():
        r = hf(pixel_values=pix)
    mine = SiglipVisionModel(**cfg_kw, layer_norm_eps=hf.config.layer_norm_eps, device=gpu, dtype=torch.bfloat16)
    mine.load_state_dict(hf.state_dict(), strict=True)
    o = mine(pix.to(gpu))
    S, d = (cfg_kw["image_size"] // cfg_kw["patch_size"]) ** 2, cfg_kw["hidden_size"]
    assert o.pooler_output.shape == (B, d) and o.pooler_output.dtype == torch.bfloat16
    assert o.last_hidden_state.shape == (B, S, d) and o.last_hidden_state.dtype == torch.bfloat16
    assert o[0] is o.last_hidden_state and o[1] is o.pooler_output
    e_p, e_h = rel_l2(o.pooler_output.float().cpu(), r.pooler_output), rel_l2(o.last_hidden_state.float().cpu(), r.last_hidden_state)
    print(f"SigLIP vision ({name}) B={B} S={S}: pooler_output {e_p:.3e}, last_hidden_state {e_h:.3e} vs transformers fp32")
    assert e_p < 1e-2 and e_h < 1e-2
    # bf16 pixel_values are the same values here (pix is bf16-representable): the same bits, and a second run too
    o16 = mine(pix.to(gpu, torch.bfloat16))
    assert torch.equal(o16.pooler_output, o.pooler_output) and torch.equal(o16.last_hidden_state, o.last_hidden_state)
    # the tuple form
    t = mine(pix.to(gpu), return_dict=False)
    assert isinstance(t, tuple) and torch.equal(t[1], o.pooler_output)


# ------------------------------------------------------------------------------------------------------------------ the pipeline
E_SIG = 576


def _tiny_siglip(gpu, seed):
    from reptext_amd.image_encoder import SiglipVisionModel

    return SiglipVisionModel(**SIG_TINY, device=gpu, dtype=torch.bfloat16).random_init_(seed)


def _photo(seed, w=90, h=70):
    from PIL import Image

    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))


def test_pipeline_image_prompt_with_the_instantx_adapter_is_the_embeds_path(gpu, tmp_path):
    from test_ip_adapter_gpu import _pipe, _pipe_inputs

    from reptext_amd.image_encoder import CLIPVisionModelWithProjection, SiglipVisionModel, siglip_preprocess

    pipe, _, _ = _pipe(gpu, 701)
    kw, _ = _pipe_inputs(gpu, 702, steps=2)
    ipp = ixr.init_instantx_params(SMALL_T, n_tokens=16, embed_dim=E_SIG, seed=703, v_std=ixr.MODEL_V_STD)
    # load_ip_adapter installs the encoder a directory with a siglip_vision_model config holds
    _tiny_siglip("cpu", 704).save_pretrained(str(tmp_path / "enc"))
    pipe.load_ip_adapter(ipp, image_encoder_pretrained_model_name_or_path=str(tmp_path), image_encoder_subfolder="enc")
    assert isinstance(pipe.image_encoder, SiglipVisionModel) and pipe.image_encoder.device.type == "cuda"
    pipe.set_ip_adapter_scale([1.0, -0.7, 0.9, -0.5])
    img1, img2 = _photo(1), _photo(2)
    pipe.capture_graphs = False
    base = pipe(**kw).images.clone()
    emb1 = pipe.encode_image(img1, gpu)
    assert emb1.shape == (1, E_SIG) and emb1.dtype == torch.bfloat16 and emb1.is_cuda
    assert torch.equal(emb1, pipe.image_encoder(siglip_preprocess(img1, 56).to(gpu)).pooler_output)
    assert pipe.encode_image(img1, gpu, num_images_per_prompt=3).shape == (3, E_SIG)
    via_embeds = pipe(**kw, ip_adapter_image_embeds=emb1).images.clone()
    via_image = pipe(**kw, ip_adapter_image=img1).images.clone()
    assert torch.equal(via_image, via_embeds) and not torch.equal(via_image, base)
    other = pipe(**kw, ip_adapter_image=[img2]).images.clone()
    assert not torch.equal(other, via_image)
    assert torch.equal(other, pipe(**kw, ip_adapter_image_embeds=pipe.encode_image(img2, gpu)).images)
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
    # with the CLIP encoder this adapter still gets the width error
    pipe.image_encoder = CLIPVisionModelWithProjection(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                                                       image_size=56, patch_size=14, projection_dim=64, device=gpu, dtype=torch.bfloat16).random_init_(705)
    with pytest.raises(ValueError, match=f"width 64 != the adapter's image embedding width {E_SIG}"):
        pipe(**kw, ip_adapter_image=img1)
