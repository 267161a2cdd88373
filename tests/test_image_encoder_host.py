"""CPU tests of the CLIP vision encoder path (reptext_amd.image_encoder): the host preprocessing against transformers'
CLIPImageProcessor, the host-side argument checks of rt_attention_hd64 / rt_patchify_nchw, state-dict compatibility with
transformers' CLIPVisionModelWithProjection, and the pipeline's rules for ip_adapter_image. No kernel runs here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402

TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14, projection_dim=32)


def _image(w, h, mode, seed):
    from PIL import Image

    rng = np.random.default_rng(seed)
    ch = {"L": (), "RGB": (3,), "RGBA": (4,)}[mode]
    # smooth content + noise: a resize is exercised on both
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0))[(...,) + (None,) * len(ch)]
    a = np.clip(base + rng.integers(-60, 60, size=(h, w) + ch), 0, 255).astype(np.uint8)
    return Image.fromarray(a)


# (width, height, mode): the five sizes at which the preprocessing was measured, plus a grayscale and an RGBA image
PREPROCESS_CASES = [(300, 517, "RGB"), (640, 480, "RGB"), (224, 224, "RGB"), (100, 90, "RGB"), (513, 1000, "RGB"), (200, 260, "L"), (260, 230, "RGBA")]


@pytest.mark.parametrize("w, h, mode", PREPROCESS_CASES)
def test_clip_preprocess_matches_transformers(w, h, mode):
    """max |difference| <= 1e-6 against CLIPImageProcessor() (its PIL backend): the two differ by expression order only, 2 fp32
    ulps at |x| < 4 (4.8e-7 measured)."""
    from transformers import CLIPImageProcessor

    from reptext_amd.image_encoder import clip_preprocess

    img = _image(w, h, mode, seed=w + h)
    ref = CLIPImageProcessor()(images=img, return_tensors="pt").pixel_values
    got = clip_preprocess(img)
    assert got.shape == (1, 3, 224, 224) and got.dtype == torch.float32 and ref.shape == got.shape
    diff = float((got - ref.float()).abs().max())
    print(f"{w}x{h} {mode}: max abs difference {diff:.3e}")
    assert diff <= 1e-6, diff
    # a uint8 array and a list are the other two accepted forms
    arr = np.asarray(img)
    assert torch.equal(clip_preprocess(arr), got)
    both = clip_preprocess([img, arr])
    assert both.shape == (2, 3, 224, 224) and torch.equal(both[0], got[0]) and torch.equal(both[1], got[0])


def test_clip_preprocess_refuses_other_inputs():
    from reptext_amd.image_encoder import clip_preprocess

    with pytest.raises(TypeError, match="uint8"):
        clip_preprocess(np.zeros((8, 8, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="PIL image"):
        clip_preprocess("a path")
    with pytest.raises(ValueError, match="no image"):
        clip_preprocess([])


def test_entry_points_reject_bad_arguments_without_gpu_memory():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                                 # aligned, never dereferenced: every call is refused first

    def attn(q=P, k=P, v=P, ld=384, sb=0, o=P, ldo=128, sob=0, B=1, S=17, H=2, scale=0.125):
        return lib.rt_attention_hd64(q, k, v, ld, sb, o, ldo, sob, B, S, H, scale, None)

    for name in ("q", "k", "v", "o"):
        assert attn(**{name: None}) == -1, name                                 # RT_E_BADARG: null pointer
    assert attn(S=0) == -1 and attn(B=0) == -1 and attn(H=0) == -1              # RT_E_BADARG: non-positive size
    assert attn(scale=0.0) == -1 and attn(scale=-1.0) == -1 and attn(scale=float("nan")) == -1
    assert attn(ld=120) == -1 and attn(ldo=64) == -1                            # a leading dimension < H*64
    assert attn(S=native.RT_ATTENTION_HD64_MAX_S + 1) == -3                     # RT_E_SHAPE: over the documented bound
    assert attn(B=65536) == -3
    assert attn(ld=388) == -2 and attn(ldo=132) == -2 and attn(sb=4) == -2 and attn(sob=12) == -2      # RT_E_ALIGN: strides % 8
    assert attn(q=P + 8) == -2 and attn(k=P + 2) == -2 and attn(v=P + 4) == -2 and attn(o=P + 8) == -2

    def patch(x=P, x_f32=1, out=P, B=1, G=4, p=14, Kp=640):
        return lib.rt_patchify_nchw(x, x_f32, out, B, G, p, Kp, None)

    assert patch(x=None) == -1 and patch(out=None) == -1
    assert patch(B=0) == -1 and patch(G=0) == -1 and patch(p=0) == -1
    assert patch(Kp=576) == -1                                                  # Kp < 3*p*p = 588
    assert patch(Kp=600) == -2                                                  # the GEMM's K % 64
    assert patch(out=P + 8) == -2 and patch(x=P + 2) == -2 and patch(x=P + 1, x_f32=0) == -2
    assert patch(G=4097) == -3 and patch(p=1025, Kp=3 * 1025 * 1025 + 61) == -3 and patch(B=1 << 20, G=64) == -3


def test_state_dict_is_transformers_state_dict():
    from transformers import CLIPVisionConfig
    from transformers import CLIPVisionModelWithProjection as HF

    from reptext_amd.image_encoder import CLIPVisionModelWithProjection

    torch.manual_seed(0)
    hf = HF(CLIPVisionConfig(**TINY))
    sd = hf.state_dict()
    mine = CLIPVisionModelWithProjection(**TINY, device="cpu", dtype=torch.float32)
    assert sorted(k for k in sd if not k.endswith("position_ids")) == sorted(mine.state_dict())
    mine.load_state_dict(sd, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the encoder's own layout (CLIPVisionModel: no `vision_model.` prefix), with a stray position_ids buffer
    bare = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in sd.items()}
    bare["embeddings.position_ids"] = torch.arange(17)[None]
    other = CLIPVisionModelWithProjection(**TINY, device="cpu", dtype=torch.float32)
    other.load_state_dict(bare, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in sd.items() if "post_layernorm" not in k}, strict=True)
    # what is not built is refused, by name
    with pytest.raises(ValueError, match="head dim must be 64"):
        CLIPVisionModelWithProjection(**dict(TINY, num_attention_heads=4))      # head dim 32
    with pytest.raises(ValueError, match="quick_gelu"):
        CLIPVisionModelWithProjection(**dict(TINY, hidden_act="gelu"))
    with pytest.raises(ValueError, match="multiple of patch_size"):
        CLIPVisionModelWithProjection(**dict(TINY, image_size=60))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mine(torch.zeros(1, 3, 56, 56))


def test_from_pretrained_reads_a_local_directory(tmp_path):
    import json

    from safetensors.torch import save_file
    from transformers import CLIPVisionConfig
    from transformers import CLIPVisionModelWithProjection as HF

    from reptext_amd.image_encoder import CLIPVisionModelWithProjection

    torch.manual_seed(1)
    sd = {k: v.contiguous() for k, v in HF(CLIPVisionConfig(**TINY)).state_dict().items()}
    d = tmp_path / "snap" / "image_encoder"
    d.mkdir(parents=True)
    save_file(sd, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps({"model_type": "clip", "vision_config": dict(TINY, hidden_act="quick_gelu")}))     # nested form
    m = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "snap"), subfolder="image_encoder")
    assert m.dtype == torch.bfloat16 and m.config.image_size == 56
    assert torch.equal(m.visual_projection.weight.data, sd["visual_projection.weight"].to(torch.bfloat16))


def test_pipeline_rules_without_a_device(tmp_path):
    from PIL import Image

    from reptext_amd.image_encoder import CLIPVisionModelWithProjection
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    cfg = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
               joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
    tr = FluxTransformer2DModel(**cfg, device="cpu", dtype=torch.bfloat16)
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None)
    assert pipe.image_encoder is None and pipe.feature_extractor is None
    assert "image_encoder" not in pipe.components and "feature_extractor" not in pipe.components
    kw = dict(prompt_embeds=torch.zeros(1, 8, 64), pooled_prompt_embeds=torch.zeros(1, 32), height=64, width=64, num_inference_steps=1)
    img = Image.new("RGB", (60, 70))
    pipe.load_ip_adapter(ipr.init_ip_params(cfg, n_tokens=4, embed_dim=32, seed=6), image_encoder_pretrained_model_name_or_path="does-not-exist")
    assert pipe.image_encoder is None                                           # nothing resolved, nothing raised, nothing fetched
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        pipe(**kw, ip_adapter_image=img)
    with pytest.raises(ValueError, match="not both"):                          # checked before the encoder is asked for
        pipe(**kw, ip_adapter_image=img, ip_adapter_image_embeds=torch.zeros(1, 1, 32))
    pipe.image_encoder = CLIPVisionModelWithProjection(**TINY, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="not both"):
        pipe(**kw, ip_adapter_image=img, ip_adapter_image_embeds=torch.zeros(1, 1, 32))
    with pytest.raises(ValueError, match="not both"):
        pipe(**kw, ip_adapter_image=img, joint_attention_kwargs={"ip_adapter_image_embeds": torch.zeros(1, 1, 32)})
    with pytest.raises(ValueError, match="3 images for a batch of 1"):
        pipe(**kw, ip_adapter_image=[img, img, img])
    with pytest.raises(ValueError, match="3 images for a batch of 1"):
        pipe(**kw, ip_adapter_image=torch.zeros(3, 3, 56, 56))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # a valid request reaches the encoder, which has no CPU path
        pipe(**kw, ip_adapter_image=img)
    assert_no_call_state(pipe)
    # a directory that holds an encoder is loaded by load_ip_adapter
    pipe.image_encoder.save_pretrained(str(tmp_path / "enc"))
    pipe.image_encoder = None
    pipe.load_ip_adapter(ipr.init_ip_params(cfg, n_tokens=4, embed_dim=32, seed=6), image_encoder_pretrained_model_name_or_path=str(tmp_path),
                         image_encoder_subfolder="enc")
    assert isinstance(pipe.image_encoder, CLIPVisionModelWithProjection) and pipe.image_encoder.config.projection_dim == 32
    assert pipe.to("cpu") is pipe
