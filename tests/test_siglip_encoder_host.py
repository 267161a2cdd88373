"""CPU tests of the SigLIP vision encoder path (reptext_amd.image_encoder.SiglipVisionModel): the host-side argument checks of
rt_attention_hd72, the constructor's refusals, state-dict compatibility with transformers' SiglipVisionModel (with and without the
``vision_model.`` prefix, from a full SiglipModel checkpoint, flat and nested config.json), the encoder-class dispatch, the host
preprocessing against transformers' SiglipImageProcessorPil, and the exactness of the plans' MLP padding. No kernel runs here."""
import json

import numpy as np
import pytest
import torch

TINY = dict(hidden_size=576, intermediate_size=592, num_hidden_layers=2, num_attention_heads=8, image_size=56, patch_size=14)


def test_attention_hd72_is_declared_bound_and_rejects_bad_arguments():
    import os

    from reptext_amd import native

    lib = native.load()
    assert lib.rt_abi_version() == native.ABI_VERSION == 15
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "reptext_hip.h")).read()
    assert "int rt_attention_hd72(" in header and f"#define RT_ATTENTION_HD72_MAX_S {native.RT_ATTENTION_HD72_MAX_S}" in header
    assert len(native.SIGNATURES["rt_attention_hd72"]) == 16
    P = 0x10000                                                                 # aligned, never dereferenced: every call is refused first
    MAX = native.RT_ATTENTION_HD72_MAX_S

    def attn(q=P, ldq=432, sqb=0, k=P, v=P, ldkv=432, skvb=0, o=P, ldo=144, sob=0, B=1, Sq=17, Sk=17, H=2, scale=0.125):
        return lib.rt_attention_hd72(q, ldq, sqb, k, v, ldkv, skvb, o, ldo, sob, B, Sq, Sk, H, scale, None)

    for name in ("q", "k", "v", "o"):
        assert attn(**{name: None}) == -1, name                                 # RT_E_BADARG: null pointer
    assert attn(Sq=0) == -1 and attn(Sk=0) == -1 and attn(B=0) == -1 and attn(H=0) == -1
    assert attn(scale=0.0) == -1 and attn(scale=-1.0) == -1 and attn(scale=float("nan")) == -1
    assert attn(ldq=136) == -1 and attn(ldkv=136) == -1 and attn(ldo=136) == -1  # a leading dimension < H*72 = 144
    assert attn(sqb=-8) == -1 and attn(skvb=-8) == -1 and attn(sob=-8) == -1
    assert attn(Sq=MAX + 1) == -3 and attn(Sk=MAX + 1) == -3                    # RT_E_SHAPE: over the documented bound
    assert attn(B=65536) == -3 and attn(H=65536, ldq=1 << 23, ldkv=1 << 23, ldo=1 << 23) == -3
    assert attn(ldq=436) == -2 and attn(ldkv=436) == -2 and attn(ldo=148) == -2  # RT_E_ALIGN: ld % 8
    assert attn(sqb=4) == -2 and attn(skvb=4) == -2 and attn(sob=12) == -2
    assert attn(q=P + 8) == -2 and attn(k=P + 2) == -2 and attn(v=P + 4) == -2 and attn(o=P + 8) == -2


def test_constructor_has_transformers_config_keys_and_refuses_what_is_not_built():
    from transformers import SiglipVisionConfig

    from reptext_amd.image_encoder import SiglipVisionModel

    keys = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_channels", "image_size", "patch_size",
            "hidden_act", "layer_norm_eps")
    hf = {k: v for k, v in SiglipVisionConfig(**TINY).to_dict().items() if k != "dtype"}
    m = SiglipVisionModel(**hf, device="cpu", dtype=torch.float32)             # the rest of transformers' dict is accepted
    for k in keys:
        assert m.config[k] == hf[k], k
    so = SiglipVisionModel.__init__.__defaults__
    assert SiglipVisionModel(num_hidden_layers=0, device="meta").config.hidden_size == 1152 and so[:3] == (1152, 4304, 27)   # so400m defaults
    with pytest.raises(ValueError, match="head dim must be 72"):
        SiglipVisionModel(**dict(TINY, num_attention_heads=9))                  # head dim 64
    with pytest.raises(ValueError, match="multiple of 64"):
        SiglipVisionModel(**dict(TINY, hidden_size=72, num_attention_heads=1))
    with pytest.raises(ValueError, match="vision_use_head"):
        SiglipVisionModel(**TINY, vision_use_head=False)
    with pytest.raises(ValueError, match="gelu_pytorch_tanh"):
        SiglipVisionModel(**TINY, hidden_act="gelu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 56, 56))
    mb = SiglipVisionModel(**TINY, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mb(torch.zeros(1, 3, 56, 56))
    for kw in (dict(output_attentions=True), dict(output_hidden_states=True), dict(interpolate_pos_encoding=True)):
        with pytest.raises(NotImplementedError):
            mb(torch.zeros(1, 3, 56, 56), **kw)


def _hf_state_dict(seed):
    from transformers import SiglipVisionConfig
    from transformers import SiglipVisionModel as HF

    torch.manual_seed(seed)
    return {k: v.contiguous() for k, v in HF(SiglipVisionConfig(**TINY)).state_dict().items()}


def test_state_dict_is_transformers_state_dict():
    from reptext_amd.image_encoder import SiglipVisionModel

    sd = _hf_state_dict(0)
    mine = SiglipVisionModel(**TINY, device="cpu", dtype=torch.float32)
    assert sorted(k for k in sd if not k.endswith("position_ids")) == sorted(mine.state_dict())
    mine.load_state_dict(sd, strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the published layout: `vision_model.` prefixed, inside a full SiglipModel checkpoint, with a stray position_ids buffer
    full = {"vision_model." + k: v for k, v in sd.items()}
    full.update({"text_model.x": torch.zeros(3), "logit_scale": torch.zeros(1), "logit_bias": torch.zeros(1),
                 "vision_model.embeddings.position_ids": torch.arange(16)[None]})
    other = SiglipVisionModel(**TINY, device="cpu", dtype=torch.float32)
    other.load_state_dict(full, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in sd.items() if "head.probe" not in k}, strict=True)


@pytest.mark.parametrize("nested", [False, True])
def test_from_pretrained_reads_flat_and_nested_configs(tmp_path, nested):
    from safetensors.torch import save_file

    from reptext_amd.image_encoder import SiglipVisionModel

    sd = _hf_state_dict(1)
    d = tmp_path / "snap" / "image_encoder"
    d.mkdir(parents=True)
    if nested:
        sd = {"vision_model." + k: v for k, v in sd.items()}
        sd.update({"text_model.x": torch.zeros(3), "logit_scale": torch.zeros(1), "logit_bias": torch.zeros(1)})
        cfg = {"model_type": "siglip", "vision_config": dict(TINY, model_type="siglip_vision_model"), "text_config": {"hidden_size": 8}}
    else:
        cfg = dict(TINY, model_type="siglip_vision_model", hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, dtype="float32")
    save_file(sd, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(cfg))
    m = SiglipVisionModel.from_pretrained(str(tmp_path / "snap"), subfolder="image_encoder")
    assert m.dtype == torch.bfloat16 and m.config.image_size == 56 and m.config.intermediate_size == 592
    key = ("vision_model." if nested else "") + "head.probe"
    assert torch.equal(m.head.probe.data, sd[key].to(torch.bfloat16))
    # and what it saves is found again as a SigLIP encoder
    from reptext_amd.image_encoder import image_encoder_class

    m.save_pretrained(str(tmp_path / "again"))
    assert image_encoder_class(str(tmp_path / "again")) is SiglipVisionModel
    again = SiglipVisionModel.from_pretrained(str(tmp_path / "again"))
    assert torch.equal(again.head.probe.data, m.head.probe.data)


def test_encoder_class_dispatch(tmp_path):
    from reptext_amd.image_encoder import CLIPVisionModelWithProjection, SiglipVisionModel, image_encoder_class

    cases = {"flat": ({"model_type": "siglip_vision_model", **TINY}, SiglipVisionModel),
             "nested": ({"model_type": "siglip", "vision_config": TINY}, SiglipVisionModel),
             "clip": ({"model_type": "clip_vision_model", "hidden_size": 128}, CLIPVisionModelWithProjection),
             "clip_nested": ({"model_type": "clip", "vision_config": {"hidden_size": 128}}, CLIPVisionModelWithProjection),
             "bare": ({"hidden_size": 128}, CLIPVisionModelWithProjection),
             "siglip_without_vision": ({"model_type": "siglip"}, CLIPVisionModelWithProjection)}
    for name, (cfg, want) in cases.items():
        d = tmp_path / name
        d.mkdir()
        (d / "config.json").write_text(json.dumps(cfg))
        assert image_encoder_class(str(d)) is want, name


def _image(w, h, mode, seed):
    from PIL import Image

    rng = np.random.default_rng(seed)
    ch = {"L": (), "RGB": (3,), "RGBA": (4,)}[mode]
    yy, xx = np.mgrid[0:h, 0:w]                                                 # smooth content + noise: a resize is exercised on both
    base = (127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0))[(...,) + (None,) * len(ch)]
    return Image.fromarray(np.clip(base + rng.integers(-60, 60, size=(h, w) + ch), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("w, h, mode, size", [(300, 517, "RGB", 384), (640, 480, "RGB", 384), (384, 384, "RGB", 384), (100, 90, "RGB", 56),
                                              (513, 1000, "RGB", 74), (200, 260, "L", 384), (260, 230, "RGBA", 64)])
def test_siglip_preprocess_matches_transformers(w, h, mode, size):
    """max |difference| <= 1e-6 against SiglipImageProcessorPil(size={"height": s, "width": s}): the bound of the clip_preprocess
    test (tests/test_image_encoder_host.py). The two can differ by expression order only; values lie in [-1, 1], where an fp32
    ulp is at most 6e-8. Measured: 1.2e-7 at every case (2 ulps at |x| near 1)."""
    from transformers import SiglipImageProcessorPil

    from reptext_amd.image_encoder import siglip_preprocess

    img = _image(w, h, mode, seed=w + h)
    ref = SiglipImageProcessorPil(size={"height": size, "width": size})(images=img, return_tensors="pt").pixel_values
    got = siglip_preprocess(img, size)
    assert got.shape == (1, 3, size, size) and got.dtype == torch.float32 and ref.shape == got.shape
    diff = float((got - ref.float()).abs().max())
    print(f"{w}x{h} {mode} -> {size}: max abs difference {diff:.3e}")
    assert diff <= 1e-6, diff
    arr = np.asarray(img)
    assert torch.equal(siglip_preprocess(arr, size), got)
    both = siglip_preprocess([img, arr], size)
    assert both.shape == (2, 3, size, size) and torch.equal(both[0], got[0]) and torch.equal(both[1], got[0])


def test_siglip_preprocess_refuses_other_inputs():
    from reptext_amd.image_encoder import siglip_preprocess

    with pytest.raises(TypeError, match="uint8"):
        siglip_preprocess(np.zeros((8, 8, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="PIL image"):
        siglip_preprocess("a path")
    with pytest.raises(ValueError, match="no image"):
        siglip_preprocess([])


def test_plan_padding_of_the_mlp_is_exact():
    """F = 592 -> 640. A padded hidden unit is gelu_tanh(0·x + 0) = 0 and meets a zero column of fc2, so the padded MLP is the
    unpadded one: in fp32 the two give the same bits (terms 0·0 appended to a sum do not change it)."""
    from reptext_amd.image_encoder import pad_mlp_to_64

    g = torch.Generator().manual_seed(3)
    d, F_ = 576, 592
    w1, b1, w2, b2 = torch.randn(F_, d, generator=g) / 24, torch.randn(F_, generator=g), torch.randn(d, F_, generator=g) / 24, torch.randn(d, generator=g)
    x = torch.randn(5, d, generator=g)
    w1p, b1p, w2p = pad_mlp_to_64(w1, b1, w2)
    assert w1p.shape == (640, d) and b1p.shape == (640,) and w2p.shape == (d, 640)
    assert torch.equal(w1p[:F_], w1) and torch.equal(b1p[:F_], b1) and torch.equal(w2p[:, :F_], w2)
    assert not w1p[F_:].any() and not b1p[F_:].any() and not w2p[:, F_:].any()
    act = lambda t: torch.nn.functional.gelu(t, approximate="tanh")

    def mlp(w1_, b1_, w2_):      # sums in index order and one activation call per hidden unit, so that only the terms matter (a
        # vectorised tanh may round an element differently in its SIMD body and in its scalar tail)
        hid = torch.stack([act((x * w1_[j]).cumsum(-1)[:, -1] + b1_[j]) for j in range(w1_.shape[0])], dim=1)
        return hid, torch.stack([(hid * w2_[i]).cumsum(-1)[:, -1] for i in range(w2_.shape[0])], dim=1) + b2

    hid, out = mlp(w1, b1, w2)
    hid_p, out_p = mlp(w1p, b1p, w2p)
    assert torch.equal(hid_p[:, :F_], hid) and not hid_p[:, F_:].any()
    assert torch.equal(out_p, out)
    # a width that needs no padding is passed through
    same = pad_mlp_to_64(w1[:576], b1[:576], w2[:, :576])
    assert same[0].shape == (576, d) and torch.equal(same[0], w1[:576]) and torch.equal(same[2], w2[:, :576])
