"""CPU tests of the IP-Adapter path (reptext_amd.ip_adapter): the two key layouts, every refusal, token-count inference, the scale
setter, the host-side argument checks of rt_ip_attention, the untouched state_dict, and the tests' own fp32 restatement
(tests/ip_adapter_reference.py) against the oracle. No kernel runs here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402

from oracle import flux_oracle as orc  # noqa: E402

CFG = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
           joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
C, D, L = 64, 128, 2


def _parse(sd):
    from reptext_amd import ip_adapter

    return ip_adapter.parse_ip_adapter_state_dict(sd, L, C, D)


def test_both_layouts_parse_to_the_same_tensors(tmp_path):
    from safetensors.torch import save_file

    from reptext_amd import ip_adapter

    sd = ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=1)
    xl = ipr.to_xlabs(sd)
    assert sorted(xl) == sorted(ipr.init_ip_params(CFG, 4, 32, seed=1, layout="xlabs")) and not set(xl) & set(sd)
    a, b = _parse(sd), _parse(xl)
    assert a.num_tokens == b.num_tokens == 4
    for name in ("proj_w", "proj_b", "norm_w", "norm_b"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    for name in ("k_w", "k_b", "v_w", "v_b"):
        for i in range(L):
            assert torch.equal(getattr(a, name)[i], getattr(b, name)[i])
    assert torch.equal(a.k_w[1], sd["ip_adapter.1.to_k_ip.weight"]) and torch.equal(a.v_b[0], sd["ip_adapter.0.to_v_ip.bias"])
    # a file, a directory + weight_name, a directory + subfolder + the default name
    save_file(xl, str(tmp_path / "xl.safetensors"))
    (tmp_path / "sub").mkdir()
    save_file(sd, str(tmp_path / "sub" / ip_adapter.DEFAULT_WEIGHT_NAME))
    for got in (ip_adapter.read_ip_adapter_file(str(tmp_path / "xl.safetensors")),
                ip_adapter.read_ip_adapter_file(str(tmp_path), weight_name="xl.safetensors")):
        assert sorted(got) == sorted(xl)
    assert sorted(ip_adapter.read_ip_adapter_file(str(tmp_path), subfolder="sub")) == sorted(sd)
    # a directory that does not say which file: the error is the IP-Adapter reader's own, and names no LoRA file
    save_file(sd, str(tmp_path / "second.safetensors"))
    with pytest.raises(ValueError, match="weight_name") as ei:
        ip_adapter.read_ip_adapter_file(str(tmp_path))
    assert "lora" not in str(ei.value).lower()
    with pytest.raises(OSError, match="absent.safetensors"):
        ip_adapter.read_ip_adapter_file(str(tmp_path), weight_name="absent.safetensors")


@pytest.mark.parametrize("n", [1, 4, 16, 128])
def test_token_count_is_inferred(n):
    assert _parse(ipr.init_ip_params(CFG, n_tokens=n, embed_dim=32, seed=2)).num_tokens == n


def test_refusals_name_the_key():
    base = ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=3)

    def refused(change, key):
        sd = dict(base)
        change(sd)
        with pytest.raises(ValueError) as ei:
            _parse(sd)
        assert key in str(ei.value), (key, str(ei.value))

    refused(lambda sd: sd.update({"image_proj.extra.weight": torch.zeros(1)}), "image_proj.extra.weight")             # unknown key
    refused(lambda sd: sd.update({"ip_adapter.0.to_q_ip.weight": torch.zeros(1)}), "ip_adapter.0.to_q_ip.weight")
    refused(lambda sd: sd.update({f"ip_adapter.2.to_{kv}_ip.{p}": sd[f"ip_adapter.1.to_{kv}_ip.{p}"] for kv in "kv" for p in ("weight", "bias")}),
            "ip_adapter.2.to_k_ip.weight")                                                                               # 3 blocks for 2
    refused(lambda sd: [sd.pop(k) for k in list(sd) if k.startswith("ip_adapter.1.")], "ip_adapter.1.to_k_ip.weight")   # 1 block for 2
    refused(lambda sd: sd.update({"image_proj.norm.weight": torch.ones(C + 8), "image_proj.norm.bias": torch.zeros(C + 8)}), "image_proj.norm.weight")
    refused(lambda sd: sd.update({"ip_adapter.1.to_v_ip.weight": torch.zeros(D + 128, C)}), "ip_adapter.1.to_v_ip.weight")   # out-features != d
    refused(lambda sd: sd.update({"ip_adapter.0.to_k_ip.weight": torch.zeros(D, C + 8)}), "ip_adapter.0.to_k_ip.weight")
    refused(lambda sd: sd.update({"image_proj.proj.weight": torch.zeros(4 * C + 8, 32), "image_proj.proj.bias": torch.zeros(4 * C + 8)}),
            "image_proj.proj.weight")                                                                                    # non-integer token count
    refused(lambda sd: sd.update({"image_proj.proj.weight": torch.zeros(129 * C, 32), "image_proj.proj.bias": torch.zeros(129 * C)}),
            "image_proj.proj.weight")                                                                                    # > 128 tokens
    refused(lambda sd: sd.pop("ip_adapter.1.to_k_ip.bias"), "ip_adapter.1.to_k_ip.bias")                                # missing biases
    refused(lambda sd: sd.pop("image_proj.proj.bias"), "image_proj.proj.bias")
    refused(lambda sd: sd.pop("image_proj.norm.bias"), "image_proj.norm.bias")
    # single-block keys: the InstantX layout
    refused(lambda sd: sd.update({"ip_adapter.single_blocks.0.to_k_ip.weight": torch.zeros(1)}), "ip_adapter.single_blocks.0.to_k_ip.weight")
    xl = ipr.to_xlabs(base)
    xl["single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight"):
        _parse(xl)
    xl = ipr.to_xlabs(base)
    xl.pop("double_blocks.0.processor.ip_adapter_double_stream_v_proj.bias")
    with pytest.raises(ValueError, match="double_blocks.0.processor.ip_adapter_double_stream_v_proj.bias"):
        _parse(xl)
    with pytest.raises(ValueError, match="some.other.key"):
        _parse({"some.other.key": torch.zeros(1)})


def test_scales_and_embeds_normalisation():
    from reptext_amd import ip_adapter
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no IP-Adapter"):
        tr.set_ip_adapter_scale(0.5)
    tr.load_ip_adapter(ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=4))
    ad = tr._ip_adapter
    assert ad.scales == [1.0, 1.0] and ad.active and (ad.num_tokens, ad.E, ad.C, ad.d) == (4, 32, C, D)
    tr.set_ip_adapter_scale(0.25)
    assert ad.scales == [0.25, 0.25]
    tr.set_ip_adapter_scale([1.0, -0.7])
    assert ad.scales == [1.0, -0.7]
    with pytest.raises(ValueError, match="2 floats"):
        tr.set_ip_adapter_scale([1.0, 2.0, 3.0])
    assert ad.scales == [1.0, -0.7]
    tr.set_ip_adapter_scale(0)
    assert not ad.active
    e = torch.randn(3, 32)
    for given in (e, [e], e[:, None], [e[:, None]]):
        assert torch.equal(ip_adapter.normalize_embeds(given), e)
    assert ip_adapter.normalize_embeds(e[:1, None]).shape == (1, 32)
    with pytest.raises(ValueError, match="one IP-Adapter"):
        ip_adapter.normalize_embeds([e, e])
    with pytest.raises(ValueError, match="one image per sample"):
        ip_adapter.normalize_embeds(torch.randn(3, 2, 32))
    # the stacked K/V weight: block i's to_k_ip rows, then its to_v_ip rows
    sd = ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=4)
    assert torch.equal(ad.kv_w[2 * D:3 * D].float(), sd["ip_adapter.1.to_k_ip.weight"]) and torch.equal(ad.kv_w[3 * D:].float(), sd["ip_adapter.1.to_v_ip.weight"])
    assert torch.equal(ad.kv_b[D:2 * D].float(), sd["ip_adapter.0.to_v_ip.bias"])


def test_state_dict_is_untouched_by_the_adapter(tmp_path):
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=torch.bfloat16)
    tr.load_state_dict(orc.init_mmdit_params(CFG, seed=11))
    before = {k: v.clone() for k, v in tr.state_dict().items()}
    tr.load_ip_adapter(ipr.to_xlabs(ipr.init_ip_params(CFG, n_tokens=16, embed_dim=32, seed=5)))
    assert tr._ip_adapter.num_tokens == 16
    loaded = tr.state_dict()
    assert list(loaded) == list(before) and all(torch.equal(loaded[k], before[k]) for k in before)
    assert not any("ip" in n.split(".")[0] for n, _ in tr.named_parameters())
    tr.load_state_dict(before, strict=True)                                    # still a strict match while loaded
    version = tr._ip_adapter.version
    tr.to(torch.bfloat16)                                                       # _apply carries the adapter along
    assert tr._ip_adapter.version == version                                    # nothing moved: same tensors, same version
    tr.load_ip_adapter(ipr.init_ip_params(CFG, n_tokens=16, embed_dim=32, seed=5))
    assert tr._ip_adapter.version > version                                     # a new load is a new version (the graph key)
    tr.unload_ip_adapter()
    tr.unload_ip_adapter()                                                      # a second unload is harmless
    assert tr._ip_adapter is None and list(tr.state_dict()) == list(before)


def test_pipeline_arguments_without_a_device():
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=torch.bfloat16)
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None)
    kw = dict(prompt_embeds=torch.zeros(1, 8, C), pooled_prompt_embeds=torch.zeros(1, 32), height=64, width=64, num_inference_steps=1)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        pipe(**kw, ip_adapter_image=object())
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(**kw, ip_adapter_image_embeds=torch.zeros(1, 1, 32))
    pipe.load_ip_adapter(ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=6), image_encoder_pretrained_model_name_or_path="ignored")
    pipe.set_ip_adapter_scale([0.5, 0.0])
    assert tr._ip_adapter.scales == [0.5, 0.0]
    with pytest.raises(ValueError, match="width 48"):
        pipe(**kw, ip_adapter_image_embeds=torch.zeros(1, 1, 48))
    with pytest.raises(ValueError, match="batch 3"):
        pipe(**kw, ip_adapter_image_embeds=torch.zeros(3, 1, 32))
    pipe.unload_ip_adapter()
    assert tr._ip_adapter is None
    inp = InpaintPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None, None)
    for bad in (dict(ip_adapter_image=object()), dict(ip_adapter_image_embeds=torch.zeros(1, 1, 32)),
                dict(joint_attention_kwargs={"ip_adapter_image_embeds": torch.zeros(1, 1, 32)})):
        with pytest.raises(ValueError, match="IP-Adapter"):
            inp(**kw, **bad)


def test_entry_point_rejects_bad_arguments_without_a_device():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                                 # aligned, never dereferenced: every call is refused first

    def call(q=P, ldq=1536, sqb=0, wq=P, k=P, v=P, ldkv=512, skvb=0, o=P, ldo=512, sob=0, o_f32=0, acc=0, B=1, N=64, H=4, n_ip=4, sm=128 ** -0.5):
        return lib.rt_ip_attention(q, ldq, sqb, wq, k, v, ldkv, skvb, o, ldo, sob, o_f32, acc, B, N, H, n_ip, sm, 1.0, 1e-6, None)

    for name in ("q", "wq", "k", "v", "o"):
        assert call(**{name: None}) == -1, name                                 # RT_E_BADARG: null pointer
    assert call(n_ip=0) == -1                                                   # RT_E_BADARG: non-positive size
    assert call(N=0) == -1 and call(B=0) == -1 and call(H=0) == -1
    assert call(sm=0.0) == -1 and call(sm=-0.1) == -1 and call(sm=float("nan")) == -1   # the softmax is stabilised for a positive scale
    assert call(n_ip=129) == -3                                                 # RT_E_SHAPE
    assert call(ldq=1540) == -2                                                 # RT_E_ALIGN: ldq % 8
    assert call(ldkv=516) == -2 and call(ldo=516) == -2 and call(q=P + 8) == -2 and call(o=P + 2) == -2
    assert call(ldo=514, o_f32=1) == -2                                         # an fp32 o: ldo % 4
    assert call(ldq=256) == -1                                                  # ldq < H*128


def test_restatement_equals_the_oracle_when_nothing_is_added():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    p = orc.init_mmdit_params(CFG, seed=8)
    ipp = ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=9)
    N, T = 16, 8
    args = (r(1, N, 64), r(1, T, C), r(1, 32), torch.full((1,), 0.6), orc.latent_image_ids(8, 8), torch.zeros(T, 3))
    samples = [r(1, N, D)]
    kw = dict(guidance=torch.full((1,), 3.5), controlnet_block_samples=samples)
    ref = orc.transformer_forward(p, CFG, *args, **kw)
    assert torch.equal(ipr.transformer_forward(p, CFG, *args, **kw), ref)                                              # no adapter
    assert torch.equal(ipr.transformer_forward(p, CFG, *args, **kw, ip_params=ipp, ip_embeds=r(1, 32), ip_scales=[0.0, 0.0]), ref)
    with orc.stored_as(torch.bfloat16):
        assert torch.equal(ipr.transformer_forward(p, CFG, *args, **kw, ip_params=ipp, ip_embeds=r(1, 32), ip_scales=[0.0, 0.0]),
                           orc.transformer_forward(p, CFG, *args, **kw))
    moved = ipr.transformer_forward(p, CFG, *args, **kw, ip_params=ipp, ip_embeds=r(1, 32), ip_scales=[1.0, -0.7])
    assert float((moved - ref).norm() / ref.norm()) > 0.05                      # and with scales the term is really there
    # the loop
    sig = orc.flow_sigmas(2, 0.5)
    cfg_c = dict(CFG, num_single_layers=0, extra_condition_channels=64)
    cp = orc.init_mmdit_params(cfg_c, 10, controlnet=True)
    largs = (p, CFG, cp, cfg_c, args[0], args[1], args[2], [r(1, N, 128)], [torch.rand(1, N, 1, generator=g)], sig, args[4], args[5], 3.5)
    assert torch.equal(ipr.denoise_loop(*largs, ip_params=ipp, ip_embeds=r(1, 32), ip_scales=[0.0, 0.0]), orc.denoise_loop(*largs))
