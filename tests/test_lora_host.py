"""CPU tests of the LoRA path (reptext_amd.lora): file and key formats, the three α sources, factor padding, every refusal, the
adapter state model, and the host-side argument checks of rt_lora_merge_bf16. No kernel runs here."""
import ctypes
import json

import pytest
import torch

SMALL_T = dict(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
               joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))


def _pair(out_f, in_f, r, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, in_f, generator=g), torch.randn(out_f, r, generator=g)


def _sd(prefix="transformer.", r=4, alpha=None):
    A, B = _pair(128, 128, r)
    A2, B2 = _pair(128 * 3, 128, r, seed=1)
    sd = {f"{prefix}transformer_blocks.0.attn.to_q.lora_A.weight": A, f"{prefix}transformer_blocks.0.attn.to_q.lora_B.weight": B,
          f"{prefix}single_transformer_blocks.0.norm.linear.lora_A.weight": A2,
          f"{prefix}single_transformer_blocks.0.norm.linear.lora_B.weight": B2}
    if alpha is not None:
        sd[f"{prefix}transformer_blocks.0.attn.to_q.alpha"] = torch.tensor(float(alpha))
    return sd


def test_keys_with_and_without_prefix_from_safetensors(tmp_path):
    from safetensors.torch import save_file

    from reptext_amd import lora

    for prefix in ("transformer.", ""):
        d = tmp_path / (prefix or "plain")
        d.mkdir()
        save_file(_sd(prefix), str(d / lora.DEFAULT_WEIGHT_NAME))
        sd, meta = lora.read_lora_file(str(d))
        parsed = lora.parse_lora_state_dict(sd, meta)
        assert sorted(parsed) == ["single_transformer_blocks.0.norm.linear", "transformer_blocks.0.attn.to_q"]
        A, B, sigma = parsed["transformer_blocks.0.attn.to_q"]
        assert A.shape == (4, 128) and B.shape == (128, 4) and sigma == 1.0
    other = tmp_path / "named"
    other.mkdir()
    save_file(_sd(), str(other / "my_lora.safetensors"))
    assert len(lora.read_lora_file(str(other))[0]) == 4                       # the only .safetensors of the directory
    assert len(lora.read_lora_file(str(other), weight_name="my_lora.safetensors")[0]) == 4
    assert len(lora.read_lora_file(str(other / "my_lora.safetensors"))[0]) == 4


def test_alpha_sources(tmp_path):
    from safetensors.torch import save_file

    from reptext_amd import lora

    p = lora.parse_lora_state_dict(_sd(r=4, alpha=8.0))                        # 1. per-module alpha
    assert p["transformer_blocks.0.attn.to_q"][2] == 2.0
    assert p["single_transformer_blocks.0.norm.linear"][2] == 1.0              # 3. no alpha anywhere
    f = tmp_path / "m.safetensors"
    save_file(_sd(r=4), str(f), metadata={"lora_adapter_metadata": json.dumps({"transformer.r": 4, "transformer.lora_alpha": 16})})
    sd, meta = lora.read_lora_file(str(f))
    p = lora.parse_lora_state_dict(sd, meta)                                   # 2. lora_alpha / r of the header metadata
    assert all(v[2] == 4.0 for v in p.values())
    p = lora.parse_lora_state_dict(_sd(r=4, alpha=2.0), {"r": 4, "lora_alpha": 16})
    assert p["transformer_blocks.0.attn.to_q"][2] == 0.5 and p["single_transformer_blocks.0.norm.linear"][2] == 4.0


def test_factor_padding_and_transpose():
    from reptext_amd import lora

    A, B = _pair(96, 40, 5)
    f = lora.pad_factors(A, B, 0.25, "cpu")
    assert f.B.shape == (96, 32) and f.At.shape == (40, 32) and f.B.dtype == torch.bfloat16 and f.r == 5 and f.sigma == 0.25
    assert torch.equal(f.B[:, :5], B.to(torch.bfloat16)) and torch.equal(f.At[:, :5], A.t().to(torch.bfloat16))
    assert not f.B[:, 5:].any() and not f.At[:, 5:].any()
    assert lora.pad_factors(*_pair(8, 8, 33), 1.0, "cpu").B.shape == (8, 64)


@pytest.mark.parametrize("key, msg", [
    ("lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight", "kohya/BFL"),
    ("transformer.transformer_blocks.0.attn.to_q.lora_up.weight", "kohya/BFL"),
    ("text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight", "text encoders"),
    ("text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_A.weight", "text encoders"),
    ("transformer.transformer_blocks.0.attn.to_q.lora_magnitude_vector", "DoRA"),
    ("transformer.transformer_blocks.0.attn.to_q.weird", "unrecognised"),
])
def test_format_refusals_name_the_key(key, msg):
    from reptext_amd import lora

    sd = dict(_sd(), **{key: torch.zeros(1)})
    with pytest.raises(ValueError, match=msg) as e:
        lora.parse_lora_state_dict(sd)
    assert key in str(e.value)


def test_metadata_and_model_refusals():
    from reptext_amd import lora
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.transformer import FluxTransformer2DModel

    for bad in ({"alpha_pattern": {"to_q": 4}}, {"transformer.rank_pattern": {"to_q": 2}}):
        with pytest.raises(ValueError, match="pattern"):
            lora.parse_lora_state_dict(_sd(), bad)
    tr = FluxTransformer2DModel(**SMALL_T, device="cpu", dtype=torch.bfloat16)
    A, B = _pair(128, 128, 4)
    with pytest.raises(ValueError, match="unknown module path.*transformer_blocks.7.attn.to_q"):
        tr.load_lora_adapter({"transformer_blocks.7.attn.to_q.lora_A.weight": A, "transformer_blocks.7.attn.to_q.lora_B.weight": B})
    with pytest.raises(ValueError, match="transformer_blocks.0.attn.to_q.*do not match"):
        tr.load_lora_adapter({"transformer_blocks.0.attn.to_q.lora_A.weight": A[:, :64], "transformer_blocks.0.attn.to_q.lora_B.weight": B})
    with pytest.raises(ValueError, match="GPU"):                       # a valid adapter on a CPU model: no CPU fallback
        tr.load_lora_adapter(_sd())
    assert getattr(tr, "_lora", None) is None and tr.active_adapters() == []
    cni = FluxControlNetModel(**dict(SMALL_T, num_single_layers=0, extra_condition_channels=4), device="cpu", dtype=torch.bfloat16)
    A68, B68 = _pair(128, 68, 4)
    with pytest.raises(ValueError, match="controlnet_x_embedder.*multiple of 8"):
        cni.load_lora_adapter({"controlnet_x_embedder.lora_A.weight": A68, "controlnet_x_embedder.lora_B.weight": B68})
    # 72 hint channels: a multiple of 8, but the tower caches a K-padded copy of that weight (_padded_hint), which a merge would leave stale
    cn72 = FluxControlNetModel(**dict(SMALL_T, num_single_layers=0, extra_condition_channels=8), device="cpu", dtype=torch.bfloat16)
    A72, B72 = _pair(128, 72, 4)
    with pytest.raises(ValueError, match="controlnet_x_embedder.*multiple of 64"):
        cn72.load_lora_adapter({"controlnet_x_embedder.lora_A.weight": A72, "controlnet_x_embedder.lora_B.weight": B72})


def _fake(sigma=1.0):
    from reptext_amd import lora

    return lora.Factor(torch.zeros(1), torch.zeros(1), 4, sigma)


def test_more_than_eight_terms_on_a_module_are_refused():
    from reptext_amd import lora

    st = lora.LoraState()
    for i in range(9):
        st.add(f"a{i}", {"x": _fake(), "y": _fake()})
    names = [f"a{i}" for i in range(8)]
    st.set_adapters(names)
    with pytest.raises(ValueError, match="more than 8 simultaneous LoRA terms on module.*x"):
        st.set_adapters(names + ["a8"])
    assert [a for a, _ in st.active] == names                        # the state is left as it was
    st.fuse(1.0, ["a0"])
    with pytest.raises(ValueError, match="more than 8"):
        st.fuse(1.0, ["a8"])


def test_state_model_sequence_and_order_independence():
    from reptext_amd import lora

    def fresh():
        st = lora.LoraState()
        st.add("a", {"m1": _fake(2.0), "m2": _fake(1.0)})
        assert st.active == [("a", 1.0)]
        st.add("b", {"m1": _fake(0.5)})
        assert st.active == [("b", 1.0)]                             # a newly loaded adapter is the only active one
        return st

    st = fresh()
    assert st.terms() == {"m1": [("b", 0.5)]}
    st.set_adapters(["a", "b"], [0.7, -0.3])
    assert st.terms() == {"m1": [("a", 0.7 * 2.0), ("b", -0.3 * 0.5)], "m2": [("a", 0.7)]}
    st.fuse(1.0, ["a"])
    assert st.fused == {"a": 0.7}
    with pytest.raises(ValueError, match="already fused"):
        st.fuse(1.0, ["a"])
    # call scale 0.5: the fused term keeps its coefficient, the unfused one is scaled
    assert st.terms(0.5) == {"m1": [("a", 0.7 * 2.0), ("b", 0.5 * -0.3 * 0.5)], "m2": [("a", 0.7)]}
    st.set_enabled(False)
    assert st.terms(0.5) == {"m1": [("a", 0.7 * 2.0)], "m2": [("a", 0.7)]}
    st.set_enabled(True)
    st.unfuse()
    assert st.terms() == {"m1": [("a", 0.7 * 2.0), ("b", -0.3 * 0.5)], "m2": [("a", 0.7)]}
    st.delete("b")
    assert st.active == [("a", 0.7)] and st.terms() == {"m1": [("a", 1.4)], "m2": [("a", 0.7)]}
    # the same state reached another way gives the same lists (terms are ordered by adapter name, zero terms dropped)
    other = fresh()
    other.set_adapters(["b", "a"], [-0.3, 0.7])
    other.fuse(2.0, ["b"])
    other.unfuse()
    assert other.terms() == fresh_terms(0.7, -0.3)
    other.delete(["b"])
    assert other.terms() == st.terms()
    z = fresh()
    z.set_adapters(["a", "b"], [0.0, 1.0])
    assert z.terms() == {"m1": [("b", 0.5)]}
    with pytest.raises(ValueError, match="unknown adapter"):
        z.set_adapters(["c"])


def fresh_terms(wa, wb):
    return {"m1": [("a", wa * 2.0), ("b", wb * 0.5)], "m2": [("a", wa * 1.0)]}


def test_merge_entry_rejects_null_pointers():
    """The null-pointer checks of rt_lora_merge_bf16 run on the host before anything else: no pointer here is a device address.
    (The shape, alignment and padding checks need real device buffers: test_lora_gpu.py.)"""
    from reptext_amd import native

    if not native.library_present():
        import __graft_entry__ as ge

        ge.build()
    lib = native.load()
    t = (native.LoraTerm * 1)(native.LoraTerm(None, None, 32, 32, 32, 1.0))
    assert lib.rt_lora_merge_bf16(t, 1, None, 64, None, 64, 64, 64, None) == -1          # RT_E_BADARG: W0 / W
    assert lib.rt_lora_merge_bf16(None, 1, None, 64, None, 64, 64, 64, None) == -1        # terms with nterms > 0
    assert lib.rt_lora_merge_bf16(None, 0, None, 64, None, 64, 0, 64, None) == -1
    assert lib.rt_lora_merge_bf16(t, 9, None, 64, None, 64, 64, 64, None) == -1
    assert ctypes.sizeof(native.LoraTerm) == 40
