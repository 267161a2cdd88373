"""The rule the four encoders' plans follow (reptext_amd.encoder_common): a plan holds views of the parameters. Weights that one GEMM
reads as one operand are fused in place, so no weight is held twice, and a write into a parameter - through ``load_state_dict`` or not -
is seen by the next forward. One layer each, at the smallest configurations of the encoders' own GPU test files."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _t5(gpu):
    from reptext_amd.text_encoders import T5EncoderModel

    m = T5EncoderModel(vocab_size=512, d_model=256, d_kv=64, d_ff=640, num_layers=1, num_heads=4, device=gpu, dtype=BF)
    return m, torch.randint(0, 512, (2, 64), generator=torch.Generator().manual_seed(3)).to(gpu)


def _clip_text(gpu):
    from reptext_amd.text_encoders import CLIPTextModel

    m = CLIPTextModel(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                      max_position_embeddings=77, eos_token_id=999, device=gpu, dtype=BF)
    ids = torch.randint(1, 990, (2, 77), generator=torch.Generator().manual_seed(4))
    ids[0, 20], ids[1, 76] = 999, 999
    return m, ids.to(gpu)


def _clip_vision(gpu):
    from reptext_amd.image_encoder import CLIPVisionModelWithProjection

    m = CLIPVisionModelWithProjection(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=56, patch_size=14,
                                      projection_dim=64, device=gpu, dtype=BF)                      # 17 tokens, K 588 -> 640
    return m, torch.randn(2, 3, 56, 56, generator=torch.Generator().manual_seed(5)).to(gpu)


def _siglip(gpu):
    from reptext_amd.image_encoder import SiglipVisionModel

    m = SiglipVisionModel(hidden_size=576, intermediate_size=592, num_hidden_layers=1, num_attention_heads=8, image_size=56, patch_size=14,
                          device=gpu, dtype=BF)                                                     # 16 tokens, K 588 -> 640, F 592 -> 640
    return m, torch.randn(2, 3, 56, 56, generator=torch.Generator().manual_seed(6)).to(gpu)


MODELS = {"t5": _t5, "clip_text": _clip_text, "clip_vision": _clip_vision, "siglip": _siglip}


def _fill_(model, seed):
    """Every parameter overwritten in place through ``p.data.copy_`` (no ``load_state_dict``): norm weights 1 + 0.1·randn, the rest
    0.05·randn."""
    g = torch.Generator().manual_seed(seed)
    for n, p in model.named_parameters():
        v = torch.randn(p.shape, generator=g)
        p.data.copy_(1.0 + 0.1 * v if "norm" in n and n.endswith("weight") else 0.05 * v)
    return model


def _outputs(model, inp):
    outs = [o for o in model(inp) if o is not None]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
    return outs


def _fused_groups(name, m):
    """[(fused plan tensor, [the parameters that went into it, in row order])] after the first forward."""
    if name == "t5":
        qkv, _, wi, *_ = m._plans[0]
        sa, ff = m.encoder.block[0].layer[0].SelfAttention, m.encoder.block[0].layer[1].DenseReluDense
        return [(qkv, [sa.q.weight, sa.k.weight, sa.v.weight]), (wi, [ff.wi_1.weight, ff.wi_0.weight])]
    layer = {"clip_text": lambda: m.text_model.encoder.layers[0], "clip_vision": lambda: m.vision_model.encoder.layers[0],
             "siglip": lambda: m.encoder.layers[0]}[name]()
    wqkv, bqkv = m._plans["layers"][0][:2]
    sa = layer.self_attn
    return [(wqkv, [sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]), (bqkv, [sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias])]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_plan_weights_are_fused_in_place(gpu, name):
    m, inp = MODELS[name](gpu)
    _fill_(m, 11)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    _outputs(m, inp)
    for fused, parts in _fused_groups(name, m):
        assert fused.shape[0] == sum(p.shape[0] for p in parts)
        row = 0
        for p in parts:
            assert p.untyped_storage().data_ptr() == fused.untyped_storage().data_ptr()
            assert p.data_ptr() == fused.data_ptr() + row * fused.stride(0) * fused.element_size()
            row += p.shape[0]
    after = m.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k].shape == v.shape and torch.equal(after[k], v), k


@pytest.mark.parametrize("name", sorted(MODELS))
def test_no_plan_goes_stale_after_in_place_writes(gpu, name):
    m, inp = MODELS[name](gpu)
    first = _outputs(_fill_(m, 21), inp)
    second = _outputs(_fill_(m, 22), inp)                    # the plans of the first forward are still in place
    fresh = _outputs(_fill_(MODELS[name](gpu)[0], 22), inp)
    assert len(second) == len(fresh) and all(torch.equal(a, b) for a, b in zip(second, fresh))
    assert not any(torch.equal(a, b) for a, b in zip(first, second))
