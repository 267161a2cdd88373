"""CPU tests of the InstantX IP-Adapter layout (reptext_amd.ip_adapter): the three input forms, token-count inference, every refusal,
the scale setter, the untouched diffusers / XLabs parse, the host-side argument checks of the new entry points, and the tests' own
fp32 restatement (tests/instantx_reference.py) — including the conditions on the GPU tests' inputs that need no GPU. No kernel runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantx_reference as ixr  # noqa: E402
import ip_adapter_reference as ipr  # noqa: E402

from oracle import flux_oracle as orc  # noqa: E402

CFG = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
           joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
C, D, L2, L1, EMB = 64, 128, 2, 1, 64


def _parse(sd):
    from reptext_amd import ip_adapter

    return ip_adapter.parse_ip_adapter_state_dict(sd, L2, C, D, L1)


def test_three_input_forms_parse_to_the_same_tensors(tmp_path):
    from safetensors.torch import save_file

    from reptext_amd import ip_adapter

    sd = ixr.init_instantx_params(CFG, n_tokens=4, embed_dim=EMB, seed=1)
    a = _parse(sd)                                                              # fails on the parent commit: the layout was refused
    assert (a.layout, a.num_tokens, a.num_double, len(a.k_w), len(a.v_w)) == ("instantx", 4, L2, L2 + L1, L2 + L1) and not a.k_b and not a.v_b
    assert torch.equal(a.proj_w, sd["image_proj.proj.0.weight"]) and torch.equal(a.proj2_b, sd["image_proj.proj.2.bias"])
    assert torch.equal(a.k_w[2], sd["ip_adapter.2.to_k_ip.weight"]) and torch.equal(a.v_w[0], sd["ip_adapter.0.to_v_ip.weight"])
    save_file(sd, str(tmp_path / "flat.safetensors"))
    torch.save(ixr.to_nested(sd), str(tmp_path / "ip-adapter.bin"))
    forms = [ip_adapter.read_ip_adapter_file(str(tmp_path / "flat.safetensors")),
             ip_adapter.read_ip_adapter_file(str(tmp_path), weight_name="ip-adapter.bin"),
             ip_adapter.read_ip_adapter_file(str(tmp_path / "ip-adapter.bin")),
             ip_adapter.read_ip_adapter_file(ixr.to_nested(sd))]
    for got in forms:
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
        b = _parse(got)
        for name in ("proj_w", "proj_b", "proj2_w", "proj2_b", "norm_w", "norm_b"):
            assert torch.equal(getattr(a, name), getattr(b, name))
        assert all(torch.equal(x, y) for x, y in zip(a.k_w + a.v_w, b.k_w + b.v_w))
    with pytest.raises(OSError, match="absent.bin"):
        ip_adapter.read_ip_adapter_file(str(tmp_path), weight_name="absent.bin")
    # a pickle that is not plain tensors is not executed: weights_only=True refuses it
    import pickle

    with open(tmp_path / "evil.bin", "wb") as f:
        pickle.dump({"image_proj": {"x": os.getcwd}}, f)
    with pytest.raises(Exception):
        ip_adapter.read_ip_adapter_file(str(tmp_path / "evil.bin"))


@pytest.mark.parametrize("n", [1, 4, 128])
def test_token_count_is_inferred(n):
    assert _parse(ixr.init_instantx_params(CFG, n_tokens=n, embed_dim=EMB, seed=2)).num_tokens == n


def test_refusals_name_the_key():
    base = ixr.init_instantx_params(CFG, n_tokens=4, embed_dim=EMB, seed=3)

    def refused(change, key, also=None):
        sd = dict(base)
        change(sd)
        with pytest.raises(ValueError) as ei:
            _parse(sd)
        assert key in str(ei.value) and (also is None or also in str(ei.value)), (key, str(ei.value))

    z = torch.zeros
    refused(lambda sd: sd.update({"ip_adapter.3.to_k_ip.weight": z(D, C), "ip_adapter.3.to_v_ip.weight": z(D, C)}), "ip_adapter.3.to_k_ip.weight", "= 3 blocks")
    refused(lambda sd: [sd.pop(k) for k in list(sd) if k.startswith("ip_adapter.2.")], "ip_adapter.2.to_k_ip.weight")       # double blocks only
    refused(lambda sd: sd.pop("ip_adapter.1.to_v_ip.weight"), "ip_adapter.1.to_v_ip.weight")
    refused(lambda sd: sd.update({"ip_adapter.1.to_k_ip.bias": z(D)}), "ip_adapter.1.to_k_ip.bias", "no bias")
    refused(lambda sd: sd.update({"ip_adapter.0.to_v_ip.bias": z(D)}), "ip_adapter.0.to_v_ip.bias")
    refused(lambda sd: sd.update({"ip_adapter.2.to_v_ip.weight": z(D + 128, C)}), "ip_adapter.2.to_v_ip.weight")
    refused(lambda sd: sd.update({"ip_adapter.0.to_k_ip.weight": z(D, C + 8)}), "ip_adapter.0.to_k_ip.weight")
    refused(lambda sd: sd.update({"image_proj.norm.weight": torch.ones(C + 8), "image_proj.norm.bias": z(C + 8)}), "image_proj.norm.weight")
    refused(lambda sd: sd.update({"image_proj.proj.2.weight": z(4 * C + 8, 2 * EMB), "image_proj.proj.2.bias": z(4 * C + 8)}), "image_proj.proj.2.weight")
    refused(lambda sd: sd.update({"image_proj.proj.2.weight": z(129 * C, 2 * EMB), "image_proj.proj.2.bias": z(129 * C)}), "image_proj.proj.2.weight")
    refused(lambda sd: sd.update({"image_proj.proj.2.weight": z(0, 2 * EMB), "image_proj.proj.2.bias": z(0)}), "image_proj.proj.2.weight")   # n = 0
    refused(lambda sd: sd.update({"image_proj.proj.2.weight": z(4 * C, EMB)}), "image_proj.proj.2.weight")                 # in-features != 2E
    refused(lambda sd: sd.update({"image_proj.proj.2.bias": z(4 * C + 1)}), "image_proj.proj.2.bias")
    refused(lambda sd: sd.update({"image_proj.proj.0.weight": z(3 * EMB, EMB)}), "image_proj.proj.0.weight")               # not [2E, E]
    refused(lambda sd: sd.update({"image_proj.proj.0.bias": z(EMB)}), "image_proj.proj.0.bias")
    # the GEMM's K rule: E (and with it 2E) a multiple of 64
    refused(lambda sd: sd.update({"image_proj.proj.0.weight": z(80, 40), "image_proj.proj.0.bias": z(80), "image_proj.proj.2.weight": z(4 * C, 80)}),
            "image_proj.proj.0.weight", "K % 64")
    refused(lambda sd: sd.pop("image_proj.proj.2.weight"), "image_proj.proj.2.weight")
    refused(lambda sd: sd.pop("image_proj.norm.bias"), "image_proj.norm.bias")
    refused(lambda sd: sd.update({"image_proj.proj.1.weight": z(1)}), "image_proj.proj.1.weight")                           # unknown keys
    refused(lambda sd: sd.update({"ip_adapter.0.to_q_ip.weight": z(1)}), "ip_adapter.0.to_q_ip.weight")
    refused(lambda sd: sd.update({"single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight": z(1)}),
            "single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight")


def test_scales_take_a_float_or_one_per_block():
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=torch.bfloat16)
    tr.load_ip_adapter(ixr.init_instantx_params(CFG, n_tokens=4, embed_dim=EMB, seed=4))
    ad = tr._ip_adapter
    assert ad.scales == [1.0] * 3 and ad.active and (ad.layout, ad.num_tokens, ad.E, ad.C, ad.d, ad.num_double) == ("instantx", 4, EMB, C, D, L2)
    tr.set_ip_adapter_scale(0.7)
    assert ad.scales == [0.7] * 3
    tr.set_ip_adapter_scale([1.0, 0.0, -0.5])
    assert ad.scales == [1.0, 0.0, -0.5]
    for bad in ([1.0, 2.0], [1.0] * 4):
        with pytest.raises(ValueError, match="3 floats"):
            tr.set_ip_adapter_scale(bad)
    assert ad.scales == [1.0, 0.0, -0.5]
    tr.set_ip_adapter_scale(0)
    assert not ad.active
    sd = ixr.init_instantx_params(CFG, n_tokens=4, embed_dim=EMB, seed=4)
    assert torch.equal(ad.k_w[2 * D:].float(), sd["ip_adapter.2.to_k_ip.weight"]) and torch.equal(ad.v_w[D:2 * D].float(), sd["ip_adapter.1.to_v_ip.weight"])
    version = ad.version
    tr.to(torch.bfloat16)
    assert tr._ip_adapter.version == version
    before = list(tr.state_dict())
    tr.load_ip_adapter(sd)
    assert tr._ip_adapter.version > version and list(tr.state_dict()) == before
    # the other layouts keep their count and their message
    tr.load_ip_adapter(ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=4))
    with pytest.raises(ValueError, match=r"2 floats \(one per double block\)"):
        tr.set_ip_adapter_scale([1.0, 2.0, 3.0])


def test_diffusers_and_xlabs_parse_is_unchanged():
    from reptext_amd import ip_adapter

    sd = ipr.init_ip_params(CFG, n_tokens=4, embed_dim=32, seed=1)
    for given, layout in ((sd, "diffusers"), (ipr.to_xlabs(sd), "xlabs")):
        for w in (ip_adapter.parse_ip_adapter_state_dict(given, L2, C, D), _parse(given)):       # with and without the single-block count
            assert (w.layout, w.num_tokens, len(w.k_w), w.proj2_w) == (layout, 4, L2, None)
            assert torch.equal(w.proj_w, sd["image_proj.proj.weight"]) and torch.equal(w.k_b[1], sd["ip_adapter.1.to_k_ip.bias"])
    three = dict(sd)
    three.update({f"ip_adapter.2.to_{kv}_ip.{p}": sd[f"ip_adapter.1.to_{kv}_ip.{p}"] for kv in "kv" for p in ("weight", "bias")})
    with pytest.raises(ValueError, match="ip_adapter.2.to_k_ip.weight"):                        # L2 + L1 blocks in the diffusers layout: still refused
        _parse(three)


def test_new_entry_points_reject_bad_arguments_without_a_device():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                                 # aligned, never dereferenced: every call is refused first

    def call(q=P, ldq=3584, sqb=0, wq=P, k=P, v=P, ldkv=512, skvb=0, gate=P, sgb=3072, o=P, ldo=512, sob=0, o_f32=0, acc=0, B=1, N=64, H=4, n_ip=4, sm=128 ** -0.5):
        return lib.rt_ip_attention_gated(q, ldq, sqb, wq, k, v, ldkv, skvb, gate, sgb, o, ldo, sob, o_f32, acc, B, N, H, n_ip, sm, 1.0, 1e-6, None)

    for name in ("q", "wq", "k", "v", "o"):
        assert call(**{name: None}) == -1, name
    assert call(n_ip=0) == -1 and call(N=0) == -1 and call(B=0) == -1 and call(H=0) == -1 and call(sm=0.0) == -1
    assert call(sgb=-4) == -1 and call(ldq=256) == -1
    assert call(n_ip=129) == -3
    assert call(gate=P + 8) == -2 and call(sgb=3074) == -2 and call(ldq=3588) == -2 and call(ldo=514, o_f32=1) == -2
    add = lambda x=P, ldx=512, sxb=0, y=P, ldy=3584, syb=0, B=1, R=8, Dd=512: lib.rt_add_bf16_2d(x, ldx, sxb, y, ldy, syb, B, R, Dd, None)
    assert add(x=None) == -1 and add(y=None) == -1 and add(R=0) == -1 and add(ldx=256) == -1 and add(syb=-8) == -1
    assert add(Dd=12, ldx=16) == -3
    assert add(ldy=3588) == -2 and add(y=P + 2) == -2 and add(sxb=4) == -2
    assert lib.rt_gelu_erf_bf16(None, P, 8, None) == -1 and lib.rt_gelu_erf_bf16(P, P, 0, None) == -1


def test_restatement_equals_the_oracle_when_nothing_is_added():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    p = orc.init_mmdit_params(CFG, seed=8)
    ipp = ixr.init_instantx_params(CFG, n_tokens=4, embed_dim=EMB, seed=9)
    N, T = 16, 8
    args = (r(1, N, 64), r(1, T, C), r(1, 32), torch.full((1,), 0.6), orc.latent_image_ids(8, 8), torch.zeros(T, 3))
    kw = dict(guidance=torch.full((1,), 3.5), controlnet_block_samples=[r(1, N, D)])
    ref = orc.transformer_forward(p, CFG, *args, **kw)
    zero = dict(ip_params=ipp, ip_embeds=r(1, EMB), ip_scales=[0.0] * 3)
    assert torch.equal(ixr.transformer_forward(p, CFG, *args, **kw), ref)
    assert torch.equal(ixr.transformer_forward(p, CFG, *args, **kw, **zero), ref)
    with orc.stored_as(torch.bfloat16):
        assert torch.equal(ixr.transformer_forward(p, CFG, *args, **kw, **zero), orc.transformer_forward(p, CFG, *args, **kw))
    for scales in ([1.0, 0.0, 0.0], [0.0, 0.0, 1.0]):                           # a double block alone, a single block alone: each term is there
        moved = ixr.transformer_forward(p, CFG, *args, **kw, ip_params=ipp, ip_embeds=r(1, EMB), ip_scales=scales)
        assert ixr.rel_l2(moved, ref) > 1e-4, scales                           # fp32 noise is ~1e-6: the term is really there
    sig = orc.flow_sigmas(2, 0.5)
    cfg_c = dict(CFG, num_single_layers=0, extra_condition_channels=64)
    cp = orc.init_mmdit_params(cfg_c, 10, controlnet=True)
    largs = (p, CFG, cp, cfg_c, args[0], args[1], args[2], [r(1, N, 128)], [torch.rand(1, N, 1, generator=g)], sig, args[4], args[5], 3.5)
    assert torch.equal(ixr.denoise_loop(*largs, **zero), orc.denoise_loop(*largs))


@pytest.mark.parametrize("samples", [True, False])
def test_model_case_inputs_show_the_term_and_both_placement_rules(samples):
    """The conditions the GPU model test relies on, checked where no GPU is needed: at its shape and scales the adapter moves the
    output by >= 10 x the bf16 storage floor, and so does each of the two wrong placements (text rows of single blocks left out of
    the term; the double-block term added without gate_msa)."""
    _, _, _, targs, okw, ikw = ixr.model_case(samples=samples)
    ref = ixr.transformer_forward(*targs, **okw, **ikw)
    with orc.stored_as(torch.bfloat16):
        ref_s = ixr.transformer_forward(*targs, **okw, **ikw)
    floor = ixr.rel_l2(ref_s, ref)
    moved = ixr.rel_l2(ref, ixr.transformer_forward(*targs, **okw))
    no_text = ixr.rel_l2(ixr.transformer_forward(*targs, **okw, **ikw, variant="no_text_rows"), ref)
    ungated = ixr.rel_l2(ixr.transformer_forward(*targs, **okw, **ikw, variant="ungated"), ref)
    print(f"samples={samples}: floor {floor:.3e}, moved {moved:.3e}, no text rows {no_text:.3e}, ungated {ungated:.3e}")
    assert moved >= 10 * floor and no_text >= 10 * floor and ungated >= 10 * floor, (floor, moved, no_text, ungated)
