"""GPU tests of the InstantX IP-Adapter form: rt_ip_attention_gated against fp32 math from the same bf16 inputs, the per-call set-up,
the transformer (every precision mode) and the pipeline against the tests' fp32 restatement (tests/instantx_reference.py), and the
pipeline contract (graph replay bitwise the eager result, scales part of the graph key, embeds a static input, all scales 0 bitwise
the no-adapter image, an XLabs adapter still on run_double's unchanged branch)."""
import contextlib
import itertools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantx_reference as ixr  # noqa: E402
import ip_adapter_reference as ipr  # noqa: E402
from instantx_reference import E, SMALL_CN, SMALL_T, rel_l2  # noqa: E402

from oracle import flux_oracle as orc  # noqa: E402

KERNEL_BOUND = 5e-3            # the bound test_ip_attention_kernel_matches_fp32 holds rt_ip_attention to


def assert_at_dtype_floor(err_fp32, err_stored, floor):
    """Restated from test_models_gpu.py: GPU vs fp32 oracle, GPU vs storage-precision oracle, that oracle vs the fp32 one."""
    assert err_fp32 <= 1.25 * floor + 1e-4, (err_fp32, floor)
    assert err_stored <= 1.45 * floor + 1e-4, (err_stored, floor)


# ------------------------------------------------------------------------------------------------------------------ the kernel
H_K, B_K = 2, 2
D_K = H_K * 128


@pytest.mark.parametrize("n_ip, rows, shared, gated, f32_acc", list(itertools.product((4, 128), (100, 64 + 257), (True, False), (True, False), (True, False))))
def test_gated_kernel_matches_fp32(gpu, n_ip, rows, shared, gated, f32_acc):
    """n_ip = 4 pads the keys to 32, n_ip = 128 takes the 256-row workgroup; 100 and 321 rows are no multiple of 16 nor of a
    workgroup's rows (321: three workgroups of 128, two of 256). The query sits where a single block has it: columns 2d.. of a
    [B, rows, 7d] buffer. The gate is the third d-wide chunk of a [B, 6d] fp32 table (batch stride 6d), as the adaLN table is."""
    from reptext_amd import ops

    g = torch.Generator().manual_seed(1000 * n_ip + rows + 2 * shared + gated)
    bf = lambda t: t.to(torch.bfloat16)
    d = D_K
    q = bf(torch.randn(B_K, rows, H_K, 128, generator=g) * 10.0 ** (torch.rand(B_K, rows, 1, 1, generator=g) * 2.0 - 1.0))
    wq = bf(torch.rand(128, generator=g) + 0.5)
    Bk = 1 if shared else B_K
    k = torch.randn(Bk, n_ip, H_K, 128, generator=g) * 1.5
    k = bf(k * torch.rsqrt(k.pow(2).mean(-1, keepdim=True) + 1e-5) * 1.5)       # as the set-up leaves it: normalised (x 1.5: sharper logits)
    v = bf(torch.randn(Bk, n_ip, H_K, 128, generator=g))
    table = torch.randn(B_K, 6 * d, generator=g)
    gate = table[:, 2 * d : 3 * d]
    ip_scale = -1.3 if rows % 2 else 0.7
    ref = ixr.ip_attention_gated_ref(q, wq, k, v, ip_scale, gate if gated else None)

    qbuf = bf(torch.randn(B_K, rows, 7 * d, generator=g))
    qbuf[..., 2 * d : 3 * d] = q.reshape(B_K, rows, d)
    qdev = qbuf.to(gpu)
    q_before = qdev.clone()
    ldo, rows_o = d + 16, rows + 3
    obuf = (torch.randn(B_K, rows_o, ldo, generator=g) * 0.5).to(torch.float32 if f32_acc else torch.bfloat16)   # non-zero contents, canaries
    odev = obuf.to(gpu)
    old = obuf[:, :rows, :d].float() if f32_acc else 0.0
    want = ref + old
    if gated:
        # a condition on the inputs: a gate that is ignored, or read with the wrong batch stride, is >= 10 x the bound away
        ungated = rel_l2(ixr.ip_attention_gated_ref(q, wq, k, v, ip_scale, None) + old, want)
        swapped = rel_l2(ixr.ip_attention_gated_ref(q, wq, k, v, ip_scale, gate.flip(0)) + old, want)
        print(f"wrong-answer distances: ungated {ungated:.3f}, other batch entry's gate {swapped:.3f}")
        assert ungated >= 10 * KERNEL_BOUND and swapped >= 10 * KERNEL_BOUND, (ungated, swapped)
    tdev = table.to(gpu)
    ops.ip_attention_gated(qdev[..., 2 * d : 3 * d], wq.to(gpu), k.reshape(Bk, n_ip, d).to(gpu), v.reshape(Bk, n_ip, d).to(gpu), odev[:, :rows, :d], H_K,
                           ip_scale=ip_scale, gate=tdev[:, 2 * d : 3 * d] if gated else None, accumulate=f32_acc)
    torch.cuda.synchronize()
    out = odev.cpu()
    err = rel_l2(out[:, :rows, :d].float(), want)
    print(f"n_ip={n_ip} rows={rows} shared={shared} gated={gated} f32 accumulate={f32_acc}: rel_l2 {err:.3e}")
    assert err < KERNEL_BOUND, err
    assert torch.equal(qdev, q_before)
    assert torch.equal(out[:, rows:], obuf[:, rows:]) and torch.equal(out[:, :, d:], obuf[:, :, d:])


def test_ungated_call_is_rt_ip_attention_bit_for_bit(gpu):
    from reptext_amd import ops

    g = torch.Generator().manual_seed(5)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(gpu)
    q, wq, k, v = bf(2, 100, D_K), bf(128), bf(2, 17, D_K), bf(2, 17, D_K)
    a, b = torch.zeros(2, 100, D_K, device=gpu), torch.zeros(2, 100, D_K, device=gpu)
    ops.ip_attention(q, wq, k, v, a, H_K, ip_scale=0.7)
    ops.ip_attention_gated(q, wq, k, v, b, H_K, ip_scale=0.7)
    assert torch.equal(a, b) and a.abs().sum() > 0


def test_new_entry_points_reject_bad_arguments_on_real_buffers(gpu):
    from reptext_amd import native, ops

    lib = native.load()
    d = D_K
    q = torch.zeros(1, 64, 7 * d, device=gpu, dtype=torch.bfloat16)
    wq = torch.ones(128, device=gpu, dtype=torch.bfloat16)
    o = torch.zeros(1, 64, d, device=gpu, dtype=torch.bfloat16)
    kv = lambda n, b=1: torch.ones(b, n, d, device=gpu, dtype=torch.bfloat16)
    gate = torch.ones(1, 6 * d, device=gpu)
    qv = q[..., 2 * d : 3 * d]
    with pytest.raises(ValueError, match="1..128"):
        ops.ip_attention_gated(qv, wq, kv(129), kv(129), o, H_K)
    with pytest.raises(ValueError, match="gate must be"):
        ops.ip_attention_gated(qv, wq, kv(4), kv(4), o, H_K, gate=gate)                      # the whole table, not its d-wide chunk
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ip_attention_gated(qv, wq, kv(4), kv(4), o, H_K, gate=gate[:, :d].cpu())
    K = kv(4)

    def call(gate_ptr=gate.data_ptr(), sgb=6 * d, n_ip=4, ldq=7 * d, N=64):
        return lib.rt_ip_attention_gated(qv.data_ptr(), ldq, 0, wq.data_ptr(), K.data_ptr(), K.data_ptr(), d, 0, gate_ptr, sgb, o.data_ptr(), d, 0, 0, 0,
                                         1, N, H_K, n_ip, 128 ** -0.5, 1.0, 1e-6, None)

    assert call(n_ip=0) == -1 and call(N=0) == -1 and call(sgb=-4) == -1 and call(ldq=128) == -1       # RT_E_BADARG
    assert call(n_ip=129) == -3                                                                        # RT_E_SHAPE
    assert call(gate_ptr=gate.data_ptr() + 4) == -2 and call(sgb=6 * d + 2) == -2 and call(ldq=7 * d + 4) == -2    # RT_E_ALIGN
    y = torch.zeros(1, 8, 7 * d, device=gpu, dtype=torch.bfloat16)
    x = torch.ones(1, 8, d, device=gpu, dtype=torch.bfloat16)
    assert lib.rt_add_bf16_2d(x.data_ptr(), d, 0, y.data_ptr(), 7 * d + 4, 0, 1, 8, d, None) == -2
    assert lib.rt_add_bf16_2d(x.data_ptr(), d, 0, y.data_ptr(), 7 * d, 0, 1, 0, d, None) == -1
    assert lib.rt_add_bf16_2d(x.data_ptr(), d, 0, y.data_ptr(), 7 * d, 0, 1, 8, 12, None) == -3
    torch.cuda.synchronize()
    assert not o.any() and not y.any()                                                                 # nothing was launched


def test_strided_add_and_exact_gelu(gpu):
    """The two small kernels: exact in their own arithmetic (one bf16 rounding of an fp32 sum / of the fp32 erf form)."""
    from reptext_amd import ops

    g = torch.Generator().manual_seed(6)
    d = D_K
    y = torch.randn(2, 37, 7 * d, generator=g).to(torch.bfloat16)
    x = torch.randn(2, 37, d, generator=g).to(torch.bfloat16)
    ydev = y.to(gpu)
    ops.add_bf16_(ydev[..., 2 * d : 3 * d], x.to(gpu))
    want = y.clone()
    want[..., 2 * d : 3 * d] = (y[..., 2 * d : 3 * d].float() + x.float()).to(torch.bfloat16)
    assert torch.equal(ydev.cpu(), want)                                                               # the other columns untouched
    h = torch.randn(3, 130, generator=g) * 3.0
    got = ops.gelu_erf(h.to(gpu)).float().cpu()
    ref = ixr.gelu_erf(h.double()).float()
    assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all())                             # one bf16 rounding: 2^-9 relative, + erff


# ------------------------------------------------------------------------------------------------------------------ the set-up
@pytest.mark.parametrize("n_tokens", [4, 128])
def test_setup_tokens_and_normalised_kv(gpu, n_tokens):
    from reptext_amd import ip_adapter

    ipp = ixr.init_instantx_params(SMALL_T, n_tokens=n_tokens, embed_dim=E, seed=500 + n_tokens)
    C, d, Hh = SMALL_T["joint_attention_dim"], 512, 4
    L = SMALL_T["num_layers"] + SMALL_T["num_single_layers"]
    w = ip_adapter.parse_ip_adapter_state_dict(ipp, SMALL_T["num_layers"], C, d, SMALL_T["num_single_layers"])
    ad = ip_adapter.IPAdapter(w, gpu)
    emb = torch.randn(2, E, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).float()
    prep = ad.prepare(emb.to(gpu, torch.bfloat16))
    torch.cuda.synchronize()
    assert prep.inside and prep.num_double == 2 and len(prep.kv) == L and prep.kv[0][0].shape == (2, n_tokens, d)

    def ref():
        tok = ixr.ix_tokens(ipp, emb, C)
        kv = [ixr.ix_kv(ipp, tok, j, Hh, 128) for j in range(L)]
        return tok, torch.stack([k for k, _ in kv]).flatten(-2), torch.stack([v for _, v in kv]).flatten(-2)

    r32 = ref()
    with orc.stored_as(torch.bfloat16):
        r16 = ref()
    got = (prep.tok.float().cpu(), torch.stack([k for k, _ in prep.kv]).float().cpu(), torch.stack([v for _, v in prep.kv]).float().cpu())
    for name, o, a, b in zip(("tokens", "K", "V"), got, r32, r16):
        floor, err, err_s = rel_l2(b, a), rel_l2(o, a), rel_l2(o, b)
        print(f"n={n_tokens} {name}: floor {floor:.3e}, GPU {err:.3e} vs fp32, {err_s:.3e} vs storage precision")
        assert_at_dtype_floor(err, err_s, floor)
    # K is normalised per head: mean square 1 up to eps and bf16
    ms = got[1].reshape(L, 2, n_tokens, Hh, 128).pow(2).mean(-1)
    assert (ms - 1.0).abs().max() < 2e-2


# ------------------------------------------------------------------------------------------------------------------ the model
def _device_model(gpu, tp, ipp, x, scales, samples=True, fp8=False, fp8_attn=False):
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    if fp8:
        tr.enable_fp8_linears(fp8)
    if fp8_attn:
        tr.enable_fp8_attention(True)
    tr.load_ip_adapter(ipp)
    tr.set_ip_adapter_scale(scales)
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    kw = dict(hidden_states=b16(x["latents"]), encoder_hidden_states=b16(x["prompt"]), pooled_projections=b16(x["pooled"]),
              timestep=x["timestep"].to(gpu), img_ids=b16(x["img_ids"]), txt_ids=b16(x["txt_ids"]), guidance=x["guidance"].to(gpu),
              controlnet_block_samples=[b16(s) for s in x["samples"]] if samples else None, return_dict=False)
    return tr, kw, b16(x["embeds"])


def _check_model(tr, kw, emb, targs, okw, ikw, contexts, min_ratio, label):
    ref = ixr.transformer_forward(*targs, **okw, **ikw)
    with contextlib.ExitStack() as st:
        for c in contexts:
            st.enter_context(c())
        ref_s = ixr.transformer_forward(*targs, **okw, **ikw)
    without = ixr.transformer_forward(*targs, **okw)
    floor, moved = rel_l2(ref_s, ref), rel_l2(ref, without)
    print(f"{label}: floor {floor:.3e}, with-against-without {moved:.3e} (ratio {moved / floor:.1f})")
    assert moved >= min_ratio * floor, (moved, floor)                           # condition on the oracle: the term cannot hide
    out = tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})[0].float().cpu()
    err, err_s = rel_l2(out, ref), rel_l2(out, ref_s)
    print(f"{label}: GPU rel-L2 {err:.3e} vs fp32 restatement, {err_s:.3e} vs storage-precision restatement")
    assert_at_dtype_floor(err, err_s, floor)
    return out, ref, floor


@pytest.mark.parametrize("samples", [True, False])
def test_transformer_with_instantx_adapter(gpu, samples):
    """B = 2, per-sample embeds, N = 81, a 0 on one double and one single block; with and without ControlNet samples. The two wrong
    placements (text rows left out of the single-block term; the double-block term ungated) are >= 10 x floor from the reference, so
    an implementation with either mistake cannot pass (test_ip_adapter_instantx_host.py checks the same without a GPU)."""
    tp, ipp, x, targs, okw, ikw = ixr.model_case(samples=samples)
    tr, kw, emb = _device_model(gpu, tp, ipp, x, ixr.MODEL_SCALES, samples=samples)
    out, ref, floor = _check_model(tr, kw, emb, targs, okw, ikw, [lambda: orc.stored_as(torch.bfloat16)], 10, f"bf16 samples={samples}")
    for variant in ("no_text_rows", "ungated"):
        dist = rel_l2(ixr.transformer_forward(*targs, **okw, **ikw, variant=variant), ref)
        print(f"variant {variant}: {dist:.3e} from the reference ({dist / floor:.1f} x floor)")
        assert dist >= 10 * floor, (variant, dist, floor)
    prepared = tr._ip_adapter.prepare(emb)
    assert torch.equal(tr(**kw, _ip=prepared)[0].float().cpu(), out)
    plain = tr(**kw)[0].float().cpu()
    assert not torch.equal(plain, out)
    tr.set_ip_adapter_scale(0.0)
    assert torch.equal(tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})[0].float().cpu(), plain)
    tr.unload_ip_adapter()
    assert torch.equal(tr(**kw)[0].float().cpu(), plain)


@pytest.mark.parametrize("level, attn", [("ln", False), ("mx", False), ("mx", True), ("ln", True)])
def test_transformer_with_instantx_adapter_fp8_modes(gpu, level, attn):
    """The (level, attention) combinations of test_transformer_with_adapter_fp8_modes at its shape (N = 256, T = 64) and with its
    floor rule. In the "mx" + e4m3-attention mode a block with the adapter takes the bf16-output attention and the quantise pass."""
    scales = [1.0, -0.7, 0.9, -0.5]
    tp, ipp, x, targs, okw, ikw = ixr.model_case(seed=440, h2=32, w2=32, scales=scales)
    tr, kw, emb = _device_model(gpu, tp, ipp, x, scales, fp8=level, fp8_attn=attn)
    ctx = [lambda: orc.stored_as(torch.bfloat16), lambda: orc.fp8_linears(level)] + ([lambda: orc.fp8_attention()] if attn else [])
    _check_model(tr, kw, emb, targs, okw, ikw, ctx, 3, f"fp8 {level} attention={attn}")


# ------------------------------------------------------------------------------------------------------------------ the pipeline
PIPE_SCALES = [1.0, -0.7, 0.9, -0.5]


def _pipe_and_inputs(gpu, seed, steps=2):
    from test_ip_adapter_gpu import _pipe, _pipe_inputs

    pipe, tp, cp = _pipe(gpu, seed)
    kw, c = _pipe_inputs(gpu, seed + 1, steps=steps)
    ipp = ixr.init_instantx_params(SMALL_T, n_tokens=16, embed_dim=E, seed=seed + 2, v_std=ixr.MODEL_V_STD)
    return pipe, tp, cp, kw, c, ipp


def test_pipeline_two_steps_with_tower_masks_and_instantx_adapter(gpu, tmp_path):
    pipe, tp, cp, kw, c, ipp = _pipe_and_inputs(gpu, 601)
    pipe.capture_graphs = False
    base = pipe(**kw).images.clone()
    torch.save(ixr.to_nested(ipp), str(tmp_path / "ip-adapter.bin"))            # the upstream file form, through the public call
    pipe.load_ip_adapter(str(tmp_path), weight_name="ip-adapter.bin")
    assert pipe.transformer._ip_adapter.scales == [1.0] * 4
    pipe.set_ip_adapter_scale(PIPE_SCALES)
    emb = c["embeds"].to(gpu, torch.bfloat16)
    assert torch.equal(pipe(**kw).images, base)                                 # no embeds: bitwise the no-adapter result
    out = pipe(**kw, ip_adapter_image_embeds=[emb[:, None]]).images.float().cpu()
    sig = orc.flow_sigmas(2, orc.calculate_shift(256, 256, 4096, 0.5, 1.15))
    largs = (tp, SMALL_T, cp, SMALL_CN, c["lat0"], c["pe"], c["pooled"], [c["hint"]], [c["mask"]], sig, orc.latent_image_ids(32, 32), torch.zeros(64, 3), 3.5)
    ikw = dict(ip_params=ipp, ip_embeds=c["embeds"], ip_scales=PIPE_SCALES)
    ref = ixr.denoise_loop(*largs, **ikw)
    with orc.stored_as(torch.bfloat16):
        ref16 = ixr.denoise_loop(*largs, **ikw)
    without = orc.denoise_loop(*largs)
    floor, moved = rel_l2(ref16, ref), rel_l2(ref, without)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"pipeline + InstantX adapter: rel-L2 {err:.3e} vs fp32 loop, {err16:.3e} vs bf16-storage loop (floor {floor:.3e}); the adapter moves "
          f"the latents by {moved:.3e}")
    assert moved >= 10 * floor
    assert_at_dtype_floor(err, err16, floor)
    pipe.set_ip_adapter_scale(0.0)
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=emb).images, base)   # all scales 0: bitwise the no-adapter image
    with pytest.raises(ValueError, match="width 768"):
        pipe(**kw, ip_adapter_image_embeds=torch.zeros(1, 1, 768, device=gpu, dtype=torch.bfloat16))


def test_pipeline_graph_with_instantx_adapter(gpu):
    pipe, tp, cp, kw, c, ipp = _pipe_and_inputs(gpu, 611, steps=3)
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale(PIPE_SCALES)
    e1, e2 = c["embeds"].to(gpu, torch.bfloat16), c["embeds2"].to(gpu, torch.bfloat16)
    pipe.capture_graphs = False
    eager1 = pipe(**kw, ip_adapter_image_embeds=e1).images.clone()
    eager2 = pipe(**kw, ip_adapter_image_embeds=e2).images.clone()
    base = pipe(**kw).images.clone()
    assert not torch.equal(eager1, eager2) and not torch.equal(eager1, base)
    pipe.capture_graphs = True
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # first sight: eager
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # captured + replayed
    n_before = len(calls)
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # replay only
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e2).images, eager2)  # new embed VALUES: the same graph, copied in
    assert len(calls) == n_before
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 1
    # a changed scale of a SINGLE block is another signature: a new graph with the right answer
    other = [1.0, -0.7, 0.9, 0.4]
    pipe.set_ip_adapter_scale(other)
    pipe._denoise_eager = orig
    pipe.capture_graphs = False
    eager3 = pipe(**kw, ip_adapter_image_embeds=e2).images.clone()
    assert not torch.equal(eager3, eager2)
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e2).images, eager3)
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 2
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, base)


def test_xlabs_adapter_stays_on_the_unchanged_branch(gpu, monkeypatch):
    """An XLabs adapter on the same model reaches run_double as before — (K, V, scale) with ip_inside off — and run_single without
    an adapter; the result is what run_double's unchanged branch gives when it is driven directly."""
    from reptext_amd import mmdit

    tp, _, x, _, _, _ = ixr.model_case()
    ipp = ipr.to_xlabs(ipr.init_ip_params(SMALL_T, n_tokens=16, embed_dim=E, seed=701))
    tr, kw, emb = _device_model(gpu, tp, ipp, x, [0.8, -0.5])
    seen = []
    real_double, real_single = mmdit.run_double, mmdit.run_single

    def spy_double(*a, **k):
        seen.append(("double", k.get("ip") is not None, bool(k.get("ip_inside", False))))
        return real_double(*a, **k)

    def spy_single(*a, **k):
        seen.append(("single", k.get("ip") is not None, False))
        return real_single(*a, **k)

    monkeypatch.setattr(mmdit, "run_double", spy_double)
    monkeypatch.setattr(mmdit, "run_single", spy_single)
    out = tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})[0].clone()
    assert seen == [("double", True, False)] * 2 + [("single", False, False)] * 2, seen
    # the same blocks driven with the parent commit's call form (no ip_inside argument at all, no ip= to run_single)
    prep = tr._ip_adapter.prepare(emb)
    assert not prep.inside and len(prep.kv) == 2

    def old_double(pl, ws, temb, cos, sin, H, inject=None, mods=None, ip=None, ip_inside=False):
        return real_double(pl, ws, temb, cos, sin, H, inject=inject, mods=mods, ip=ip)

    def old_single(pl, ws, temb, cos, sin, H, inject=None, mods=None, ip=None):
        return real_single(pl, ws, temb, cos, sin, H, inject=inject, mods=mods)

    monkeypatch.setattr(mmdit, "run_double", old_double)
    monkeypatch.setattr(mmdit, "run_single", old_single)
    assert torch.equal(tr(**kw, _ip=prep)[0], out)
    assert not torch.equal(tr(**kw)[0], out)
