"""Regional image prompts end to end on the GPU: ``ip_adapter_mask`` and one image prompt per text line through the one
loaded adapter, in both layouts, against tests/regional_ip_reference.py (the blocks restated with a list of weighted terms) inside
tests/loop_reference.py's loop.

Model: SMALL_T / SMALL_CN, latents 32 x 32 (N = 256 on a 16 x 16 token grid), T = 64, two masked text lines with OVERLAPPING boxes,
2 steps with the tower on. "The regional terms are felt" is a condition on the inputs, checked with the references alone before the
GPU is compared: with against without the line terms, and masked against unmasked, lie at least 5 x the bf16 floor apart. It is
arranged in the weights: the adapter's value projections are drawn V_GAIN times as large (the InstantX cases take the v_std the existing
InstantX tests take)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import H, N, T, W, graph_keys, mask_images, token_mask  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402

import instantx_reference as ixr  # noqa: E402
import ip_adapter_reference as ipr  # noqa: E402
import line_prompt_reference as lpr  # noqa: E402
import regional_ip_reference as rr  # noqa: E402
from instantx_reference import SMALL_CN, SMALL_T, rel_l2  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

pytestmark = pytest.mark.gpu

E = 64
BOXES = ((48, 112, 30, 200), (96, 160, 120, 240))          # overlapping: image rows 96..112, columns 120..200 belong to both lines
GLOBAL_BOX = (0, 256, 0, 136)                               # the call's own prompt: the left half, a fractional edge at token column 8
LINE_SCALES = [1.0, 1.5]
SCALES = {"instantx": [1.0, -0.7, 0.9, -0.5], "diffusers": [1.0, -0.7]}
V_GAIN = 10.0
STEPS = 2
L = 64


@functools.lru_cache(maxsize=None)
def params(layout):
    tp = orc.init_mmdit_params(SMALL_T, seed=911)
    cp = orc.init_mmdit_params(SMALL_CN, seed=912, controlnet=True)
    if layout == "instantx":
        ipp = ixr.init_instantx_params(SMALL_T, n_tokens=16, embed_dim=E, seed=913, v_std=ixr.MODEL_V_STD)
    else:
        ipp = ipr.init_ip_params(SMALL_T, n_tokens=16, embed_dim=E, seed=913)
        for k in [k for k in ipp if "to_v_ip" in k]:
            ipp[k] = (ipp[k] * V_GAIN).to(torch.bfloat16).float()
    return tp, cp, ipp


@functools.lru_cache(maxsize=None)
def inputs():
    g = torch.Generator().manual_seed(914)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    x = dict(pe=r(2, T, 256), pooled=r(2, 64), npe=(3 * r(2, T, 256)).to(torch.bfloat16).float(), npooled=(3 * r(2, 64)).to(torch.bfloat16).float(),
             lat=orc.pack_latents(r(2, 16, 32, 32)), hints=[r(2, N, 128), r(2, N, 128)], e0=r(2, E), neg=r(2, E), e1=r(2, E), e2=r(2, E),
             e1b=r(2, E), lines=[(3.0 * r(2, L, 256)).to(torch.bfloat16).float() for _ in range(2)])
    x["rms"] = [token_mask(b) for b in BOXES]
    x["gm"] = token_mask(GLOBAL_BOX)
    assert float((x["rms"][0] * x["rms"][1]).max()) > 0                      # the boxes overlap
    assert 0 < float(x["gm"].reshape(16, 16)[0, 8]) < 1                       # a fractional edge
    x["sig"] = orc.flow_sigmas(STEPS, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    x["ids"] = orc.latent_image_ids(32, 32)
    return x


def models_on(gpu, tp, cp):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    cn.load_state_dict(cp)
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return tr, pipe


@functools.lru_cache(maxsize=None)
def device_pipe(layout, fp8=False):
    tp, cp, ipp = params(layout)
    tr, pipe = models_on(torch.device("cuda:0"), tp, cp)
    if fp8:
        tr.enable_fp8_linears("mx")
        tr.enable_fp8_attention(True)
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale(SCALES[layout])
    return pipe


def terms_of(case, B=1, rms=None, gm=None, line_embeds=("e1", "e2"), line_scales=LINE_SCALES):
    """The reference's terms of a case: "g" the call's own prompt, "m" with its mask, "l" the two line prompts."""
    x = inputs()
    rms = x["rms"] if rms is None else rms
    out = []
    if "g" in case:
        out.append(dict(embeds=x["e0"][:B], neg_embeds=x["neg"][:B], mask=(x["gm"] if gm is None else gm) if "m" in case else None, scale=1.0, line=False))
    if "l" in case:
        out += [dict(embeds=x[k][:B], mask=m, scale=s, line=True) for k, m, s in zip(line_embeds, rms, line_scales)]
    return out


def reference(layout, case, B=1, cfg=False, guider=None, rms=None, modes=(), prompts=False):
    """(fp32, storage precision) latents of the loop reference for the case."""
    x = inputs()
    tp, cp, ipp = params(layout)
    rms = x["rms"] if rms is None else rms
    cut = lambda t: t[:B]
    lines = None
    if prompts:
        from test_line_prompts_gpu import table
        lines = (torch.cat([cut(l) for l in x["lines"]], dim=1), (T, T + L, T + 2 * L, T + 2 * L + N), table([m.expand(B, -1, -1) for m in rms], cfg=cfg))
    args = (tp, SMALL_T, cp, SMALL_CN, cut(x["lat"]), cut(x["pe"]), cut(x["pooled"]), [cut(h) for h in x["hints"]], rms, x["sig"], x["ids"],
            torch.zeros(T, 3), 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=STEPS, guider=guider,
               image_prompt=rr.image_prompt_slot(ipp, SCALES[layout], terms_of(case, B, rms), layout, B, lines=lines))
    if cfg:
        rkw["negative"] = dict(prompt_embeds=cut(x["npe"]), pooled=cut(x["npooled"]), scale=2.0)
    ref = denoise_loop_reference(*args, **rkw)
    import contextlib
    with contextlib.ExitStack() as st:
        st.enter_context(orc.stored_as(torch.bfloat16))
        for m in modes:
            st.enter_context(m())
        ref16 = denoise_loop_reference(*args, **rkw)
    return ref, ref16


reference_cached = functools.lru_cache(maxsize=None)(lambda layout, case, cfg=False, prompts=False: reference(layout, case, cfg=cfg, prompts=prompts))


def call(case, B=1, cfg=False, per_image=None, prompts=False, **over):
    """The pipeline call of a case (see ``terms_of``)."""
    x = inputs()
    dev = lambda t: t[:B].to("cuda:0", torch.bfloat16)
    kw = dict(prompt_embeds=dev(x["pe"]), pooled_prompt_embeds=dev(x["pooled"]), height=H, width=W, num_inference_steps=STEPS, guidance_scale=3.5,
              control_image=[dev(h) for h in x["hints"]], control_mask=mask_images(BOXES) if per_image is None else [m.to("cuda:0", torch.bfloat16) for m in per_image],
              controlnet_conditioning_scale=1.0, controlnet_conditioning_step=STEPS, latents=dev(x["lat"]), output_type="latent")
    if "g" in case:
        kw["ip_adapter_image_embeds"] = dev(x["e0"])
        if cfg:
            kw["negative_ip_adapter_image_embeds"] = dev(x["neg"])
    if "m" in case:
        kw["ip_adapter_mask"] = mask_images([GLOBAL_BOX])[0]
    if "l" in case:
        kw.update(control_ip_adapter_image_embeds=[dev(x["e1"]), dev(x["e2"])[:, None]], control_ip_adapter_scale=list(LINE_SCALES))
    if prompts:
        kw.update(control_prompt_embeds=[dev(l) for l in x["lines"]], control_prompt_max_sequence_length=L)
    if cfg:
        kw.update(negative_prompt_embeds=dev(x["npe"]), negative_pooled_prompt_embeds=dev(x["npooled"]), true_cfg_scale=2.0)
    kw.update(over)
    return kw


def run(pipe, kw, guider=None, graphs=False):
    pipe.capture_graphs, pipe.guider = graphs, guider
    try:
        return pipe(**kw).images.clone()
    finally:
        pipe.guider = None


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("layout", ["instantx", "diffusers"])
@pytest.mark.parametrize("case, prompts", [("gm", False), ("l", False), ("gl", False), ("gml", True)])
def test_loop_matches_the_reference(gpu, layout, case, prompts):
    """The call's own prompt under a mask; two line image prompts alone; both kinds with overlapping boxes; and all of it with
    per-line text prompts too. Always with the tower's masked samples."""
    ref, ref16 = reference_cached(layout, case, prompts=prompts)
    floor = rel_l2(ref16, ref)
    # the visibility condition, on the references alone
    if "l" in case:
        felt = rel_l2(reference_cached(layout, case.replace("l", "") or "none", prompts=prompts)[0], ref)
        print(f"{layout} {case}: without the line terms the reference lies {felt:.3e} = {felt / floor:.1f} x floor away")
        assert felt >= 5 * floor, (felt, floor)
    if "m" in case:
        felt = rel_l2(reference_cached(layout, case.replace("m", ""), prompts=prompts)[0], ref)
        print(f"{layout} {case}: with the call's own prompt unmasked the reference lies {felt:.3e} = {felt / floor:.1f} x floor away")
        assert felt >= 5 * floor, (felt, floor)
    pipe = device_pipe(layout)
    out = run(pipe, call(case, prompts=prompts)).float().cpu()
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"{layout} {case} prompts={prompts}: latents rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)


@pytest.mark.parametrize("layout", ["instantx", "diffusers"])
@pytest.mark.parametrize("interval", [None, (0.0, 0.5)])
def test_true_cfg_and_guider(gpu, layout, interval):
    """True CFG at B = 1: the negative half gets the negative image embedding under the same mask and no line term. A guider that ends
    after the first step: the second runs on the positive half, the [B:] views of every table."""
    from reptext_amd.guidance import TrueCFGGuider

    guider = None if interval is None else TrueCFGGuider(start=interval[0], stop=interval[1])
    ref, ref16 = reference(layout, "gml", cfg=True, guider=guider)
    floor = rel_l2(ref16, ref)
    x = inputs()
    if interval is None:        # a line term in the negative half too would be visible
        both_halves = [dict(t, line=False, neg_embeds=t["embeds"]) if t["line"] else t for t in terms_of("gml")]
        tp, cp, ipp = params(layout)
        cut = lambda t: t[:1]
        wrong = denoise_loop_reference(tp, SMALL_T, cp, SMALL_CN, cut(x["lat"]), cut(x["pe"]), cut(x["pooled"]), [cut(h) for h in x["hints"]], x["rms"],
                                       x["sig"], x["ids"], torch.zeros(T, 3), 3.5, conditioning_scale=1.0, conditioning_step=STEPS,
                                       negative=dict(prompt_embeds=cut(x["npe"]), pooled=cut(x["npooled"]), scale=2.0),
                                       image_prompt=rr.image_prompt_slot(ipp, SCALES[layout], both_halves, layout, 1))
        felt = rel_l2(wrong, ref)
        print(f"{layout} cfg: line terms in the negative half too lie {felt:.3e} = {felt / floor:.1f} x floor away")
        assert felt >= 5 * floor
    pipe = device_pipe(layout)
    out = run(pipe, call("gml", cfg=True), guider=guider).float().cpu()
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"{layout} cfg interval={interval}: rel-L2 {err:.3e} vs fp32, {err16:.3e} vs bf16-storage (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)


def test_fp8_mx_with_e4m3_attention(gpu):
    """The mode of test_transformer_with_instantx_adapter_fp8_modes ("mx", e4m3 attention) and its reference mode."""
    modes = (lambda: orc.fp8_linears("mx"), lambda: orc.fp8_attention())
    ref, ref16 = reference("instantx", "gml", modes=modes)
    floor = rel_l2(ref16, ref)
    out = run(device_pipe("instantx", fp8=True), call("gml")).float().cpu()
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"fp8 mx + e4m3 attention: rel-L2 {err:.3e} vs fp32, {err16:.3e} vs the mode's reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)


# ------------------------------------------------------------------------------------------------------------------ 2. bitwise identities
@pytest.mark.parametrize("layout", ["instantx", "diffusers"])
def test_bitwise_identities(gpu, layout):
    from PIL import Image

    pipe = device_pipe(layout)
    x = inputs()
    dev = lambda t: t.to(gpu, torch.bfloat16)
    # an all-white ip_adapter_mask is the call without the mask
    plain = run(pipe, call("g"))
    white = Image.fromarray(np.full([H, W], 255, dtype=np.uint8))
    assert torch.equal(run(pipe, call("g", ip_adapter_mask=white)), plain)
    assert not torch.equal(run(pipe, call("gm")), plain)
    # a line image prompt under an empty control_mask, beside an active global prompt, is that entry None
    empty = [token_mask(BOXES[0]), torch.zeros(1, N, 1)]
    e1, e2 = dev(x["e1"][:1]), dev(x["e2"][:1])
    with_empty = run(pipe, call("g", per_image=empty, control_ip_adapter_image_embeds=[e1, e2]))
    assert torch.equal(with_empty, run(pipe, call("g", per_image=empty, control_ip_adapter_image_embeds=[e1, None])))
    assert not torch.equal(with_empty, run(pipe, call("g", per_image=empty)))
    full = [token_mask(b) for b in BOXES]
    # B = 2 with per-sample masks: each sample is its own B = 1 call
    per = [torch.cat([full[0], full[1]]), torch.cat([full[1], full[0]])]
    gmask = torch.cat([token_mask(GLOBAL_BOX), token_mask((0, 136, 0, 256))])
    kw2 = call("gl", B=2, per_image=per, ip_adapter_mask=dev(gmask))
    whole = run(pipe, kw2)
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, list) else v)
               for k, v in kw2.items()}
        assert torch.equal(run(pipe, one), whole[b : b + 1]), b


@pytest.mark.parametrize("layout", ["instantx", "diffusers"])
def test_scale_folds_into_the_weights(gpu, layout):
    """control_ip_adapter_scale = 0.5 with weights m equals scale 1 with weights m / 2 (m / 2 exact): the terms prepared by hand, so
    that the towers' masks stay what they are."""
    from reptext_amd.ip_adapter import regional_ip_weights

    pipe = device_pipe(layout)
    tr, x = pipe.transformer, inputs()
    m = x["rms"][0]
    emb = [x["e0"][:1].to(gpu, torch.bfloat16), x["e1"][:1].to(gpu, torch.bfloat16)]
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    kw = dict(hidden_states=b16(x["lat"][:1]), encoder_hidden_states=b16(x["pe"][:1]), pooled_projections=b16(x["pooled"][:1]),
              timestep=torch.full((1,), 0.6, device=gpu), img_ids=b16(x["ids"]), txt_ids=torch.zeros(T, 3, device=gpu, dtype=torch.bfloat16),
              guidance=torch.full((1,), 3.5, device=gpu), return_dict=False)
    outs = []
    for mask, scale in ((m, 0.5), (m / 2, 1.0), (m, 1.0)):
        terms = tr._ip_adapter.prepare_terms(emb, [(None, None), regional_ip_weights(mask, scale, N=N, line=True)], T=T)
        outs.append(tr(**kw, _ip=terms)[0].clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    # one term without weights through the list is the single prepared term
    single = tr(**kw, _ip=tr._ip_adapter.prepare(emb[0]))[0]
    assert torch.equal(tr(**kw, _ip=tr._ip_adapter.prepare_terms(emb[:1]))[0], single)


# ------------------------------------------------------------------------------------------------------------------ 3. capture
@pytest.mark.parametrize("layout", ["instantx", "diffusers"])
def test_capture_and_replay_are_the_eager_bits(gpu, layout):
    tp, cp, ipp = params(layout)
    _, pipe = models_on(gpu, tp, cp)
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale(SCALES[layout])
    x = inputs()
    dev = lambda t: t.to(gpu, torch.bfloat16)
    plain_kw = call("g")
    want_plain = run(pipe, plain_kw)
    assert torch.equal(run(pipe, plain_kw, graphs=True), want_plain)
    keys = graph_keys(pipe)
    assert len(keys) == 1 and "regional_ip" not in str(keys[0])              # a call without the new arguments builds the key it always built
    kw = call("gml")
    eager = run(pipe, kw)
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(run(pipe, kw, graphs=True), eager)
    keys2 = graph_keys(pipe)
    assert len(keys2) == 2 and keys2[0] == keys[0] and isinstance(pipe._graph_cache[keys2[1]], dict)
    tag = [e for e in keys2[1] if isinstance(e, tuple) and e and e[0] == "regional_ip"]
    assert len(tag) == 1 and tag[0][1] == 3 and tag[0][2] == (True, True, True)
    # other mask values and another line image, same shapes: the same graph, copied in
    # (the text lines keep their image rows: the towers' row window is part of every call's key)
    other = dict(kw, control_mask=mask_images(((48, 112, 60, 220), (96, 160, 20, 150))), ip_adapter_mask=mask_images([(100, 256, 0, 256)])[0],
                 control_ip_adapter_image_embeds=[dev(x["e1b"][:1]), dev(x["e2"][:1])])
    eager2 = run(pipe, other)
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        assert torch.equal(run(pipe, other, graphs=True), eager2) and not torch.equal(eager2, eager)
    finally:
        pipe._denoise_eager = orig
    assert not calls and graph_keys(pipe) == keys2
    for _ in range(2):
        assert torch.equal(run(pipe, plain_kw, graphs=True), want_plain)
    assert_no_call_state(pipe)


def test_a_call_with_every_loop_extension_is_captured_and_replayed_bit_for_bit(gpu):
    """Every field of ``LoopExtras`` that reaches the captured graph in ONE call of the repaint pipeline at B = 1: two masked text lines
    with a prompt (L = 64) and an image prompt each, the call's own image prompt under ``ip_adapter_mask``, the union tower on the first
    two of the three steps that run (4 grid steps, strength 0.75), true CFG with negative embeds, a projected guider that ends before the
    last step, source and mask as packed latents, the second-order scheduler. Eager = seen = captured = replayed; then new VALUES for
    every static input (same shapes, the text lines keep their image rows) replay the same graph without a call of the eager loop, and the
    scheduler's host state after a replay is what the eager call leaves."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.guidance import TrueCFGGuider
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline
    from reptext_amd.scheduler import FlowMatchMultistepScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tp, cp, ipp = params("instantx")
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    cn.load_state_dict(cp)
    pipe = FluxControlNetRepaintPipeline(FlowMatchMultistepScheduler(), None, None, None, None, None, tr, cn)      # fresh: its cache holds this key alone
    pipe.controlnet_union = FluxControlNetModel(**dict(SMALL_T, num_layers=2, num_single_layers=0), device=gpu, dtype=torch.bfloat16).random_init_(915)
    pipe.set_progress_bar_config(disable=True)
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale(SCALES["instantx"])
    guider = TrueCFGGuider(stop=0.67, eta=0.0, norm_threshold=2.0, momentum=-0.5)          # guided at steps 0 and 1 of the 3
    g = torch.Generator().manual_seed(916)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, torch.bfloat16)

    def drawn(boxes, global_box):
        """The arguments that become static inputs, drawn anew: every one of them but the latents comes from here."""
        return dict(control_mask=mask_images(boxes), ip_adapter_mask=mask_images([global_box])[0], control_image_union=r(1, N, 64),
                    image=r(1, N, 64).float() * 0.5 + 0.123, mask_image=(torch.rand(1, N, 64, generator=g) > 0.4).to(gpu, torch.float32),
                    controlnet_conditioning_scale_union=0.7, control_guidance_end_union=0.67, num_inference_steps=4, strength=0.75)

    kw = call("gml", cfg=True, prompts=True, **drawn(BOXES, GLOBAL_BOX))
    eager = run(pipe, kw, guider=guider)
    host = (pipe.scheduler._step_index, pipe.scheduler._history_len)
    assert host == (4, 1) and graph_keys(pipe) == []                           # begin index 1 + 3 steps; the history holds a velocity
    for _ in range(3):                                                          # seen, captured, replayed
        assert torch.equal(run(pipe, kw, guider=guider, graphs=True), eager)
        assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == host
    keys = graph_keys(pipe)
    assert len(keys) == 1 and isinstance(pipe._graph_cache[keys[0]], dict)
    tags = [e[0] for e in keys[0] if isinstance(e, tuple) and e and isinstance(e[0], str)]
    assert tags == ["cfg", "repaint", "guidance", "line_prompts", "regional_ip", "solver"] and "union" in keys[0]
    static = set(pipe._graph_cache[keys[0]]["static"])
    assert {"union_hint", "repaint_src", "repaint_noise", "repaint_mask", "line_embeds", "line_row_vis", "rip_embeds2", "rip_img_w0"} <= static
    assert "ip_embeds" not in static                                            # the call's own image prompt is the regional record's first term
    # new values for every static input
    other = dict(kw, **drawn(((48, 112, 60, 220), (96, 160, 20, 150)), (100, 256, 0, 256)), prompt_embeds=r(1, T, 256), pooled_prompt_embeds=r(1, 64),
                 negative_prompt_embeds=r(1, T, 256), negative_pooled_prompt_embeds=r(1, 64), control_image=[r(1, N, 128), r(1, N, 128)],
                 latents=r(1, N, 64), ip_adapter_image_embeds=r(1, E), negative_ip_adapter_image_embeds=r(1, E),
                 control_ip_adapter_image_embeds=[r(1, E), r(1, 1, E)], control_prompt_embeds=[r(1, L, 256), r(1, L, 256)])
    eager2 = run(pipe, other, guider=guider)
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        assert torch.equal(run(pipe, other, guider=guider, graphs=True), eager2) and not torch.equal(eager2, eager)
    finally:
        pipe._denoise_eager = orig
    assert not calls and graph_keys(pipe) == keys
    assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == host
    assert torch.equal(run(pipe, kw, guider=guider, graphs=True), eager)        # and the first values again
    assert_no_call_state(pipe)
