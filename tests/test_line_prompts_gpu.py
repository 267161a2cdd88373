"""Per-line prompts end to end on the GPU: the transformer with key groups and the pipelines' ``control_prompt_embeds``
against tests/line_prompt_reference.py — the oracle's own forward and loop with the masked softmax in place of ``orc.attention``.

Model: SMALL_T / SMALL_CN, latents 32 x 32 (N = 256 on a 16 x 16 token grid), T0 = 64, L = 64, two masked text lines with disjoint
boxes: S = 64 + 2 * 64 + 256 = 448. "The line prompts are felt" is a condition on the inputs, checked on the CPU with the references
alone before the GPU is involved: the result with them lies more than 20 x the bf16 floor from the result of the same call with the
line bits cleared from the image rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import BOXES, H, N, T, W, graph_keys, mask_images, random_pipe, token_mask, two_line_call  # noqa: E402
from test_true_cfg_host import _kw, _pipe, assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2  # noqa: E402

import line_prompt_reference as lpr  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

pytestmark = pytest.mark.gpu

L = 64
ENDS = (T, T + L, T + 2 * L, T + 2 * L + N)
# These reduced random models hardly read their text stream: replacing the WHOLE base prompt moves the transformer's output by 2 x its
# bf16 floor, and two line prompts seen from the two boxes by 0.8 x (measured on the CPU references alone). Drawing the line embeddings
# larger does not help — the text stream's first LayerNorm takes the gain out again (LINE_GAIN only turns them away from the
# context_embedder's bias) —, so "the line prompts are felt" is arranged in the weights: the double blocks' text value projection is
# drawn TEXT_V_GAIN times as large, which is linear in the distance (x 32: 14 x floor, x 64: 29 x) and leaves the floor where it was.
LINE_GAIN = 3.0
TEXT_V_GAIN = 64.0


def reference_params():
    tp = orc.init_mmdit_params(SMALL_T, seed=811)
    cp = orc.init_mmdit_params(SMALL_CN, seed=812, controlnet=True)
    for i in range(SMALL_T["num_layers"]):
        for part in ("weight", "bias"):
            k = f"transformer_blocks.{i}.attn.add_v_proj.{part}"
            tp[k] = (tp[k] * TEXT_V_GAIN).to(torch.bfloat16).float()
    return tp, cp


def table(masks, cfg=False, lines=True):
    """The contract written out for two lines with prompts: uint32 words as int32 [B or 2B, S]. masks: per line [1 or B, N, 1] token masks.
    ``lines=False``: the line bits cleared from the image rows."""
    B = max(m.shape[0] for m in masks)
    v = np.full((B, ENDS[-1]), 1 | 8, dtype=np.uint32)
    v[:, T : T + L], v[:, T + L : T + 2 * L] = 2 | 8, 4 | 8
    neg = v.copy()
    if lines:
        for r, m in enumerate(masks, start=1):
            v[:, T + 2 * L :] |= np.where(m.reshape(m.shape[0], N).float().numpy() > 0, np.uint32(1 << r), np.uint32(0))
    return torch.from_numpy((np.concatenate([neg, v]) if cfg else v).view(np.int32))


def models_on(gpu, tp, cp):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp); cn.load_state_dict(cp)
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return tr, pipe


@pytest.fixture(scope="module")
def setup(gpu):
    """Weights, inputs and token masks shared by the reference tests; computed once, never modified."""
    tp, cp = reference_params()
    tr, pipe = models_on(gpu, tp, cp)
    g = torch.Generator().manual_seed(813)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    x = dict(pe=r(2, T, 256), pooled=r(2, 64), npe=(3 * r(2, T, 256)).to(torch.bfloat16).float(), npooled=(3 * r(2, 64)).to(torch.bfloat16).float(),
             lines=[(LINE_GAIN * r(2, L, 256)).to(torch.bfloat16).float() for _ in range(2)], lat=orc.pack_latents(r(2, 16, 32, 32)),
             hints=[r(2, N, 128), r(2, N, 128)])
    rms = [token_mask(b) for b in BOXES]
    assert float((rms[0] * rms[1]).abs().max()) == 0.0 and all(float(m.max()) > 0 for m in rms)        # disjoint, non-empty
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    return dict(tp=tp, cp=cp, tr=tr, pipe=pipe, x=x, rms=rms, sig=sig, ids=orc.latent_image_ids(32, 32))


def both(fn):
    """(fp32 reference, bf16-storage reference) of fn()."""
    ref = fn()
    with orc.stored_as(torch.bfloat16):
        ref16 = fn()
    return ref, ref16


def b16(t, gpu):
    return t.to(gpu, torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ 1. one forward
def test_transformer_forward_with_key_groups(setup, gpu):
    import reptext_amd.ops as ops

    s, x = setup, setup["x"]
    one = lambda t: t[:1]
    le = torch.cat([one(l) for l in x["lines"]], dim=1)
    ts, gd = torch.full((1,), 0.622459), torch.full((1,), 3.5)
    fwd = lambda vis: lpr.transformer_forward(s["tp"], SMALL_T, one(x["lat"]), one(x["pe"]), one(x["pooled"]), ts, s["ids"], None, guidance=gd,
                                              line_embeds=le, ends=ENDS, row_vis=vis)
    ref, ref16 = both(lambda: fwd(table(s["rms"])))
    floor = rel_l2(ref16, ref)
    unseen, unseen16 = both(lambda: fwd(table(s["rms"], lines=False)))
    felt = rel_l2(unseen, ref)
    print(f"line prompts, one forward: bf16 floor {floor:.3e}; with the line bits cleared the reference lies {felt:.3e} = {felt / floor:.0f} x floor away")
    assert felt > 20 * floor

    def run(vis, pe):
        Tt = pe.shape[1]
        kw = {} if vis is None else dict(_groups=ops.KeyGroups(ENDS, vis.to(gpu)))
        return s["tr"](hidden_states=b16(one(x["lat"]), gpu), encoder_hidden_states=b16(pe, gpu), pooled_projections=b16(one(x["pooled"]), gpu),
                       timestep=ts.to(gpu), img_ids=b16(s["ids"], gpu), txt_ids=torch.zeros(Tt, 3, device=gpu, dtype=torch.bfloat16),
                       guidance=gd.to(gpu), return_dict=False, **kw)[0].float().cpu()

    joint = torch.cat([one(x["pe"]), le], dim=1)
    out = run(table(s["rms"]), joint)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line prompts, one forward: rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    # a line prompt nobody sees is not there: with the line bits cleared the image tokens get what the plain call at T0 gives them
    plain, plain16 = both(lambda: orc.transformer_forward(s["tp"], SMALL_T, one(x["lat"]), one(x["pe"]), one(x["pooled"]), ts, s["ids"],
                                                          torch.zeros(T, 3), guidance=gd))
    assert rel_l2(unseen, plain) < 1e-5                                    # the two references agree: same keys, other summation order
    out0 = run(table(s["rms"], lines=False), joint)
    e0, e016, floor0 = rel_l2(out0, plain), rel_l2(out0, plain16), rel_l2(plain16, plain)
    print(f"unseen line prompts vs the plain call at T0: rel-L2 {e0:.3e} / {e016:.3e} (floor {floor0:.3e})")
    assert_at_dtype_floor(e0, e016, floor0)
    dense = run(None, one(x["pe"]))
    assert rel_l2(out0, dense) <= 1.45 * floor0 + 1e-4                     # and the plain GPU call itself, at the distance of two bf16 runs


# ------------------------------------------------------------------------------------------------------------------ 2. the loop
def loop_case(s, B, cfg, per_image=False):
    """(pipeline call, reference thunk) of a 3-step loop with the text tower on two masked lines, at batch B."""
    x = s["x"]
    cut = lambda t: t[:B]
    if per_image:       # entry 1 takes the boxes the other way round
        rms = [torch.cat([token_mask(BOXES[0]), token_mask(BOXES[1])]), torch.cat([token_mask(BOXES[1]), token_mask(BOXES[0])])]
    else:
        rms = s["rms"]
    le = torch.cat([cut(l) for l in x["lines"]], dim=1)
    vis = table(rms if per_image else [m.expand(B, -1, -1) for m in rms], cfg=cfg)
    args = (s["tp"], SMALL_T, s["cp"], SMALL_CN, cut(x["lat"]), cut(x["pe"]), cut(x["pooled"]), [cut(h) for h in x["hints"]], rms, s["sig"], s["ids"],
            torch.zeros(T, 3), 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=2, image_prompt=lpr.image_prompt_slot(le, ENDS, vis))
    if cfg:
        rkw["negative"] = dict(prompt_embeds=cut(x["npe"]), pooled=cut(x["npooled"]), scale=2.0)
    return args, rkw, rms, le


def pipe_call(s, gpu, B, cfg, rms, per_image, lines=True):
    x = s["x"]
    cut = lambda t: b16(t[:B], gpu)
    kw = dict(prompt_embeds=cut(x["pe"]), pooled_prompt_embeds=cut(x["pooled"]), height=H, width=W, num_inference_steps=3, guidance_scale=3.5,
              control_image=[cut(h) for h in x["hints"]], control_mask=[b16(m, gpu) for m in rms] if per_image else mask_images(BOXES),
              controlnet_conditioning_scale=1.0, controlnet_conditioning_step=2, latents=cut(x["lat"]), output_type="latent")
    if lines:
        kw["control_prompt_embeds"] = [cut(l) for l in x["lines"]]
        kw["control_prompt_max_sequence_length"] = L
    if cfg:
        kw.update(negative_prompt_embeds=cut(x["npe"]), negative_pooled_prompt_embeds=cut(x["npooled"]), true_cfg_scale=2.0)
    return kw


@pytest.mark.parametrize("B,cfg,interval", [(1, False, None), (1, True, None), (2, True, None), (2, True, (0.0, 0.67))])
def test_loop_matches_the_reference(setup, gpu, B, cfg, interval):
    """3 steps, the tower on two masked lines for 2 of them; plain, under true CFG, and at B = 2 with per-image masks under true CFG,
    where each sample also equals its own B = 1 call bit for bit. With a guider whose interval ends after the second step the third
    runs on the positive half alone: rows [B:] of the [2B, S] table."""
    from reptext_amd.guidance import TrueCFGGuider

    s = setup
    per_image = B == 2
    args, rkw, rms, le = loop_case(s, B, cfg, per_image)
    guider = None if interval is None else TrueCFGGuider(start=interval[0], stop=interval[1])
    rkw["guider"] = guider
    ref, ref16 = both(lambda: denoise_loop_reference(*args, **rkw))
    floor = rel_l2(ref16, ref)
    if B == 1:
        cleared = dict(rkw, image_prompt=lpr.image_prompt_slot(le, ENDS, table(rms, cfg=cfg, lines=False)))
        felt = rel_l2(denoise_loop_reference(*args, **cleared), ref)
        print(f"line prompts, loop B={B} cfg={cfg}: with the line bits cleared the reference lies {felt:.3e} = {felt / floor:.0f} x floor away")
        assert felt > 20 * floor
    pipe = s["pipe"]
    pipe.capture_graphs = False
    pipe.guider = guider
    kw = pipe_call(s, gpu, B, cfg, rms, per_image)
    try:
        out = pipe(**kw).images.float().cpu()
    finally:
        pipe.guider = None
    assert pipe._tower_window_used is not None
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line prompts, loop B={B} cfg={cfg}: latents rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)
    if B == 2 and guider is None:
        whole = pipe(**kw).images
        for b in range(2):
            one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if isinstance(v, list) else v) for k, v in kw.items()}
            assert torch.equal(pipe(**one).images, whole[b : b + 1]), b


# ------------------------------------------------------------------------------------------------------------------ 3. capture
def line_kw(r, B=1):
    return dict(control_prompt_embeds=[LINE_GAIN * r(B, L, 256), LINE_GAIN * r(B, L, 256)], control_prompt_max_sequence_length=L)


def test_capture_and_replay_are_the_eager_bits(gpu):
    pipe, r = random_pipe(gpu, 821)
    kw = two_line_call(r)
    lkw = dict(kw, **line_kw(r))
    fresh, r2 = random_pipe(gpu, 821)
    want_plain = fresh(**two_line_call(r2)).images.clone()
    plain_key = graph_keys(fresh)
    assert torch.equal(pipe(**kw).images, want_plain)                       # before: the key and the bits of a fresh pipeline
    keys = graph_keys(pipe)
    # the key a fresh pipeline builds for the plain call: entry for entry, but for the one that identifies the models
    assert len(keys) == 1 and len(keys[0]) == len(plain_key[0]) and sum(a != b for a, b in zip(keys[0], plain_key[0])) == 1
    assert "line_prompts" not in str(keys[0])
    pipe.capture_graphs = False
    eager = pipe(**lkw).images.clone()
    assert not torch.equal(eager, want_plain)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**lkw).images, eager)
    keys2 = graph_keys(pipe)
    assert len(keys2) == 2 and keys2[0] == keys[0] and isinstance(pipe._graph_cache[keys2[1]], dict)
    tag = [e for e in keys2[1] if isinstance(e, tuple) and e and e[0] == "line_prompts"]
    assert len(tag) == 1 and tag[0][1] == ENDS
    # new line embeddings, same signature: replayed, copied in
    lkw2 = dict(kw, **line_kw(r))
    pipe.capture_graphs = False
    eager2 = pipe(**lkw2).images.clone()
    pipe.capture_graphs = True
    assert torch.equal(pipe(**lkw2).images, eager2) and not torch.equal(eager2, eager) and graph_keys(pipe) == keys2
    for _ in range(3):                                                      # after: the plain call is what it was (captured, replayed)
        assert torch.equal(pipe(**kw).images, want_plain)
    assert graph_keys(pipe) == keys2
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 4. toggles
def test_overlap_and_row_window_are_bitwise_neutral_with_line_prompts(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 831)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, steps=3, cn_steps=3), **line_kw(r))
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    want = pipe(**kw).images.clone()
    assert pipe._tower_window_used is None
    for overlap, window in ((True, False), (False, True), (True, True)):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        monkeypatch.setattr(P, "TOWER_WINDOW", window)
        assert torch.equal(pipe(**kw).images, want), (overlap, window)
        assert (pipe._tower_window_used is not None) == window


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    pipe, r = random_pipe(gpu, 841)
    kw = dict(two_line_call(r), **line_kw(r))
    pipe.transformer.enable_fp8_attention(True)
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**kw)
    pipe.transformer.enable_fp8_attention(False)
    assert pipe(**kw).images.shape == (1, N, 64)
    with pytest.raises(ValueError, match="control_mask"):
        pipe(**dict(kw, control_mask=None))
    with pytest.raises(ValueError, match="inpaint pipeline does not support per-line prompts"):
        _pipe(inpaint=True)(**_kw(), control_prompt_embeds=[torch.zeros(1, L, 64)])
    assert_no_call_state(pipe)
