"""Region isolation of per-line prompts end to end on the GPU (``control_prompt_isolation=True``): the transformer with
``ops.KeyClasses`` and the pipelines' keyword against the oracle's own forward and loop under ``line_prompt_reference.masked_attention``,
given the bool [B, S, S] that this file builds from the two tables by its own restatement of the rule.

Model, weights and helpers are test_line_prompts_gpu.py's: SMALL_T / SMALL_CN, latents 32 x 32 (N = 256 on a 16 x 16 token grid),
T0 = 64, L = 64, two masked text lines, S = 448. The boxes are larger than that file's (84 tokens each, disjoint): with its 33-token boxes
isolation moves the fp32 reference by only 3.7-4.5 x the bf16 floor. "Isolation is felt" is a condition on the inputs, checked on the
CPU with the references alone before the GPU is involved: the isolated reference lies more than 10 x the bf16 floor from the reference
of the same call under the non-isolated rule (measured: one forward 16.0 x, the 3-step loops 15.6-17.1 x; each case prints its own).

What this file cannot see: whether a line's TEXT rows read only their own box. That half alone moves the output of these 2 + 3-block
models by 1.8-3.3 x the floor (measured with an image-value gain of up to 64), which no test at the floor can tell from rounding. It is
pinned by the known answers of test_line_isolation_host.py and by the per-element tests of test_attention_keyed_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import H, N, T, W, graph_keys, mask_images, random_pipe, token_mask, two_line_call  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2  # noqa: E402
from test_line_prompts_gpu import L, LINE_GAIN, b16, both, line_kw, models_on, reference_params  # noqa: E402

import line_prompt_reference as lpr  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

pytestmark = pytest.mark.gpu

BOXES = ((16, 112, 16, 240), (144, 240, 16, 240))        # 84 tokens each, disjoint
OTHER_BOXES = ((16, 112, 48, 208), (144, 240, 48, 208))  # the same token rows (the same tower window), other columns
S = T + 2 * L + N
FELT = 10.0


def tables(masks, cfg=False, isolated=True):
    """The rule written out for two lines with prompts and DISJOINT boxes -> (row_vis int32 [B or 2B, S], key_class uint8 [B or 2B, S]).
    Classes: 0 base, 1 and 2 the lines, 3 the background, 4 / 5 the image tokens in box 1 / 2. ``isolated=False``: the same keys under
    the rule without isolation (line rows read every image token; a box row every image token and its line)."""
    B = max(m.shape[0] for m in masks)
    in1, in2 = (np.broadcast_to(m.reshape(m.shape[0], N).float().numpy() > 0, (B, N)) for m in masks)
    assert not (in1 & in2).any()
    img = 8 | 16 | 32
    cls = np.zeros((B, S), dtype=np.uint8)
    cls[:, T : T + L], cls[:, T + L : T + 2 * L] = 1, 2
    cls[:, T + 2 * L :] = np.where(in1, 4, np.where(in2, 5, 3))
    neg = np.full((B, S), 1 | img, dtype=np.uint32)
    neg[:, T : T + L], neg[:, T + L : T + 2 * L] = (2 | 16, 4 | 32) if isolated else (2 | img, 4 | img)
    v = neg.copy()
    box1, box2 = (1 | 2 | 8 | 16, 1 | 4 | 8 | 32) if isolated else (1 | 2 | img, 1 | 4 | img)
    v[:, T + 2 * L :] = np.where(in1, box1, np.where(in2, box2, 1 | img)).astype(np.uint32)
    words = np.concatenate([neg, v]) if cfg else v
    return torch.from_numpy(words.view(np.int32)), torch.from_numpy(np.concatenate([cls, cls]) if cfg else cls)


def visible(row_vis, key_class):
    """bool [B, S, S]: row i sees key j iff bit key_class[b, j] of row_vis[b, i] is set."""
    w, c = row_vis.numpy().view(np.uint32), key_class.numpy().astype(np.uint32)
    return torch.from_numpy(((w[:, :, None] >> c[:, None, :]) & 1).astype(bool))


def forward_under(see):
    """orc.transformer_forward on cat([prompt, line embeddings]) with the masked softmax of ``see`` [B, S, S]."""
    def forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                controlnet_block_samples=None, line_embeds=None, **unused):
        pe = torch.cat([encoder_hidden_states, line_embeds], dim=1)
        with lpr.attention_as(lpr.masked_attention(see[-hidden_states.shape[0]:])):
            return orc.transformer_forward(p, cfg, hidden_states, pe, pooled_projections, timestep, img_ids, torch.zeros(pe.shape[1], 3),
                                           guidance=guidance, controlnet_block_samples=controlnet_block_samples)
    return forward


def loop_slot(line_embeds, see):
    """denoise_loop_reference(image_prompt=): the forward above on the rows of ``see`` that belong to the batch it is called with."""
    def forward(p, cfg, hidden_states, *args, **kw):
        Bc = hidden_states.shape[0]
        le = line_embeds if Bc == line_embeds.shape[0] else torch.cat([line_embeds, line_embeds], dim=0)
        return forward_under(see)(p, cfg, hidden_states, *args, line_embeds=le, **kw)
    z = torch.zeros(line_embeds.shape[0], 1)
    return dict(forward=forward, ip_params=None, ip_scales=None, embeds=z, neg_embeds=z)


@pytest.fixture(scope="module")
def setup(gpu):
    """Weights, inputs and token masks shared by the reference tests; computed once, never modified."""
    tp, cp = reference_params()
    tr, pipe = models_on(gpu, tp, cp)
    g = torch.Generator().manual_seed(913)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    x = dict(pe=r(2, T, 256), pooled=r(2, 64), npe=(3 * r(2, T, 256)).to(torch.bfloat16).float(), npooled=(3 * r(2, 64)).to(torch.bfloat16).float(),
             lines=[(LINE_GAIN * r(2, L, 256)).to(torch.bfloat16).float() for _ in range(2)], lat=orc.pack_latents(r(2, 16, 32, 32)),
             hints=[r(2, N, 128), r(2, N, 128)])
    rms = [token_mask(b) for b in BOXES]
    assert float((rms[0] * rms[1]).abs().max()) == 0.0 and [int((m > 0).sum()) for m in rms] == [84, 84]
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    return dict(tp=tp, cp=cp, tr=tr, pipe=pipe, x=x, rms=rms, sig=sig, ids=orc.latent_image_ids(32, 32))


def forward_case(s):
    """(reference thunk of see, inputs) of one forward at B = 1."""
    x = s["x"]
    one = lambda t: t[:1]
    le = torch.cat([one(l) for l in x["lines"]], dim=1)
    ts, gd = torch.full((1,), 0.622459), torch.full((1,), 3.5)
    fwd = lambda see: forward_under(see)(s["tp"], SMALL_T, one(x["lat"]), one(x["pe"]), one(x["pooled"]), ts, s["ids"], None, guidance=gd,
                                         line_embeds=le)
    return fwd, le, ts, gd


# ------------------------------------------------------------------------------------------------------------------ 1. one forward
def test_transformer_forward_with_key_classes(setup, gpu, monkeypatch):
    import reptext_amd.ops as ops
    from reptext_amd import native

    s, x = setup, setup["x"]
    one = lambda t: t[:1]
    fwd, le, ts, gd = forward_case(s)
    vis, cls = tables(s["rms"])
    ref, ref16 = both(lambda: fwd(visible(vis, cls)))
    floor = rel_l2(ref16, ref)
    felt = rel_l2(fwd(visible(*tables(s["rms"], isolated=False))), ref)
    print(f"line isolation, one forward: bf16 floor {floor:.3e}; the non-isolated reference lies {felt:.3e} = {felt / floor:.1f} x floor away")
    assert felt > FELT * floor
    # the library's own rule gives the tables written out above
    from reptext_amd.pipeline import line_prompt_classes

    own = line_prompt_classes(T, L, s["rms"], N)
    assert torch.equal(own[0], vis) and torch.equal(own[1], cls)

    names = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    joint = torch.cat([one(x["pe"]), le], dim=1)
    out = s["tr"](hidden_states=b16(one(x["lat"]), gpu), encoder_hidden_states=b16(joint, gpu), pooled_projections=b16(one(x["pooled"]), gpu),
                  timestep=ts.to(gpu), img_ids=b16(s["ids"], gpu), txt_ids=torch.zeros(joint.shape[1], 3, device=gpu, dtype=torch.bfloat16),
                  guidance=gd.to(gpu), return_dict=False, _groups=ops.KeyClasses(vis, cls).to(gpu))[0].float().cpu()
    attn = [n for n in names if n.startswith("rt_attention")]
    assert attn == ["rt_attention_fwd_keyed"] * (SMALL_T["num_layers"] + SMALL_T["num_single_layers"])      # every joint attention
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line isolation, one forward: rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)


# ------------------------------------------------------------------------------------------------------------------ 2. the loop
def loop_case(s, B, cfg, per_image=False, isolated=True):
    """(positional arguments, keywords) of denoise_loop_reference for a 3-step loop with the text tower on two masked lines, and the masks."""
    x = s["x"]
    cut = lambda t: t[:B]
    if per_image:       # entry 1 takes the boxes the other way round
        rms = [torch.cat([token_mask(BOXES[0]), token_mask(BOXES[1])]), torch.cat([token_mask(BOXES[1]), token_mask(BOXES[0])])]
    else:
        rms = s["rms"]
    le = torch.cat([cut(l) for l in x["lines"]], dim=1)
    see = visible(*tables(rms if per_image else [m.expand(B, -1, -1) for m in rms], cfg=cfg, isolated=isolated))
    args = (s["tp"], SMALL_T, s["cp"], SMALL_CN, cut(x["lat"]), cut(x["pe"]), cut(x["pooled"]), [cut(h) for h in x["hints"]], rms, s["sig"], s["ids"],
            torch.zeros(T, 3), 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=2, image_prompt=loop_slot(le, see))
    if cfg:
        rkw["negative"] = dict(prompt_embeds=cut(x["npe"]), pooled=cut(x["npooled"]), scale=2.0)
    return args, rkw, rms


def pipe_call(s, gpu, B, cfg, rms, per_image):
    x = s["x"]
    cut = lambda t: b16(t[:B], gpu)
    kw = dict(prompt_embeds=cut(x["pe"]), pooled_prompt_embeds=cut(x["pooled"]), height=H, width=W, num_inference_steps=3, guidance_scale=3.5,
              control_image=[cut(h) for h in x["hints"]], control_mask=[b16(m, gpu) for m in rms] if per_image else mask_images(BOXES),
              controlnet_conditioning_scale=1.0, controlnet_conditioning_step=2, latents=cut(x["lat"]), output_type="latent",
              control_prompt_embeds=[cut(l) for l in x["lines"]], control_prompt_max_sequence_length=L, control_prompt_isolation=True)
    if cfg:
        kw.update(negative_prompt_embeds=cut(x["npe"]), negative_pooled_prompt_embeds=cut(x["npooled"]), true_cfg_scale=2.0)
    return kw


@pytest.mark.parametrize("B,cfg,interval", [(1, False, None), (1, True, None), (2, True, None), (1, True, (0.0, 0.67))])
def test_loop_matches_the_reference(setup, gpu, B, cfg, interval):
    """3 steps, the tower on two masked lines for 2 of them; plain, under true CFG, at B = 2 with per-image masks under true CFG (each
    sample also its own B = 1 call bit for bit), and with a guider whose interval ends after the second step: the third then runs on the
    positive half alone, on the [B:] view of both tables."""
    from reptext_amd.guidance import TrueCFGGuider

    s = setup
    per_image = B == 2
    args, rkw, rms = loop_case(s, B, cfg, per_image)
    guider = None if interval is None else TrueCFGGuider(start=interval[0], stop=interval[1])
    rkw["guider"] = guider
    ref, ref16 = both(lambda: denoise_loop_reference(*args, **rkw))
    floor = rel_l2(ref16, ref)
    if B == 1:
        plain = dict(rkw, image_prompt=loop_case(s, B, cfg, per_image, isolated=False)[1]["image_prompt"])
        felt = rel_l2(denoise_loop_reference(*args, **plain), ref)
        print(f"line isolation, loop B={B} cfg={cfg} interval={interval}: bf16 floor {floor:.3e}; the non-isolated reference lies {felt:.3e} = "
              f"{felt / floor:.1f} x floor away")
        assert felt > FELT * floor
    pipe = s["pipe"]
    pipe.capture_graphs = False
    pipe.guider = guider
    kw = pipe_call(s, gpu, B, cfg, rms, per_image)
    try:
        out = pipe(**kw).images.float().cpu()
    finally:
        pipe.guider = None
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line isolation, loop B={B} cfg={cfg}: latents rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)
    if B == 2:
        whole = pipe(**kw).images
        for b in range(2):
            one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if isinstance(v, list) else v) for k, v in kw.items()}
            assert torch.equal(pipe(**one).images, whole[b : b + 1]), b


# ------------------------------------------------------------------------------------------------------------------ 3. capture
def test_capture_and_replay_are_the_eager_bits(gpu):
    pipe, r = random_pipe(gpu, 921)
    kw = dict(two_line_call(r), control_mask=mask_images(BOXES))
    lkw = dict(kw, **line_kw(r))
    ikw = dict(lkw, control_prompt_isolation=True)
    fresh, _ = random_pipe(gpu, 921)
    fresh(**lkw)
    today = graph_keys(fresh)                                               # the key of the call without the argument, from a pipeline that never saw it
    pipe.capture_graphs = False
    grouped, eager = pipe(**lkw).images.clone(), pipe(**ikw).images.clone()
    assert not torch.equal(eager, grouped)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**ikw).images, eager)
    keys = graph_keys(pipe)
    assert len(keys) == 1 and isinstance(pipe._graph_cache[keys[0]], dict)
    tag = [e for e in keys[0] if isinstance(e, tuple) and e and e[0] in ("line_prompts", "line_isolation")]
    assert [e[0] for e in tag] == ["line_prompts", "line_isolation"]
    # other mask values of the same shape: the same graph, the tables copied in
    ikw2 = dict(ikw, control_mask=mask_images(OTHER_BOXES))
    pipe.capture_graphs = False
    eager2 = pipe(**ikw2).images.clone()
    pipe.capture_graphs = True
    assert torch.equal(pipe(**ikw2).images, eager2) and not torch.equal(eager2, eager) and graph_keys(pipe) == keys
    # the call without the argument, and with it False: the key it has today, which is not the isolated call's
    for _ in range(3):
        assert torch.equal(pipe(**lkw).images, grouped)
    assert torch.equal(pipe(**dict(lkw, control_prompt_isolation=False)).images, grouped)
    keys2 = graph_keys(pipe)
    assert len(keys2) == 2 and keys2[0] == keys[0] and "line_isolation" not in str(keys2[1])
    assert len(keys2[1]) == len(today[0]) and sum(a != b for a, b in zip(keys2[1], today[0])) == 1       # but for the models' identity
    assert len(keys[0]) == len(keys2[1]) + 1
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 4. toggles
def test_overlap_and_row_window_are_bitwise_neutral_with_isolation(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 931)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, steps=3, cn_steps=3), **line_kw(r), control_prompt_isolation=True)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    want = pipe(**kw).images.clone()
    assert pipe._tower_window_used is None
    for overlap, window in ((True, False), (False, True), (True, True)):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        monkeypatch.setattr(P, "TOWER_WINDOW", window)
        assert torch.equal(pipe(**kw).images, want), (overlap, window)
        assert (pipe._tower_window_used is not None) == window


# ------------------------------------------------------------------------------------------------------------------ 5. repaint
def test_repaint_with_isolated_line_prompts_keeps_the_source_outside_the_mask(gpu):
    """The repaint pipeline takes the line arguments and the isolation keyword: 3 steps at strength 1.0, the mask the union of the two
    boxes; tokens outside it end as the source's latents bit for bit, inside nothing does, and isolation changes the result."""
    import test_repaint_gpu as rp

    pipe, r = rp.random_pipe(gpu, 941)
    kw = dict(rp.two_line_call(r, steps=3, strength=1.0), control_mask=mask_images(BOXES), **line_kw(r))
    grouped = pipe(**kw).images.clone()
    out = pipe(**kw, control_prompt_isolation=True).images
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()) and not torch.equal(out, grouped)
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, gpu)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(out[mask == 0], kw["image"][mask == 0])
    assert not bool((out[mask == 1] == kw["image"][mask == 1]).any())
    assert_no_call_state(pipe)
