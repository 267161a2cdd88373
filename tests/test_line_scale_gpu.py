"""A strength per line prompt end to end on the GPU (``control_prompt_scale``): the transformer with ``_key_bias`` and the
pipelines' keyword against tests/line_scale_reference.py — the oracle's own forward and loop under ``line_prompt_reference``'s masked
softmax with ln w added to the logits of a line prompt's keys, at the same rounding points.

Model, weights, inputs, boxes and helpers are test_line_prompts_gpu.py's and test_line_isolation_gpu.py's: SMALL_T / SMALL_CN with the
``TEXT_V_GAIN`` text value projection, latents 32 x 32 (N = 256), T0 = 64, L = 64, two masked text lines with disjoint boxes of 84
tokens, S = 448; scales (2.0, 0.5). "The scales are felt" is a condition on the inputs, checked on the CPU with the references alone
before the GPU is involved: the scaled reference lies more than 4 x the bf16 floor from the unscaled one (each case prints its own
ratio).

What this file cannot see apart: the bias on a line's own TEXT rows (they weigh their own tokens by w_r too: the bias is per key). It is
in the reference as it is in the kernel, and pinned per element by test_attention_biased_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import H, N, T, W, graph_keys, random_pipe, token_mask, two_line_call  # noqa: E402
from test_true_cfg_host import _kw, _pipe, assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2, vae_pair  # noqa: E402,F401
from test_line_prompts_gpu import ENDS, L, LINE_GAIN, b16, both, line_kw, models_on, reference_params, table as group_table  # noqa: E402
from test_line_isolation_gpu import BOXES, S, pipe_call as isolated_call, tables as class_tables, visible as class_visible  # noqa: E402

import line_prompt_reference as lpr  # noqa: E402
import line_scale_reference as lsr  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (2.0, 0.5)
FELT = 4.0
RULES = ["grouped", "keyed"]


def see_under(rule, masks, cfg=False):
    """bool [B or 2B, S, S] of the rule's tables for two lines with prompts."""
    if rule == "keyed":
        return class_visible(*class_tables(masks, cfg=cfg))
    return lpr.visible(ENDS, group_table(masks, cfg=cfg))


def device_tables(rule, masks, gpu):
    import reptext_amd.ops as ops

    if rule == "keyed":
        return ops.KeyClasses(*class_tables(masks)).to(gpu)
    return ops.KeyGroups(ENDS, group_table(masks).to(gpu))


@pytest.fixture(scope="module")
def setup(gpu):
    """Weights, inputs and token masks shared by the reference tests; computed once, never modified."""
    tp, cp = reference_params()
    tr, pipe = models_on(gpu, tp, cp)
    g = torch.Generator().manual_seed(1013)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    x = dict(pe=r(1, T, 256), pooled=r(1, 64), npe=(3 * r(1, T, 256)).to(torch.bfloat16).float(), npooled=(3 * r(1, 64)).to(torch.bfloat16).float(),
             lines=[(LINE_GAIN * r(1, L, 256)).to(torch.bfloat16).float() for _ in range(2)], lat=orc.pack_latents(r(1, 16, 32, 32)),
             hints=[r(1, N, 128), r(1, N, 128)])
    rms = [token_mask(b) for b in BOXES]
    assert float((rms[0] * rms[1]).abs().max()) == 0.0 and [int((m > 0).sum()) for m in rms] == [84, 84]
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    bias = lsr.key_log_scale(T, L, SCALES, S)
    assert bias[:T].abs().max() == 0 and bias[T + 2 * L :].abs().max() == 0 and float(bias[T]) == np.float32(np.log(2.0)) and float(bias[T + L]) < 0
    return dict(tp=tp, cp=cp, tr=tr, pipe=pipe, x=x, rms=rms, sig=sig, ids=orc.latent_image_ids(32, 32), bias=bias, zero=torch.zeros(S))


# ------------------------------------------------------------------------------------------------------------------ 1. one forward
@pytest.mark.parametrize("rule", RULES)
def test_transformer_forward_with_a_key_bias(setup, gpu, monkeypatch, rule):
    from reptext_amd import native
    from reptext_amd.pipeline import line_prompt_bias

    s, x = setup, setup["x"]
    le = torch.cat(x["lines"], dim=1)
    ts, gd = torch.full((1,), 0.622459), torch.full((1,), 3.5)
    see = see_under(rule, s["rms"])
    fwd = lambda bias: lsr.forward_under(see, bias)(s["tp"], SMALL_T, x["lat"], x["pe"], x["pooled"], ts, s["ids"], None, guidance=gd, line_embeds=le)
    # the library's own rule gives the reference's restated bias: its table, looked up by the class of every key under this rule
    key_class = class_tables(s["rms"])[1][0].long() if rule == "keyed" else torch.bucketize(torch.arange(S), torch.tensor(ENDS), right=True)
    assert torch.equal(line_prompt_bias(SCALES, [True, True])[0][key_class], s["bias"])
    ref, ref16 = both(lambda: fwd(s["bias"]))
    floor = rel_l2(ref16, ref)
    felt = rel_l2(fwd(s["zero"]), ref)
    print(f"line scales {SCALES}, one forward, {rule}: bf16 floor {floor:.3e}; the unscaled reference lies {felt:.3e} = {felt / floor:.1f} x floor away")
    assert felt > FELT * floor

    names = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    joint = torch.cat([x["pe"], le], dim=1)
    out = s["tr"](hidden_states=b16(x["lat"], gpu), encoder_hidden_states=b16(joint, gpu), pooled_projections=b16(x["pooled"], gpu),
                  timestep=ts.to(gpu), img_ids=b16(s["ids"], gpu), txt_ids=torch.zeros(joint.shape[1], 3, device=gpu, dtype=torch.bfloat16),
                  guidance=gd.to(gpu), return_dict=False, _groups=device_tables(rule, s["rms"], gpu),
                  _key_bias=line_prompt_bias(SCALES, [True, True]).to(gpu))[0].float().cpu()
    attn = [n for n in names if n.startswith("rt_attention")]
    assert attn == [f"rt_attention_fwd_{rule}_biased"] * (SMALL_T["num_layers"] + SMALL_T["num_single_layers"])      # every joint attention
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line scales, one forward, {rule}: rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)


# ------------------------------------------------------------------------------------------------------------------ 2. the loop
def loop_case(s, rule, cfg, bias):
    """(positional arguments, keywords) of denoise_loop_reference for a 3-step loop with the text tower on two masked lines at B = 1."""
    x = s["x"]
    le = torch.cat(x["lines"], dim=1)
    args = (s["tp"], SMALL_T, s["cp"], SMALL_CN, x["lat"], x["pe"], x["pooled"], x["hints"], s["rms"], s["sig"], s["ids"], torch.zeros(T, 3), 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=2, image_prompt=lsr.loop_slot(le, see_under(rule, s["rms"], cfg=cfg), bias))
    if cfg:
        rkw["negative"] = dict(prompt_embeds=x["npe"], pooled=x["npooled"], scale=2.0)
    return args, rkw


def pipe_call(s, gpu, rule, cfg, **more):
    kw = isolated_call(s, gpu, 1, cfg, s["rms"], False)
    if rule == "grouped":
        del kw["control_prompt_isolation"]
    return dict(kw, **more)


@pytest.mark.parametrize("rule,cfg,interval", [("grouped", False, None), ("keyed", False, None), ("grouped", True, None), ("keyed", True, (0.0, 0.67))])
def test_loop_matches_the_reference(setup, gpu, rule, cfg, interval):
    """3 steps at B = 1, the tower on two masked lines for 2 of them: plain under either rule, under true CFG, and with a guider whose
    interval ends after the second step — the third then runs on the positive half alone, with the same [1, 32] table."""
    from reptext_amd.guidance import TrueCFGGuider

    s = setup
    args, rkw = loop_case(s, rule, cfg, s["bias"])
    guider = None if interval is None else TrueCFGGuider(start=interval[0], stop=interval[1])
    rkw["guider"] = guider
    ref, ref16 = both(lambda: denoise_loop_reference(*args, **rkw))
    floor = rel_l2(ref16, ref)
    unscaled = dict(rkw, image_prompt=loop_case(s, rule, cfg, s["zero"])[1]["image_prompt"])
    felt = rel_l2(denoise_loop_reference(*args, **unscaled), ref)
    print(f"line scales, loop {rule} cfg={cfg} interval={interval}: bf16 floor {floor:.3e}; the unscaled reference lies {felt:.3e} = "
          f"{felt / floor:.1f} x floor away")
    assert felt > FELT * floor
    pipe = s["pipe"]
    pipe.capture_graphs = False
    pipe.guider = guider
    try:
        out = pipe(**pipe_call(s, gpu, rule, cfg, control_prompt_scale=list(SCALES))).images.float().cpu()
    finally:
        pipe.guider = None
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"line scales, loop {rule} cfg={cfg} interval={interval}: latents rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage "
          f"reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("rule", RULES)
def test_scale_one_is_the_call_without_the_keyword_through_the_biased_launch(gpu, monkeypatch, rule):
    from reptext_amd import native

    pipe, r = random_pipe(gpu, 1021)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r), **line_kw(r), **(dict(control_prompt_isolation=True) if rule == "keyed" else {}))
    names = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    want = pipe(**kw).images.clone()
    blocks = SMALL_T["num_layers"] + SMALL_T["num_single_layers"]
    joint = lambda: [n for n in names if n.startswith(("rt_attention_fwd_grouped", "rt_attention_fwd_keyed"))]
    assert joint() == [f"rt_attention_fwd_{rule}"] * (3 * blocks)
    for scale in (1.0, [1.0, None], [None, None]):
        names.clear()
        assert torch.equal(pipe(**kw, control_prompt_scale=scale).images, want), scale
        assert joint() == [f"rt_attention_fwd_{rule}_biased"] * (3 * blocks)         # named: the biased launch, in every joint attention
    names.clear()
    assert not torch.equal(pipe(**kw, control_prompt_scale=[4.0, 0.25]).images, want)
    assert torch.equal(pipe(**kw, control_prompt_scale=None).images, want) and joint()[-1] == f"rt_attention_fwd_{rule}"      # None names nothing
    assert_no_call_state(pipe)


@pytest.mark.parametrize("rule", RULES)
def test_capture_and_replay_are_the_eager_bits_and_new_scales_replay_the_graph(gpu, rule):
    pipe, r = random_pipe(gpu, 1031)
    kw = dict(two_line_call(r), **line_kw(r), **(dict(control_prompt_isolation=True) if rule == "keyed" else {}))
    pipe.capture_graphs = False
    plain = pipe(**kw).images.clone()
    eager = pipe(**kw, control_prompt_scale=[2.0, 0.5]).images.clone()
    eager2 = pipe(**kw, control_prompt_scale=[0.25, 3.0]).images.clone()
    assert not torch.equal(eager, plain) and not torch.equal(eager2, eager)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw, control_prompt_scale=[2.0, 0.5]).images, eager)
    keys = graph_keys(pipe)
    assert len(keys) == 1 and isinstance(pipe._graph_cache[keys[0]], dict)
    tag = [e for e in keys[0] if isinstance(e, tuple) and e and e[0] == "line_scale"]
    assert len(tag) == 1 and tag[0][1][0] == (1, 32) and keys[0][-1] == tag[0]
    graph = pipe._graph_cache[keys[0]]
    # other scale values: the same key, the same captured graph, the table copied in
    assert torch.equal(pipe(**kw, control_prompt_scale=[0.25, 3.0]).images, eager2)
    assert graph_keys(pipe) == keys and pipe._graph_cache[keys[0]] is graph
    assert torch.equal(pipe(**kw, control_prompt_scale=[2.0, 0.5]).images, eager) and graph_keys(pipe) == keys
    # the call without the keyword: its own key, without the marker, and its old bits
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, plain)
    keys2 = graph_keys(pipe)
    assert len(keys2) == 2 and keys2[0] == keys[0] and "line_scale" not in str(keys2[1]) and keys2[1] == keys[0][:-1]
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 4. the other pipelines
def test_repaint_with_line_scales_keeps_the_source_outside_the_mask(gpu):
    """3 steps at strength 1.0 through the repaint pipeline: the scales change the result under the mask; tokens outside it end as the
    source, bit for bit."""
    import test_repaint_gpu as rp

    pipe, r = rp.random_pipe(gpu, 1041)
    kw = dict(rp.two_line_call(r, steps=3, strength=1.0), **line_kw(r))
    plain = pipe(**kw).images.clone()
    out = pipe(**kw, control_prompt_scale=[4.0, 0.25]).images
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), rp.H, rp.W, gpu)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(out[mask == 0], kw["image"][mask == 0])
    assert not bool((out[mask == 1] == kw["image"][mask == 1]).any())
    assert not torch.equal(out[mask == 1], plain[mask == 1])
    assert torch.equal(pipe(**kw, control_prompt_scale=1.0).images, plain)
    assert_no_call_state(pipe)


def test_photo_with_a_line_prompt_and_its_scale(vae_pair, gpu):
    """The photo pipeline takes the line keywords through the shared call: the result has the photo's size, the photo's bytes farther
    than the feather's radius from the mask, other bytes inside it than the call without the scale gives, and scale 1.0 gives that call's."""
    import test_photo_pipeline_gpu as ph

    _, vae = vae_pair
    pipe, r = ph.photo_pipe(gpu, 1051, vae)
    pipe.capture_graphs = False
    photo = ph.random_photo(11)
    kw = dict(ph.photo_call(r, photo), control_prompt_embeds=[LINE_GAIN * r(1, L, 256)], control_prompt_max_sequence_length=L, output_type="pil")
    plain = np.array(ph.photo_run(pipe, kw)[0])
    out = ph.photo_run(pipe, kw, control_prompt_scale=[8.0])
    assert len(out) == 1 and out[0].size == (ph.PW, ph.PH) and out[0].mode == "RGB"
    got = np.array(out[0])
    dist, depth = ph.distance_to_box(ph.BOX, ph.PH, ph.PW)
    assert np.array_equal(got[dist > ph.R], photo[dist > ph.R]) and np.array_equal(plain[dist > ph.R], photo[dist > ph.R])
    assert float((got[depth > 0] != photo[depth > 0]).mean()) > 0.9 and not np.array_equal(got[depth > 0], plain[depth > 0])
    assert np.array_equal(np.array(ph.photo_run(pipe, kw, control_prompt_scale=1.0)[0]), plain)
    ph.no_photo_left(pipe, photo)


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    pipe, r = random_pipe(gpu, 1061)
    kw = dict(two_line_call(r), **line_kw(r))
    pipe.transformer.enable_fp8_attention(True)
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**kw, control_prompt_scale=2.0)
    pipe.transformer.enable_fp8_attention(False)
    assert pipe(**kw, control_prompt_scale=2.0).images.shape == (1, N, 64)
    with pytest.raises(ValueError, match="needs a per-line prompt"):
        pipe(**two_line_call(r), control_prompt_scale=2.0)
    with pytest.raises(ValueError, match="per text line"):
        pipe(**kw, control_prompt_scale=[2.0])
    with pytest.raises(ValueError, match=r"\[1/64, 64\]"):
        pipe(**kw, control_prompt_scale=[2.0, 65.0])
    with pytest.raises(ValueError, match="without a prompt cannot have a scale"):
        pipe(**dict(kw, control_prompt_embeds=[kw["control_prompt_embeds"][0], None]), control_prompt_scale=[2.0, 2.0])
    with pytest.raises(ValueError, match="control_mask"):
        pipe(**dict(kw, control_mask=None), control_prompt_scale=2.0)
    with pytest.raises(ValueError, match=r"inpaint pipeline does not support per-line prompts \(control_prompt_scale\)"):
        _pipe(inpaint=True)(**_kw(), control_prompt_scale=2.0)
    assert_no_call_state(pipe)
