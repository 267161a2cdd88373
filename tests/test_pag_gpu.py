"""Perturbed-attention guidance end to end on the GPU (``pag_scale`` / ``pag_applied_layers``): the transformer with
``_perturbed`` and the pipelines' keywords against tests/pag_reference.py — the oracle's own forward and the loop of
tests/loop_reference.py with the masked softmax in the applied blocks of the perturbed half only, at the same rounding points.

Model, weights and helpers are the sibling files': SMALL_T / SMALL_CN with test_line_prompts_gpu.py's ``TEXT_V_GAIN`` text value
projection, latents 32 x 32 (N = 256), T = 64, S = 320, two masked text lines, 3 steps with the tower on for 2. Applied layers:
``transformer_blocks.1`` and ``single_transformer_blocks.0``; pag_scale 3.0. Two conditions on the inputs are checked on the CPU with the
references alone before the GPU is involved (each case prints its ratios): the perturbed reference lies more than 4 x the bf16 floor
from the unperturbed one, and so does the reference with the layer set moved by one block — so a launch that perturbs nothing, or the
wrong blocks, cannot pass.

What this file cannot see apart: which key of the image class a perturbed image row keeps (its own). That is pinned per element by
test_attention_self_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import BOXES, H, N, T, W, graph_keys, mask_images, negatives, random_pipe, token_mask, two_line_call  # noqa: E402,F401
from test_true_cfg_host import _kw, _pipe, assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2  # noqa: E402
from test_line_prompts_gpu import b16, both, models_on, reference_params  # noqa: E402

import pag_reference as pgr  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

pytestmark = pytest.mark.gpu

LAYERS = ["transformer_blocks.1", "single_transformer_blocks.0"]
DOUBLE, SINGLE = {1}, {0}
MOVED = ({0}, {1})                  # the layer set moved by one block
PAG_SCALE = 3.0
FELT = 4.0
PAG = dict(pag_scale=PAG_SCALE, pag_applied_layers=LAYERS)
BLOCKS = SMALL_T["num_layers"] + SMALL_T["num_single_layers"]


def make_inputs():
    """Weights and inputs of the reference tests (CPU); computed once, never modified."""
    tp, cp = reference_params()
    g = torch.Generator().manual_seed(1113)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    x = dict(pe=r(1, T, 256), pooled=r(1, 64), lat=orc.pack_latents(r(1, 16, 32, 32)), hints=[r(1, N, 128), r(1, N, 128)])
    rms = [token_mask(b) for b in BOXES]
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    return dict(tp=tp, cp=cp, x=x, rms=rms, sig=sig, ids=orc.latent_image_ids(32, 32))


@pytest.fixture(scope="module")
def setup(gpu):
    s = make_inputs()
    s["tr"], s["pipe"] = models_on(gpu, s["tp"], s["cp"])
    return s


def forward_reference(s, double_ids, single_ids):
    """The transformer at batch 2 = [perturbed, positive] of the same conditioning."""
    x = s["x"]
    two = lambda t: torch.cat([t, t], dim=0)
    ts, gd = torch.full((2,), 0.622459), torch.full((2,), 3.5)
    return pgr.forward_under(T, double_ids, single_ids)(s["tp"], SMALL_T, two(x["lat"]), two(x["pe"]), two(x["pooled"]), ts, s["ids"],
                                                       torch.zeros(T, 3), guidance=gd)


def loop_reference_of(s, double_ids, single_ids, guider=None, pag=True):
    x = s["x"]
    args = (s["tp"], SMALL_T, s["cp"], SMALL_CN, x["lat"], x["pe"], x["pooled"], x["hints"], s["rms"], s["sig"], s["ids"], torch.zeros(T, 3), 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=2)
    if pag:
        rkw.update(negative=pgr.negative_slot(x["pe"], x["pooled"], PAG_SCALE), image_prompt=pgr.loop_slot(1, T, double_ids, single_ids), guider=guider)
    return denoise_loop_reference(*args, **rkw)


def felt(what, ref, floor, unperturbed, moved):
    a, b = rel_l2(unperturbed, ref), rel_l2(moved, ref)
    print(f"PAG, {what}: bf16 floor {floor:.3e}; the unperturbed reference lies {a:.3e} = {a / floor:.1f} x floor away, the reference with the "
          f"layer set moved by one block {b:.3e} = {b / floor:.1f} x floor")
    assert a > FELT * floor and b > FELT * floor


def pipe_call(s, gpu, **more):
    x = s["x"]
    return dict(prompt_embeds=b16(x["pe"], gpu), pooled_prompt_embeds=b16(x["pooled"], gpu), height=H, width=W, num_inference_steps=3,
                guidance_scale=3.5, control_image=[b16(h, gpu) for h in x["hints"]], control_mask=mask_images(BOXES),
                controlnet_conditioning_step=2, latents=b16(x["lat"], gpu), output_type="latent", **more)


# ------------------------------------------------------------------------------------------------------------------ 1. one forward
def test_transformer_forward_at_batch_two(setup, gpu, monkeypatch):
    from reptext_amd import native
    from reptext_amd.pipeline import Perturbed, perturbed_attention_tables

    s, x = setup, setup["x"]
    ref, ref16 = both(lambda: forward_reference(s, DOUBLE, SINGLE))
    floor = rel_l2(ref16, ref)
    felt("one forward", ref, floor, forward_reference(s, set(), set()), forward_reference(s, *MOVED))
    assert torch.equal(ref[1], forward_reference(s, set(), set())[1])                    # the positive half is the unperturbed forward

    names = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    row_vis, key_class = perturbed_attention_tables(T, N, 1)
    rec = Perturbed(row_vis.to(gpu), key_class.to(gpu), frozenset(DOUBLE), frozenset(SINGLE))
    two = lambda t: torch.cat([t, t], dim=0)
    out = s["tr"](hidden_states=b16(two(x["lat"]), gpu), encoder_hidden_states=b16(two(x["pe"]), gpu), pooled_projections=b16(two(x["pooled"]), gpu),
                  timestep=torch.full((2,), 0.622459, device=gpu), img_ids=b16(s["ids"], gpu), txt_ids=torch.zeros(T, 3, device=gpu, dtype=torch.bfloat16),
                  guidance=torch.full((2,), 3.5, device=gpu), return_dict=False, _perturbed=rec)[0].float().cpu()
    attn = [n for n in names if n.startswith("rt_attention_fwd")]
    assert len(attn) == BLOCKS and [i for i, n in enumerate(attn) if n == "rt_attention_fwd_keyed_self"] == [1, SMALL_T["num_layers"]]
    assert not any("keyed" in n or "grouped" in n for i, n in enumerate(attn) if i not in (1, SMALL_T["num_layers"]))
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"PAG, one forward: rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    e0, e1 = rel_l2(out[0], ref[0]), rel_l2(out[1], ref[1])
    print(f"PAG, one forward: perturbed half {e0:.3e}, positive half {e1:.3e}")
    with pytest.raises(ValueError, match="_perturbed and _groups"):
        s["tr"](hidden_states=b16(two(x["lat"]), gpu), encoder_hidden_states=b16(two(x["pe"]), gpu), pooled_projections=b16(two(x["pooled"]), gpu),
                timestep=torch.full((2,), 0.622459, device=gpu), img_ids=b16(s["ids"], gpu), txt_ids=torch.zeros(T, 3, device=gpu, dtype=torch.bfloat16),
                guidance=torch.full((2,), 3.5, device=gpu), return_dict=False, _perturbed=rec, _groups=rec.groups())


# ------------------------------------------------------------------------------------------------------------------ 2. the loop
@pytest.mark.parametrize("interval", [None, (0.0, 0.67)])
def test_loop_matches_the_reference(setup, gpu, interval):
    """3 steps at B = 1, the tower on two masked lines for 2 of them: PAG alone, and with a guider whose interval ends after the second
    step — the third then runs on the positive half alone, at batch 1, without tables."""
    from reptext_amd.guidance import TrueCFGGuider

    s = setup
    guider = None if interval is None else TrueCFGGuider(start=interval[0], stop=interval[1])
    ref, ref16 = both(lambda: loop_reference_of(s, DOUBLE, SINGLE, guider))
    floor = rel_l2(ref16, ref)
    felt(f"loop interval={interval}", ref, floor, loop_reference_of(s, DOUBLE, SINGLE, pag=False), loop_reference_of(s, *MOVED, guider))
    pipe = s["pipe"]
    pipe.capture_graphs = False
    pipe.guider = guider
    try:
        out = pipe(**pipe_call(s, gpu, **PAG)).images.float().cpu()
    finally:
        pipe.guider = None
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"PAG, loop interval={interval}: latents rel-L2 {err:.3e} vs fp32 reference, {err16:.3e} vs bf16-storage reference (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 3. bits
def test_launches_and_the_calls_that_are_the_plain_call(gpu, monkeypatch):
    """The applied blocks alone take the self launch, at guided steps alone; pag_scale 0, and a guider with an empty interval, give the
    plain call bit for bit (the latter through the positive half at batch B, without a table in any block)."""
    from reptext_amd import native
    from reptext_amd.guidance import TrueCFGGuider

    pipe, r = random_pipe(gpu, 1121)
    pipe.capture_graphs = False
    kw = two_line_call(r)
    names = []
    call = native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    selfs = lambda: sum(n == "rt_attention_fwd_keyed_self" for n in names)
    masked = lambda: sum(n.startswith(("rt_attention_fwd_keyed", "rt_attention_fwd_grouped")) for n in names)
    want = pipe(**kw).images.clone()
    assert masked() == 0
    names.clear()
    out = pipe(**kw, **PAG).images
    assert not torch.equal(out, want) and selfs() == 3 * len(LAYERS) == masked()
    names.clear()
    assert torch.equal(pipe(**kw, pag_scale=0.0, pag_applied_layers=LAYERS).images, want) and masked() == 0
    pipe.guider = TrueCFGGuider(start=0.9, stop=0.95)                       # no step of three lies inside
    try:
        assert torch.equal(pipe(**kw, **PAG).images, want) and masked() == 0
        names.clear()
        pipe.guider = TrueCFGGuider(start=0.0, stop=0.67)
        assert not torch.equal(pipe(**kw, **PAG).images, want) and selfs() == 2 * len(LAYERS) == masked()
    finally:
        pipe.guider = None
    assert_no_call_state(pipe)


def test_capture_and_replay_are_the_eager_bits(gpu):
    pipe, r = random_pipe(gpu, 1131)
    kw = two_line_call(r)
    pipe.capture_graphs = False
    plain = pipe(**kw).images.clone()
    eager = pipe(**kw, **PAG).images.clone()
    assert not torch.equal(eager, plain)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw, **PAG).images, eager)
    keys = graph_keys(pipe)
    assert len(keys) == 1 and isinstance(pipe._graph_cache[keys[0]], dict)
    tag = [e for e in keys[0] if isinstance(e, tuple) and e and e[0] == "pag"]
    assert len(tag) == 1 and keys[0][-1] == tag[0] and tag[0][1] == ("transformer_blocks.1", "single_transformer_blocks.0")
    assert ("cfg", 1.0 + PAG_SCALE) in keys[0]
    # the call without the keywords: its own key, without the markers, and its old bits
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, plain)
    keys2 = graph_keys(pipe)
    assert len(keys2) == 2 and keys2[0] == keys[0] and "pag" not in str(keys2[1]) and "cfg" not in str(keys2[1])
    # another layer set is another graph
    assert not torch.equal(pipe(**kw, pag_scale=PAG_SCALE, pag_applied_layers=["transformer_blocks.0"]).images, eager)
    keys3 = graph_keys(pipe)                                                # the pipeline keeps two graphs: the oldest key made room
    assert keys3[-1] not in keys2 and keys3[-1][-1][1] == ("transformer_blocks.0",) and keys3[-1][:-1] == keys[0][:-1]
    assert_no_call_state(pipe)


def test_batch_two_is_two_calls_at_batch_one(gpu):
    pipe, r = random_pipe(gpu, 1141)
    pipe.capture_graphs = False
    kw = two_line_call(r, B=2)
    out = pipe(**kw, **PAG).images
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k == "control_image" else v) for k, v in kw.items()}
        assert torch.equal(pipe(**one, **PAG).images[0], out[b]), b
    assert_no_call_state(pipe)


def test_overlap_and_row_window_are_bitwise_neutral(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 1151)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, steps=3, cn_steps=3), **PAG)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    want = pipe(**kw).images.clone()
    assert pipe._tower_window_used is None
    for overlap, window in ((True, False), (False, True), (True, True)):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        monkeypatch.setattr(P, "TOWER_WINDOW", window)
        assert torch.equal(pipe(**kw).images, want), (overlap, window)
        assert (pipe._tower_window_used is not None) == window


# ------------------------------------------------------------------------------------------------------------------ 4. repaint
def test_repaint_with_pag_keeps_the_source_outside_the_mask(gpu):
    """3 steps at strength 1.0 through the repaint pipeline: PAG changes the result under the mask; tokens outside it end as the source,
    bit for bit."""
    import test_repaint_gpu as rp

    pipe, r = rp.random_pipe(gpu, 1161)
    kw = rp.two_line_call(r, steps=3, strength=1.0)
    plain = pipe(**kw).images.clone()
    out = pipe(**kw, **PAG).images
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), rp.H, rp.W, gpu)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(out[mask == 0], kw["image"][mask == 0])
    assert not bool((out[mask == 1] == kw["image"][mask == 1]).any())
    assert not torch.equal(out[mask == 1], plain[mask == 1])
    assert torch.equal(pipe(**kw, pag_scale=0.0).images, plain)
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    pipe, r = random_pipe(gpu, 1171)
    kw = two_line_call(r)
    pipe.transformer.enable_fp8_attention(True)
    with pytest.raises(ValueError, match="enable_fp8_attention"):
        pipe(**kw, **PAG)
    pipe.transformer.enable_fp8_attention(False)
    assert pipe(**kw, **PAG).images.shape == (1, N, 64)
    with pytest.raises(ValueError, match="needs pag_applied_layers"):
        pipe(**kw, pag_scale=3.0)
    with pytest.raises(ValueError, match="out of range"):
        pipe(**kw, pag_scale=3.0, pag_applied_layers=["transformer_blocks.2"])
    with pytest.raises(ValueError, match="negative prompt"):
        pipe(**kw, **PAG, **negatives(r), true_cfg_scale=2.0)
    with pytest.raises(ValueError, match=r"inpaint pipeline does not support perturbed-attention guidance"):
        _pipe(inpaint=True)(**_kw(), **PAG)
    assert_no_call_state(pipe)
