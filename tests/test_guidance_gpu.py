"""A guider on a true-CFG call (``pipe.guider``, reptext_amd/guidance.py) on the GPU: parity of the loop with the CPU oracle's
(tests/loop_reference.py) for a guidance interval, projected guidance and both under the multistep scheduler; off means off; an
empty interval is the plain call; eager = captured = replay; batch invariance and the loop's toggles; one call each with a repaint,
the union tower, an image prompt and the fp8 modes; the refusal of the inpaint pipeline and the momentum after a callback.
256x256 (N = 256, T = 64) with the reduced models of test_vae_pipeline_gpu.py, 4 steps, s = 2.0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import BOXES, graph_keys, negatives, random_pipe, token_mask, two_line_call  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2  # noqa: E402

import ip_adapter_reference as ipr  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

H = W = 256
N, T, E = 256, 64, 64
STEPS = 4
_SHARED = {}
# Chosen on the CPU reference alone, before any GPU run, so that every guided result lies more than 20 bf16-storage floors from the
# plain-CFG result and from the plain result (floors away, [interval, projected, both] as (from CFG, from plain)): seeds 911.. with the
# negatives three times as large gave (25, 16), (18, 18), (43, 25) — not felt enough; these give (43, 28), (30, 31), (66, 26).
SEED, NEG_SCALE = 921, 4


def guider(**kw):
    from reptext_amd.guidance import TrueCFGGuider

    return TrueCFGGuider(**kw)


def call_without_negatives(kw):
    return {k: v for k, v in kw.items() if "negative" not in k and k != "true_cfg_scale"}


def cfg_call(r, **kw):
    return dict(two_line_call(r, steps=STEPS, **kw), **negatives(r, B=kw.get("B", 1)), true_cfg_scale=2.0)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
def parity_setup():
    """Parameters, inputs and the three references that every parity case shares (fp32 and bf16-storage): the plain loop, the CFG
    loop, and ‖d‖ of the first guided step, which sets the clamp. Computed once."""
    if _SHARED:
        return _SHARED
    tp = orc.init_mmdit_params(SMALL_T, seed=SEED)
    cp = orc.init_mmdit_params(SMALL_CN, seed=SEED + 1, controlnet=True)
    g = torch.Generator().manual_seed(SEED + 2)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    pe, pooled, npe, npooled, hint = r(1, T, 256), r(1, 64), r(1, T, 256), r(1, 64), r(1, N, 128)
    # the negative half must be felt (test_true_cfg_gpu.py draws it three times as large): NEG_SCALE times as large
    npe, npooled = (NEG_SCALE * npe).to(torch.bfloat16).float(), (NEG_SCALE * npooled).to(torch.bfloat16).float()
    lat0 = orc.pack_latents(r(1, 16, 32, 32))
    box = (60, 140, 80, 200)
    sig = orc.flow_sigmas(STEPS, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    ids = orc.latent_image_ids(32, 32)
    args = (tp, SMALL_T, cp, SMALL_CN, lat0, pe, pooled, [hint], [token_mask(box)], sig, ids, torch.zeros(T, 3), 3.5)
    neg = dict(prompt_embeds=npe, pooled=npooled, scale=2.0)
    info = {}                                                       # one step: its d is the plain CFG difference
    denoise_loop_reference(*args[:9], sig[:2], *args[10:], negative=neg, guider=guider(eta=0.0), info=info)
    plain_cfg = denoise_loop_reference(*args, negative=neg)
    plain = orc.denoise_loop(*args)
    _SHARED.update(tp=tp, cp=cp, args=args, neg=neg, box=box, norm_d0=float(info["norm_d"][0]), plain_cfg=plain_cfg, plain=plain,
                   inputs=dict(pe=pe, pooled=pooled, npe=npe, npooled=npooled, hint=hint, lat0=lat0))
    return _SHARED


@pytest.mark.parametrize("case", ["interval", "projected", "both_multistep"])
def test_guided_loop_matches_the_oracle_loop(gpu, case):
    """interval: (0, 0.5) with the plain mix; projected: (0, 1) with η = 0, momentum −0.5 and the clamp at half the ‖d‖ the reference
    shows at step 0 (active); both_multistep: the interval and the projection under the second-order scheduler. The GPU error sits at
    the bf16-storage oracle's own floor, and — a condition on the inputs, asserted on the CPU reference alone — the guided result lies
    more than 20 floors from the plain-CFG result and from the plain result."""
    from PIL import Image

    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    S = parity_setup()
    tau = 0.5 * S["norm_d0"]
    gd = {"interval": guider(stop=0.5), "projected": guider(eta=0.0, momentum=-0.5, norm_threshold=tau),
          "both_multistep": guider(stop=0.5, eta=0.0, momentum=-0.5, norm_threshold=tau)}[case]
    order = 2 if case == "both_multistep" else 1
    ref = denoise_loop_reference(*S["args"], negative=S["neg"], guider=gd, order=order)
    with orc.stored_as(torch.bfloat16):
        ref16 = denoise_loop_reference(*S["args"], negative=S["neg"], guider=gd, order=order)
    floor = rel_l2(ref16, ref)
    felt_cfg, felt_plain = rel_l2(S["plain_cfg"], ref), rel_l2(S["plain"], ref)
    print(f"guided [{case}] floor {floor:.3e}; the plain-CFG loop lies {felt_cfg / floor:.0f} floors away, the plain loop {felt_plain / floor:.0f}")
    assert felt_cfg > 20 * floor and felt_plain > 20 * floor

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(S["tp"]); cn.load_state_dict(S["cp"])
    sched = FlowMatchMultistepScheduler() if order == 2 else FlowMatchEulerDiscreteScheduler()
    pipe = FluxControlNetPipeline(sched, None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    pipe.guider = gd
    i = S["inputs"]
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    box = S["box"]
    mask_np = np.zeros([H, W], dtype=np.uint8)
    mask_np[box[0]:box[1], box[2]:box[3]] = 255
    out = pipe(prompt_embeds=b16(i["pe"]), pooled_prompt_embeds=b16(i["pooled"]), negative_prompt_embeds=b16(i["npe"]),
               negative_pooled_prompt_embeds=b16(i["npooled"]), true_cfg_scale=2.0, height=H, width=W, num_inference_steps=STEPS, guidance_scale=3.5,
               control_image=[b16(i["hint"])], control_mask=[Image.fromarray(mask_np)], controlnet_conditioning_scale=1.0,
               controlnet_conditioning_step=30, latents=b16(i["lat0"]), output_type="latent").images.float().cpu()
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"guided [{case}] latents rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e})")
    assert_at_dtype_floor(err, err16, floor)


# ------------------------------------------------------------------------------------------------------------------ 2. off means off
def test_off_means_off(gpu):
    """guider=None, a default guider, a guider on a call without a negative prompt and one on a call with true_cfg_scale=1: the graph
    cache holds the one key the call builds without a guider, and the latents are its bits."""
    pipe, r = random_pipe(gpu, 921)
    kw = cfg_call(r)
    want = pipe(**kw).images.clone()
    keys = graph_keys(pipe)
    assert len(keys) == 1 and not any(isinstance(k, tuple) and k and k[0] == "guidance" for k in keys[0])
    for g in (None, guider()):
        pipe.guider = g
        assert torch.equal(pipe(**kw).images, want) and graph_keys(pipe) == keys
    pipe2, r2 = random_pipe(gpu, 922)
    kw2 = two_line_call(r2, steps=STEPS)
    want2 = pipe2(**kw2).images.clone()
    keys2 = graph_keys(pipe2)
    pipe2.guider = guider(stop=0.5, eta=0.0, momentum=-0.5, norm_threshold=1.0)
    assert torch.equal(pipe2(**kw2).images, want2) and graph_keys(pipe2) == keys2                       # no negative prompt
    assert torch.equal(pipe2(**kw2, **negatives(r2), true_cfg_scale=1.0).images, want2) and graph_keys(pipe2) == keys2
    pipe2.capture_graphs = False
    calls = []
    real = pipe2.scheduler.step_master_
    pipe2.scheduler.step_master_ = lambda *a, **k: (calls.append((a[0].shape[0], k.get("v_text"), k.get("projected"))), real(*a, **k))[-1]
    assert torch.equal(pipe2(**kw2).images, want2)
    assert calls == [(1, None, None)] * STEPS                                 # the plain step on a batch-1 velocity: the same launches


# ------------------------------------------------------------------------------------------------------------------ 3. empty interval
def test_an_empty_interval_is_the_plain_call(gpu):
    """TrueCFGGuider(stop=0.0) with a negative prompt: no step is guided, every step runs on the positive half at batch B through
    views of what the call prepared at 2B — bit for bit the latents of the call without the negative prompt; eager and captured."""
    pipe, r = random_pipe(gpu, 931)
    kw = cfg_call(r)
    pipe.capture_graphs = False
    want = pipe(**call_without_negatives(kw)).images.clone()
    assert not torch.equal(pipe(**kw).images, want)
    pipe.guider = guider(stop=0.0)
    shapes = []
    real = pipe.scheduler.step_master_
    pipe.scheduler.step_master_ = lambda *a, **k: (shapes.append((a[0].shape[0], k.get("v_text"))), real(*a, **k))[-1]
    assert torch.equal(pipe(**kw).images, want)
    assert shapes == [(1, None)] * STEPS
    pipe.scheduler.step_master_ = real
    pipe.guider = guider(stop=0.0, eta=0.0, momentum=-0.5)
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, want)


def test_steps_outside_the_interval_have_the_plain_steps_bits(gpu):
    """Interval (0.5, 1): steps 0 and 1 run on the positive half. After them the state is that of the plain call with the positive
    prompt, bit for bit (a callback reads it)."""
    pipe, r = random_pipe(gpu, 932)
    kw = cfg_call(r)
    seen = {}

    def grab(name):
        def cb(p, i, t, env):
            if i == 1:
                seen[name] = env["latents"].clone()
            return {}
        return cb

    pipe(**call_without_negatives(kw), callback_on_step_end=grab("plain"))
    pipe.guider = guider(start=0.5)
    out = pipe(**kw, callback_on_step_end=grab("guided")).images
    assert torch.equal(seen["plain"], seen["guided"])
    pipe.guider = None
    assert not torch.equal(out, pipe(**kw).images)


# ------------------------------------------------------------------------------------------------------------------ 4. capture, replay
def test_guided_loop_graph_replay_is_bitwise_the_eager_loop(gpu):
    pipe, r = random_pipe(gpu, 941)
    kw = cfg_call(r)
    first = pipe(**kw).images.clone()                                       # the plain CFG call: seen
    cfg_keys = graph_keys(pipe)
    pipe.guider = guider(stop=0.5, eta=0.0, momentum=-0.5, norm_threshold=1.0)
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert not torch.equal(eager, first)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw).images, eager)
    assert pipe.scheduler._step_index == STEPS
    keys = graph_keys(pipe)
    assert len(keys) == 2 and keys[0] == cfg_keys[0] and ("guidance", (0, 1), 0.0, 1.0, -0.5) in keys[1]
    assert isinstance(pipe._graph_cache[keys[1]], dict)
    # new values, same signature: replayed, copied in
    kw2 = dict(kw, **negatives(r), latents=r(1, N, 64))
    pipe.capture_graphs = False
    eager2 = pipe(**kw2).images.clone()
    pipe.capture_graphs = True
    assert torch.equal(pipe(**kw2).images, eager2) and not torch.equal(eager2, eager) and graph_keys(pipe) == keys
    # the plain CFG call's key is what it was, and it returns its first bits: captured now, then replayed
    pipe.guider = None
    for _ in range(2):
        assert torch.equal(pipe(**kw).images, first)
    assert graph_keys(pipe) == keys


# ------------------------------------------------------------------------------------------------------------------ 5. batch, toggles
def test_guided_batch_of_two_is_two_calls(gpu):
    pipe, r = random_pipe(gpu, 951)
    pipe.capture_graphs = False
    pipe.guider = guider(stop=0.5, eta=0.0, momentum=-0.5, norm_threshold=2.0)
    kw = cfg_call(r, B=2)
    kw["control_mask"] = [torch.cat([token_mask(a), token_mask(b)]).to(gpu, torch.bfloat16) for a, b in
                          (((48, 96, 30, 200), (64, 112, 10, 120)), ((100, 150, 60, 240), (90, 140, 100, 250)))]
    both = pipe(**kw).images.clone()
    assert not torch.equal(both[0], both[1])
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k in ("control_image", "control_mask") else v)
               for k, v in kw.items()}
        assert torch.equal(pipe(**one).images, both[b : b + 1]), b


def test_overlap_and_row_window_are_bitwise_neutral_with_an_interval(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 961)
    pipe.capture_graphs = False
    pipe.guider = guider(start=0.25, stop=0.75, eta=0.0)
    kw = cfg_call(r, cn_steps=4)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    serial = pipe(**kw).images.clone()
    assert pipe._tower_window_used is not None
    for overlap, window in ((True, True), (False, False), (True, False)):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        monkeypatch.setattr(P, "TOWER_WINDOW", window)
        assert torch.equal(pipe(**kw).images, serial), (overlap, window)
        assert (pipe._tower_window_used is not None) == window


# ------------------------------------------------------------------------------------------------------------------ 6. combinations
def test_repaint_with_an_interval(gpu):
    """Strength 0.75 of 4 steps runs 3: the interval (0, 0.34) counts over those and guides the first of them only; the tokens outside
    the mask end as the source's latents bit for bit."""
    import test_repaint_gpu as RG

    pipe, r = RG.random_pipe(gpu, 971)
    pipe.capture_graphs = False
    kw = dict(RG.two_line_call(r), **negatives(r), true_cfg_scale=2.0)
    pipe.guider = guider(stop=0.34, eta=0.0, norm_threshold=1.0)
    seen = []
    real = pipe.scheduler.step_master_
    pipe.scheduler.step_master_ = lambda *a, **k: (seen.append((a[0].shape[0], k.get("v_text") is not None, k.get("projected") is not None)), real(*a, **k))[-1]
    out = pipe(**kw).images
    pipe.scheduler.step_master_ = real
    assert seen == [(1, True, True), (1, False, False), (1, False, False)]
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, gpu)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(out[mask == 0], kw["image"][mask == 0]) and not bool((out[mask == 1] == kw["image"][mask == 1]).any())
    pipe.guider = None
    assert not torch.equal(pipe(**kw).images, out)
    pipe.guider = guider(stop=0.34, eta=0.0, norm_threshold=1.0)
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, out)


def test_union_tower_across_the_intervals_end(gpu):
    """The union tower on [0.2, 0.8] of 4 steps (steps 1 and 2), guidance on (0, 0.5) (steps 0 and 1): the tower runs at 2B at step 1 and
    at B at step 2. Eager = captured, and the serial order gives the same bits."""
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 972, union=True)
    kw = dict(cfg_call(r, cn_steps=3), control_image_union=r(1, N, 64), controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.2,
              control_guidance_end_union=0.8)
    pipe.guider = guider(stop=0.5, eta=0.0, momentum=-0.5)
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert bool(torch.isfinite(eager).all())
    assert not torch.equal(pipe(**{k: v for k, v in kw.items() if "union" not in k}).images, eager)
    old = P.OVERLAP_TOWER
    try:
        P.OVERLAP_TOWER = not old
        assert torch.equal(pipe(**kw).images, eager)
    finally:
        P.OVERLAP_TOWER = old
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, eager)


def test_image_prompt_with_an_interval(gpu):
    """An image prompt with explicit negative embeds: outside the interval the positive half's K/V are views of the ones prepared at 2B.
    With an empty interval the call is the one without a negative prompt, bit for bit; with (0, 0.5) eager = captured."""
    pipe, r = random_pipe(gpu, 973)
    ipp = ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=E, seed=974)
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale([1.0, -0.7])
    emb, nemb = r(1, E), r(1, E)
    kw = dict(cfg_call(r), ip_adapter_image_embeds=emb, negative_ip_adapter_image_embeds=[nemb[:, None]])
    pipe.capture_graphs = False
    plain = pipe(**{k: v for k, v in kw.items() if "negative" not in k and k != "true_cfg_scale"}).images.clone()
    pipe.guider = guider(stop=0.0)
    assert torch.equal(pipe(**kw).images, plain)
    pipe.guider = guider(stop=0.5, eta=0.0)
    eager = pipe(**kw).images.clone()
    assert not torch.equal(eager, plain) and bool(torch.isfinite(eager).all())
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, eager)


def test_guided_call_in_the_fp8_modes(gpu):
    pipe, r = random_pipe(gpu, 975)
    pipe.transformer.enable_fp8_linears("mx").enable_fp8_attention(True)
    pipe.guider = guider(stop=0.5, eta=0.0, momentum=-0.5, norm_threshold=1.0)
    kw = cfg_call(r)
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert bool(torch.isfinite(eager).all()) and not torch.equal(eager, kw["latents"].float())
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, eager)
    assert sum(isinstance(v, dict) for v in pipe._graph_cache.values()) == 1


# ------------------------------------------------------------------------------------------------------------------ 7. refusal, callback
def test_the_inpaint_pipeline_refuses_a_guider(gpu):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as Inpaint
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16).random_init_(981)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16).random_init_(982)
    cni = FluxControlNetModel(**dict(SMALL_CN, extra_condition_channels=4), device=gpu, dtype=torch.bfloat16).random_init_(983)
    pipe = Inpaint(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn, cni)
    pipe.guider = guider(stop=0.5)
    with pytest.raises(ValueError, match="guider"):
        pipe(prompt_embeds=torch.zeros(1, T, 256, device=gpu), pooled_prompt_embeds=torch.zeros(1, 64, device=gpu), height=H, width=W,
             num_inference_steps=2)


def test_a_callback_that_returns_latents_restarts_the_momentum(gpu):
    """A callback returns ``latents`` after step 0: step 1 is a first guided step again, β = 0 — its difference buffer is written and
    not read. Shown by poisoning the buffer with NaN before that step: the result is the same bits, and finite. Without the callback's
    replacement the same poison reaches the state."""
    pipe, r = random_pipe(gpu, 991)
    pipe.guider = guider(eta=0.0, momentum=-0.5)
    kw = cfg_call(r)
    real = pipe.scheduler.step_master_
    firsts = []

    def run(replace, poison):
        n = [0]

        def step(*a, **k):
            rec = k["projected"]
            firsts.append(rec.first)
            if poison and n[0] == 1:
                rec.diff.fill_(float("nan"))
            n[0] += 1
            return real(*a, **k)

        pipe.scheduler.step_master_ = step
        cb = (lambda p, i, t, env: {"latents": env["latents"]} if i == 0 else {}) if replace else (lambda p, i, t, env: {})
        try:
            return pipe(**kw, callback_on_step_end=cb).images.clone()
        finally:
            pipe.scheduler.step_master_ = real

    clean = run(True, False)
    assert firsts == [True, True, False, False]
    firsts.clear()
    poisoned = run(True, True)
    assert torch.equal(poisoned, clean) and bool(torch.isfinite(clean).all())
    firsts.clear()
    assert not bool(torch.isfinite(run(False, True)).all()) and firsts == [True, False, False, False]
    assert not torch.equal(run(False, False), clean)
