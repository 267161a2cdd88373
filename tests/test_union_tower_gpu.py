"""The second ControlNet of the base pipeline (pipe.controlnet_union + control_image_union=...) on the GPU: parity with the CPU
oracle's loop (tests/loop_reference.py), and the bitwise properties of its schedule — zero tower, empty interval, side stream,
row window, captured graph, batch, image path. 256x256 (N = 256, T = 64) with the reduced models of test_vae_pipeline_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402
from oracle import vae_oracle as vorc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, VAE_SMALL, rel_l2  # noqa: E402
from loop_reference import denoise_loop_reference  # noqa: E402

SMALL_UN = dict(SMALL_T, num_layers=2, num_single_layers=0)
BOXES = ((48, 96, 30, 200), (100, 150, 60, 240))        # two text lines inside image rows 48..144 of 256: the row window is active


@pytest.fixture(scope="module")
def vae(gpu):
    from reptext_amd.vae import AutoencoderKL

    v = AutoencoderKL(**VAE_SMALL, device=gpu, dtype=torch.bfloat16)
    v.load_state_dict(vorc.init_vae_params(VAE_SMALL, seed=3), strict=True)
    return v


def mask_images(boxes, H=256, W=256):
    from PIL import Image

    out = []
    for box in boxes:
        m = np.zeros([H, W], dtype=np.uint8); m[box[0]:box[1], box[2]:box[3]] = 255
        out.append(Image.fromarray(m))
    return out


def random_pipe(gpu, vae, seed, zero_union=False, cn_layers=2, un_layers=2):
    """(pipe, r): a base pipeline with random transformer, text tower and union tower; r(*shape) draws bf16 device tensors."""
    import reptext_amd.pipeline as P
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16).random_init_(seed)
    cn = FluxControlNetModel(**dict(SMALL_CN, num_layers=cn_layers), device=gpu, dtype=torch.bfloat16).random_init_(seed + 1)
    un = FluxControlNetModel(**dict(SMALL_UN, num_layers=un_layers), device=gpu, dtype=torch.bfloat16).random_init_(seed + 2)
    if zero_union:
        un.zero_init_controlnet_()
    pipe = P.FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), vae, None, None, None, None, tr, cn)
    pipe.controlnet_union = un
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(seed)
    return pipe, (lambda *s: torch.randn(*s, generator=g).to(gpu, torch.bfloat16))


@pytest.mark.parametrize("case", ["text_line_256", "no_text_line_256", "text_line_384", "shallow_union_256"])
def test_union_tower_matches_the_oracle_loop(vae, gpu, case):
    """3 steps, one masked text line with controlnet_conditioning_step=2, union scale 0.7 on [0.3, 1.0]: step 0 text only, step 1 both
    (union first), step 2 union only; the mask box leaves the text tower's row window active. Also without any text line, at
    width 384 (N = 384), and with a union tower of one block against the text tower's two (it adds into the first sample only; every
    block of every tower is then evaluated and there is no window). GPU error at the bf16-storage oracle's own floor."""
    from reptext_amd.controlnet import FluxControlNetModel, active_row_window
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    H, W = (256, 384) if case == "text_line_384" else (256, 256)
    h2, w2, T = 2 * (H // 16), 2 * (W // 16), 64
    N = (h2 // 2) * (w2 // 2)
    UN = dict(SMALL_UN, num_layers=1) if case == "shallow_union_256" else SMALL_UN
    tp = orc.init_mmdit_params(SMALL_T, seed=111)
    cp = orc.init_mmdit_params(SMALL_CN, seed=112, controlnet=True)
    up = orc.init_mmdit_params(UN, seed=113, controlnet=True)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    un = FluxControlNetModel(**UN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp); cn.load_state_dict(cp); un.load_state_dict(up)
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), vae, None, None, None, None, tr, cn)
    pipe.controlnet_union = un
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    pe, pooled, hint, uhint = r(1, T, 256), r(1, 64), r(1, N, 128), r(1, N, 64)
    lat0 = orc.pack_latents(r(1, 16, h2, w2))
    mask_np = np.zeros([H, W], dtype=np.uint8)
    mask_np[60:140, 80:200] = 255                                   # the box of test_pipeline_c1_latents_and_image
    rm = torch.nn.functional.interpolate(torch.from_numpy(mask_np)[None, None].float() / 255.0, scale_factor=1 / 16, mode="bilinear").reshape(1, -1, 1)
    lines = case != "no_text_line_256"
    hints, rms = ([hint], [rm]) if lines else ([], [])
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    args = (tp, SMALL_T, cp, SMALL_CN, lat0, pe, pooled, hints, rms, sig, orc.latent_image_ids(h2, w2), torch.zeros(T, 3), 3.5)
    kw = dict(conditioning_scale=1.0, conditioning_step=2, union=dict(params=up, cfg=UN, cond=uhint, scale=0.7, start=0.3, end=1.0))
    ref = denoise_loop_reference(*args, **kw)
    with orc.stored_as(torch.bfloat16):
        ref16 = denoise_loop_reference(*args, **kw)
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    from PIL import Image

    call = dict(prompt_embeds=b16(pe), pooled_prompt_embeds=b16(pooled), height=H, width=W, num_inference_steps=3, guidance_scale=3.5,
                controlnet_conditioning_scale=1.0, controlnet_conditioning_step=2, latents=b16(lat0), output_type="latent",
                control_image_union=b16(uhint), controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.3,
                control_guidance_end_union=1.0)
    if lines:
        call.update(control_image=[b16(hint)], control_mask=[Image.fromarray(mask_np)])
    out = pipe(**call).images.float().cpu()
    if lines:
        assert active_row_window([b16(rm)], N) is not None
        assert (pipe._tower_window_used is None) == (case == "shallow_union_256")       # equal depths: the window was in use
    err, err16, floor = rel_l2(out, ref), rel_l2(out, ref16), rel_l2(ref16, ref)
    print(f"union tower [{case}] latents rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e})")
    # the union tower is felt: the same loop without it is far from this reference
    no_union = orc.denoise_loop(tp, SMALL_T, cp, SMALL_CN, lat0, pe, pooled, hints, rms, sig, orc.latent_image_ids(h2, w2), torch.zeros(T, 3), 3.5,
                                conditioning_step=2)
    assert rel_l2(no_union, ref) > 20 * floor
    assert_at_dtype_floor(err, err16, floor)


def two_line_call(r, steps=4, cn_steps=4, B=1):
    """Two masked text lines (row window active) on every step; a union interval [0.2, 0.8] of 4 steps covers steps 1 and 2, so the loop
    sees text-only -> both -> both -> text-only: the buffers are written in full and must read zero outside the window again."""
    return dict(prompt_embeds=r(B, 64, 256), pooled_prompt_embeds=r(B, 64), height=256, width=256, num_inference_steps=steps, guidance_scale=3.5,
                control_image=[r(B, 256, 128), r(B, 256, 128)], control_mask=mask_images(BOXES), controlnet_conditioning_step=cn_steps,
                latents=r(B, 256, 64), output_type="latent")


UNION_MID = dict(controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.2, control_guidance_end_union=0.8)


def test_zero_initialised_union_tower_changes_nothing(vae, gpu):
    """Two text lines for 2 of 3 steps; a zero-initialised union tower on every step adds exact zeros, also on the union-only step."""
    pipe, r = random_pipe(gpu, vae, 121, zero_union=True)
    kw = two_line_call(r, steps=3, cn_steps=2)
    want = pipe(**kw).images.clone()
    assert not torch.equal(want, kw["latents"].float())
    for _ in range(2):                                               # eager, then captured
        assert torch.equal(pipe(**kw, control_image_union=r(1, 256, 64)).images, want)


def test_empty_union_interval_is_the_call_without_it(vae, gpu):
    pipe, r = random_pipe(gpu, vae, 131)
    kw = two_line_call(r, steps=3, cn_steps=2)
    want = pipe(**kw).images.clone()
    got = pipe(**kw, control_image_union=r(1, 256, 64), control_guidance_start_union=0.9, control_guidance_end_union=0.1).images
    assert torch.equal(got, want)
    felt = pipe(**kw, control_image_union=r(1, 256, 64)).images
    assert not torch.equal(felt, want)


@pytest.mark.parametrize("case", ["equal_depths", "deeper_text_tower", "shallow_union_alone"])
def test_event_records_per_step_are_what_the_transformer_waits_on(vae, gpu, monkeypatch, case):
    """The side stream's events, counted on the host per step (``torch.cuda.Event.record`` patched on the class; eager loop). The
    transformer waits on the events k < need_d, the highest sample its block map i // ceil(n_blocks / n_samples) reaches. A call
    without a union image records exactly those per tower step: the one loop must not cost it a stream operation, which no output bit
    would show. A union call records no fewer, and a step without towers none. Two masked text lines, 4 steps, union on steps 1 and 2.
    ``deeper_text_tower``: 3 tower blocks against the transformer's 2, so sample 2 is never read or waited on. ``shallow_union_alone``:
    a 1-block union tower with the text towers off after step 2, so step 2 is the union tower alone, which writes one sample of two."""
    import math

    import reptext_amd.pipeline as P

    cn_layers, un_layers, cn_steps = {"equal_depths": (2, 2, 4), "deeper_text_tower": (3, 2, 4), "shallow_union_alone": (2, 1, 2)}[case]
    pipe, r = random_pipe(gpu, vae, 181, cn_layers=cn_layers, un_layers=un_layers)
    pipe.capture_graphs = False
    monkeypatch.setattr(P, "OVERLAP_TOWER", True)
    n_td = len(pipe.transformer.transformer_blocks)
    need_d = (n_td - 1) // math.ceil(n_td / cn_layers) + 1
    assert need_d == 2
    per_step, pending, joining = [], [0], [False]
    record, wait_stream, forward = torch.cuda.Event.record, torch.cuda.Stream.wait_stream, pipe.transformer.forward

    def counted_record(self, *a, **k):
        pending[0] += not joining[0]
        return record(self, *a, **k)

    def uncounted_wait_stream(self, stream):                            # the step's fork and join record an event of their own
        joining[0] = True
        try:
            return wait_stream(self, stream)
        finally:
            joining[0] = False

    def counted_forward(*a, **k):                                       # the tower(s) of a step are enqueued before its transformer
        per_step.append(pending[0]); pending[0] = 0
        return forward(*a, **k)

    monkeypatch.setattr(torch.cuda.Event, "record", counted_record)
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", uncounted_wait_stream)
    monkeypatch.setattr(pipe.transformer, "forward", counted_forward)
    kw = two_line_call(r, cn_steps=cn_steps)
    want = pipe(**kw).images.clone()
    tower_step = [i < cn_steps for i in range(4)]
    print(f"[{case}] need_d {need_d}; records per step without a union image {per_step}")
    assert per_step == [need_d if on else 0 for on in tower_step] and pending[0] == 0
    del per_step[:]
    empty = pipe(**kw, control_image_union=r(1, 256, 64), control_guidance_start_union=0.9, control_guidance_end_union=0.1).images
    assert torch.equal(empty, want)
    assert per_step == [need_d if on else 0 for on in tower_step] and pending[0] == 0
    del per_step[:]
    pipe(**kw, control_image_union=r(1, 256, 64), **UNION_MID)
    print(f"[{case}] records per step with the union tower on steps 1 and 2 {per_step}")
    tower_step = [on or i in (1, 2) for i, on in enumerate(tower_step)]
    assert len(per_step) == 4 and pending[0] == 0
    assert all(n >= need_d if on else n == 0 for n, on in zip(per_step, tower_step))


def test_overlap_and_row_window_are_bitwise_neutral_with_a_union_tower(vae, gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, vae, 141)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r), control_image_union=r(1, 256, 64), **UNION_MID)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    serial = pipe(**kw).images.clone()
    assert pipe._tower_window_used is not None
    monkeypatch.setattr(P, "OVERLAP_TOWER", True)
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, serial)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    for overlap in (False, True):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        assert torch.equal(pipe(**kw).images, serial)
        assert pipe._tower_window_used is None
    # a call WITHOUT the union tower right after: its window promise ("zero outside, zeroed once") must be re-established
    plain = {k: v for k, v in kw.items() if "union" not in k}
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    want_plain = pipe(**plain).images.clone()
    monkeypatch.setattr(P, "TOWER_WINDOW", True)
    pipe(**kw)
    assert torch.equal(pipe(**plain).images, want_plain)


def test_union_loop_graph_replay_is_bitwise_the_eager_loop(vae, gpu):
    pipe, r = random_pipe(gpu, vae, 151)

    def inputs():
        kw = two_line_call(r)
        return {k: kw[k] for k in ("prompt_embeds", "pooled_prompt_embeds", "control_image", "latents")} | dict(control_image_union=r(1, 256, 64))

    fixed = {k: v for k, v in two_line_call(r).items() if k not in ("prompt_embeds", "pooled_prompt_embeds", "control_image", "latents")}
    fixed.update(UNION_MID)
    a, b = inputs(), inputs()

    def eager(kw):
        pipe.capture_graphs = False
        try:
            return pipe(**kw).images.clone()
        finally:
            pipe.capture_graphs = True

    ref_a, ref_b = eager({**a, **fixed}), eager({**b, **fixed})
    assert not torch.equal(ref_a, ref_b)
    assert torch.equal(pipe(**a, **fixed).images, ref_a)                       # eager, signature remembered
    assert torch.equal(pipe(**a, **fixed).images, ref_a)                       # captured + replayed
    assert sum(isinstance(v, dict) for v in pipe._graph_cache.values()) == 1   # exactly one graph for this signature
    assert torch.equal(pipe(**b, **fixed).images, ref_b)                       # replay on inputs (and a union hint) never seen
    assert torch.equal(pipe(**{**a, "control_image_union": b["control_image_union"]}, **fixed).images,
                       eager({**a, "control_image_union": b["control_image_union"], **fixed}))
    assert torch.equal(pipe(**a, **fixed).images, ref_a)
    assert sum(isinstance(v, dict) for v in pipe._graph_cache.values()) == 1
    assert pipe.scheduler._step_index == 4
    # another scale, another end: new keys, each equal to its own eager run (and not served by the first graph)
    for change in (dict(controlnet_conditioning_scale_union=0.5), dict(control_guidance_end_union=0.6)):
        kw = {**a, **fixed, **change}
        want = eager(kw)
        assert not torch.equal(want, ref_a)
        assert torch.equal(pipe(**kw).images, want)
        assert torch.equal(pipe(**kw).images, want)
    # a call without the union argument afterwards
    plain = {k: v for k, v in {**a, **fixed}.items() if "union" not in k}
    want = eager(plain)
    assert torch.equal(pipe(**plain).images, want)
    assert torch.equal(pipe(**plain).images, want)


def test_union_hints_per_sample_are_batch_invariant(vae, gpu):
    pipe, r = random_pipe(gpu, vae, 161)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, B=2), control_image_union=r(2, 256, 64), **UNION_MID)
    both = pipe(**kw).images.clone()
    assert not torch.equal(both[0], both[1])
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k == "control_image" else v) for k, v in kw.items()}
        assert torch.equal(pipe(**one).images, both[b : b + 1]), b


def test_union_image_is_encoded_like_the_canny_hint_after_the_text_lines(vae, gpu):
    """A PIL control_image_union gives the bits of the packed latents computed here the same way (preprocess, posterior sample from the
    global RNG, shift/scale, pack); with text-line images in the call the union image is encoded after them, so their hints are those
    of the call without it under the same seed."""
    from PIL import Image, ImageDraw

    pipe, r = random_pipe(gpu, vae, 171)
    pipe.capture_graphs = False
    img = Image.new("RGB", (256, 256), (0, 0, 0))
    ImageDraw.Draw(img).ellipse((40, 60, 200, 220), outline=(255, 255, 255), width=3)
    base = dict(prompt_embeds=r(1, 64, 256), pooled_prompt_embeds=r(1, 64), height=256, width=256, num_inference_steps=2, guidance_scale=3.5,
                latents=r(1, 256, 64), output_type="latent", controlnet_conditioning_scale_union=0.7)
    torch.manual_seed(77)
    from_image = pipe(**base, control_image_union=img).images.clone()
    torch.manual_seed(77)
    px = pipe.image_processor.preprocess(img, height=256, width=256).to(device=gpu, dtype=torch.bfloat16)
    lat = pipe.vae.encode(px).latent_dist.sample()
    lat = ((lat - pipe.vae.config.shift_factor) * pipe.vae.config.scaling_factor).to(torch.bfloat16)
    packed = pipe._pack_latents(lat, 1, 16, 32, 32)
    assert packed.shape == (1, 256, 64)
    assert torch.equal(pipe(**base, control_image_union=packed).images, from_image)
    assert not torch.equal(pipe(**base).images, from_image)
    # text-line hints from images: record what the loop receives
    edges = Image.new("RGB", (256, 256), (255, 255, 255))
    ImageDraw.Draw(edges).rectangle((60, 90, 190, 150), outline=(0, 0, 0))
    pos_np = np.zeros([256, 256], dtype=np.uint8); pos_np[90:150, 60:190] = 255
    seen = []
    inner = pipe._denoise
    pipe._denoise = lambda *a, **k: (seen.append([h.clone() for h in a[6]]), inner(*a, **k))[1]
    lines = dict(base, control_image=[edges], control_position=[Image.fromarray(pos_np)], control_mask=mask_images(BOXES[:1]))
    torch.manual_seed(78)
    pipe(**lines)
    torch.manual_seed(78)
    pipe(**lines, control_image_union=img)
    assert len(seen) == 2 and len(seen[0]) == 1 and torch.equal(seen[0][0], seen[1][0])
