"""Stochastic flow-match sampling (the scheduler's ``stochastic_sampling``) in the pipelines on the GPU: parity of the loop with the
CPU oracle's (tests/loop_reference.py with the oracle's Euler step replaced by the stochastic rule, tests/stochastic_reference.py) —
plain, under true CFG, in a repaint and at eta = 0.5 — and the bitwise properties of the call: eager = captured = replay, another
seed replays the same graph, a sample of a batch is its own call, and the Euler call's key and result are untouched by stochastic
calls around it. 256x256 (N = 256, T = 64) with the reduced models of test_vae_pipeline_gpu.py, 4 steps, like test_multistep_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_repaint_gpu import BOX, H, N, T, W, box_image  # noqa: E402
from test_repaint_gpu import random_pipe as random_repaint_pipe  # noqa: E402
from test_repaint_gpu import two_line_call as two_line_repaint_call  # noqa: E402
from test_true_cfg_gpu import graph_keys, negatives, random_pipe, token_mask, two_line_call  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2  # noqa: E402

from loop_reference import denoise_loop_reference  # noqa: E402
from stochastic_reference import stochastic_euler_step  # noqa: E402

BF16 = torch.bfloat16


def stochastic(pipe, eta=1.0):
    """Swap the pipeline's scheduler for one with the switch on; returns the one it had."""
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    old = pipe.scheduler
    pipe.scheduler = FlowMatchEulerDiscreteScheduler.from_config(dict(old.config, stochastic_sampling=True, stochastic_eta=eta))
    return old


def stochastic_entries(key):
    return [k for k in key if isinstance(k, tuple) and k[:1] == ("stochastic",)]


def seeded(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", ["plain", "cfg", "repaint", "eta_half"])
def test_stochastic_matches_the_oracle_loop(gpu, case):
    """4 steps, one masked text line: GPU error at the bf16-storage oracle's own floor; under true CFG at s = 2; in a repaint at
    strength 0.75 (3 steps run, from sigma_1, drawing at the absolute steps 1..3); and at eta = 0.5. The condition on the inputs —
    asserted on the oracle alone — is that the Euler loop lies at least 10 floors away."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline, repaint_t_start
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    eta, seed = (0.5 if case == "eta_half" else 1.0), 4242
    tp = orc.init_mmdit_params(SMALL_T, seed=1011)
    cp = orc.init_mmdit_params(SMALL_CN, seed=1012, controlnet=True)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    tr.load_state_dict(tp); cn.load_state_dict(cp)
    cls = FluxControlNetRepaintPipeline if case == "repaint" else FluxControlNetPipeline
    pipe = cls(FlowMatchEulerDiscreteScheduler(stochastic_sampling=True, stochastic_eta=eta), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(1013)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).float()
    pe, pooled, npe, npooled, hint = r(1, T, 256), r(1, 64), r(1, T, 256), r(1, 64), r(1, N, 128)
    npe, npooled = (3 * npe).to(BF16).float(), (3 * npooled).to(BF16).float()          # as in test_true_cfg_matches_the_oracle_loop
    noise = orc.pack_latents(r(1, 16, 32, 32))
    src = torch.randn(1, N, 64, generator=g) * 0.7 + 0.2                                # fp32, not on the bf16 grid
    rm = token_mask(BOX)
    b16 = lambda t: t.to(gpu, BF16)
    call = dict(prompt_embeds=b16(pe), pooled_prompt_embeds=b16(pooled), height=H, width=W, num_inference_steps=4, guidance_scale=3.5,
                control_image=[b16(hint)], control_mask=[box_image(BOX)], controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30,
                latents=b16(noise), output_type="latent", generator=seeded(seed))
    sig = orc.flow_sigmas(4, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    ids = (orc.latent_image_ids(32, 32), torch.zeros(T, 3))
    args = (tp, SMALL_T, cp, SMALL_CN, noise, pe, pooled, [hint], [rm], sig, *ids, 3.5)
    rkw = dict(conditioning_scale=1.0, conditioning_step=30)
    if case == "cfg":
        call.update(negative_prompt_embeds=b16(npe), negative_pooled_prompt_embeds=b16(npooled), true_cfg_scale=2.0)
        rkw["negative"] = dict(prompt_embeds=npe, pooled=npooled, scale=2.0)
    elif case == "repaint":
        call.update(image=src.to(gpu), mask_image=box_image(BOX), strength=0.75)
        mask = pipe._pack_mask(box_image(BOX), H, W, "cpu")
        t_start = repaint_t_start(4, 0.75)
        assert t_start == 1 and 0 < int(mask.sum()) < mask.numel()
        rkw["repaint"] = dict(src=src, noise=noise, mask=mask, t_start=t_start)
    with stochastic_euler_step(sig, [(seed, 0)], eta):
        ref = denoise_loop_reference(*args, **rkw)
        with orc.stored_as(BF16):
            ref16 = denoise_loop_reference(*args, **rkw)
    euler = denoise_loop_reference(*args, **rkw)
    if case == "plain":
        assert torch.equal(euler, orc.denoise_loop(*args, **rkw))                        # the substitution is gone
    floor, felt = rel_l2(ref16, ref), rel_l2(euler, ref)
    out = pipe(**call).images.float().cpu()
    assert pipe.scheduler._step_index == 4 and len(pipe.scheduler.sigmas) == len(sig)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"stochastic [{case}] latents rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e}); the Euler "
          f"loop lies {felt:.3e} = {felt / floor:.0f} x floor away")
    assert felt >= 10 * floor
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)
    assert not [k for k in pipe.__dict__ if "noise" in k or "rng" in k]


# ------------------------------------------------------------------------------------------------------------------ 2. eager = captured = replay
def test_graph_replay_is_bitwise_the_eager_loop_and_the_euler_key_stays(gpu):
    pipe, r = random_pipe(gpu, 1111)
    kw = two_line_call(r, steps=4)
    euler_first = pipe(**kw).images.clone()                                 # seen: the Euler call's key
    euler_keys = graph_keys(pipe)
    assert len(euler_keys) == 1 and not stochastic_entries(euler_keys[0])
    euler_sched = stochastic(pipe, eta=0.5)
    a, b = dict(kw, generator=seeded(1)), dict(kw, generator=seeded(2))
    pipe.capture_graphs = False
    eager_a, eager_b = pipe(**a).images.clone(), pipe(**b).images.clone()
    assert pipe.scheduler._step_index == 4 and graph_keys(pipe) == euler_keys
    assert not torch.equal(eager_a, euler_first) and not torch.equal(eager_a, eager_b)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**a).images, eager_a) and pipe.scheduler._step_index == 4
    keys = graph_keys(pipe)
    assert len(keys) == 2 and keys[0] == euler_keys[0] and stochastic_entries(keys[1]) == [("stochastic", 0.5)] and keys[1][-1] == ("stochastic", 0.5)
    assert isinstance(pipe._graph_cache[keys[1]], dict)
    assert list(keys[1][:-1]) == list(keys[0])                              # the Euler key plus one entry at its end
    # seed A, then B, then A through the one graph: the seeds are a static input, the step index is baked per node
    assert torch.equal(pipe(**b).images, eager_b) and torch.equal(pipe(**a).images, eager_a) and graph_keys(pipe) == keys
    # the Euler scheduler back: its old key, now captured and replayed, its first bits; then the stochastic replay again
    stoch_sched, pipe.scheduler = pipe.scheduler, euler_sched
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, euler_first)
    assert graph_keys(pipe) == keys and isinstance(pipe._graph_cache[keys[0]], dict)
    pipe.scheduler = stoch_sched
    assert torch.equal(pipe(**a).images, eager_a) and graph_keys(pipe) == keys
    assert_no_call_state(pipe)


def test_graph_replay_under_cfg_in_a_repaint(gpu):
    pipe, r = random_repaint_pipe(gpu, 1121)
    stochastic(pipe)
    kw = dict(two_line_repaint_call(r), **negatives(r), true_cfg_scale=2.0, generator=seeded(3))
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert pipe.scheduler._step_index == 4                                  # begin index 1 + 3 steps
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, eager) and pipe.scheduler._step_index == 4
    keys = graph_keys(pipe)
    assert len(keys) == 1 and stochastic_entries(keys[0]) == [("stochastic", 1.0)] and ("cfg", 2.0) in keys[0]
    assert isinstance(pipe._graph_cache[keys[0]], dict)
    # the background is still the source, bit for bit: the kept region keeps its rule
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, gpu)
    assert torch.equal(eager[mask == 0], kw["image"][mask == 0])


# ------------------------------------------------------------------------------------------------------------------ 3. batch
def test_batch_of_two_with_two_generators_is_two_calls(gpu):
    pipe, r = random_pipe(gpu, 1141)
    stochastic(pipe)
    pipe.capture_graphs = False
    kw = two_line_call(r, steps=4, B=2)
    kw["control_mask"] = [torch.cat([token_mask(a), token_mask(b)]).to(gpu, BF16) for a, b in
                          (((48, 96, 30, 200), (64, 112, 10, 120)), ((100, 150, 60, 240), (90, 140, 100, 250)))]
    gens = [seeded(21), seeded(22)]
    both = pipe(**kw, generator=gens).images.clone()
    assert not torch.equal(both[0], both[1])
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k in ("control_image", "control_mask") else v)
               for k, v in kw.items()}
        assert torch.equal(pipe(**one, generator=gens[b]).images, both[b : b + 1]), b
        assert torch.equal(pipe(**one, generator=[gens[b]]).images, both[b : b + 1]), b
    # one generator for the batch: the samples take subsequences 0 and 1 of its stream — sample 0 is the call above, sample 1 is not
    shared = pipe(**kw, generator=gens[0]).images
    assert torch.equal(shared[0], both[0]) and not torch.equal(shared[1], both[1])
