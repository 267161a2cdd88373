"""The second-order multistep scheduler (reptext_amd.scheduler.FlowMatchMultistepScheduler) in the pipelines on the GPU: parity of the
loop with the CPU oracle's (tests/loop_reference.py) — plain, under true CFG and in a repaint — and the bitwise properties of the
call: eager = captured = replay, the Euler call's graph key and result untouched by multistep calls around it, ``solver_order=1`` is
the Euler call, batch invariance, the loop's toggles, and a callback that hands the latents back makes the next step first order.
256x256 (N = 256, T = 64) with the reduced models of test_vae_pipeline_gpu.py, 4 steps, like test_repaint_gpu.py."""
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

BF16 = torch.bfloat16


def multistep(pipe, **config):
    """Swap the pipeline's scheduler the diffusers way; returns the one it had."""
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    old = pipe.scheduler
    pipe.scheduler = FlowMatchMultistepScheduler.from_config(dict(old.config, **config))
    return old


def solver_entries(key):
    return [k for k in key if isinstance(k, tuple) and k[:1] == ("solver",)]


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", ["plain", "cfg", "repaint"])
def test_multistep_matches_the_oracle_loop(gpu, case):
    """4 steps, one masked text line: GPU error at the bf16-storage oracle's own floor; under true CFG at s = 2; and in a repaint at
    strength 0.75 (3 steps run, from sigma_1, the first of them first order). The condition on the inputs — asserted on the oracle alone
    — is that the Euler loop lies at least 10 floors away. The Euler loop is the same reference at ``order=1`` (every weight 0), so the
    two differ in the rule alone; without extensions it is held bit for bit to orc.denoise_loop."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline, repaint_t_start
    from reptext_amd.scheduler import FlowMatchMultistepScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tp = orc.init_mmdit_params(SMALL_T, seed=811)
    cp = orc.init_mmdit_params(SMALL_CN, seed=812, controlnet=True)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    tr.load_state_dict(tp); cn.load_state_dict(cp)
    cls = FluxControlNetRepaintPipeline if case == "repaint" else FluxControlNetPipeline
    pipe = cls(FlowMatchMultistepScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(813)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).float()
    pe, pooled, npe, npooled, hint = r(1, T, 256), r(1, 64), r(1, T, 256), r(1, 64), r(1, N, 128)
    npe, npooled = (3 * npe).to(BF16).float(), (3 * npooled).to(BF16).float()          # as in test_true_cfg_matches_the_oracle_loop
    noise = orc.pack_latents(r(1, 16, 32, 32))
    src = torch.randn(1, N, 64, generator=g) * 0.7 + 0.2                                # fp32, not on the bf16 grid
    rm = token_mask(BOX)
    b16 = lambda t: t.to(gpu, BF16)
    call = dict(prompt_embeds=b16(pe), pooled_prompt_embeds=b16(pooled), height=H, width=W, num_inference_steps=4, guidance_scale=3.5,
                control_image=[b16(hint)], control_mask=[box_image(BOX)], controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30,
                latents=b16(noise), output_type="latent")
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
    ref = denoise_loop_reference(*args, **rkw, order=2)
    with orc.stored_as(BF16):
        ref16 = denoise_loop_reference(*args, **rkw, order=2)
    euler = denoise_loop_reference(*args, **rkw, order=1)
    if case == "plain":
        assert torch.equal(euler, orc.denoise_loop(*args, **rkw))
    floor, felt = rel_l2(ref16, ref), rel_l2(euler, ref)
    out = pipe(**call).images.float().cpu()
    assert pipe.scheduler._step_index == 4 and pipe.scheduler._history_len == 1 and len(pipe.scheduler.sigmas) == len(sig)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"multistep [{case}] latents rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e}); the Euler "
          f"loop lies {felt:.3e} = {felt / floor:.0f} x floor away")
    assert felt >= 10 * floor
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)
    assert not [k for k in pipe.__dict__ if "hist" in k]


# ------------------------------------------------------------------------------------------------------------------ 2. eager = captured = replay
def test_graph_replay_is_bitwise_the_eager_loop_and_the_euler_key_stays(gpu):
    pipe, r = random_pipe(gpu, 911)
    kw = two_line_call(r, steps=4)
    euler_first = pipe(**kw).images.clone()                                 # seen: the Euler call's key
    euler_keys = graph_keys(pipe)
    assert len(euler_keys) == 1 and not solver_entries(euler_keys[0])
    euler_sched = multistep(pipe)
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    state = (pipe.scheduler._step_index, pipe.scheduler._history_len)
    assert state == (4, 1) and graph_keys(pipe) == euler_keys and not torch.equal(eager, euler_first)
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw).images, eager)
        assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == state
    keys = graph_keys(pipe)
    assert len(keys) == 2 and keys[0] == euler_keys[0] and solver_entries(keys[1]) == [("solver", 2)]
    assert isinstance(pipe._graph_cache[keys[1]], dict)
    assert [k for k in keys[1] if k not in solver_entries(keys[1])] == list(keys[0])          # the Euler key plus one entry
    # new latents, same signature: replayed, copied in
    kw2 = dict(kw, latents=r(1, N, 64))
    pipe.capture_graphs = False
    eager2 = pipe(**kw2).images.clone()
    pipe.capture_graphs = True
    assert torch.equal(pipe(**kw2).images, eager2) and not torch.equal(eager2, eager) and graph_keys(pipe) == keys
    # the Euler scheduler back: its old key, now captured and replayed, its first bits; then the multistep replay again
    multi_sched, pipe.scheduler = pipe.scheduler, euler_sched
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, euler_first)
    assert graph_keys(pipe) == keys and isinstance(pipe._graph_cache[keys[0]], dict)
    pipe.scheduler = multi_sched
    assert torch.equal(pipe(**kw).images, eager) and graph_keys(pipe) == keys
    assert_no_call_state(pipe)
    assert not [k for k in pipe.__dict__ if "hist" in k]


def test_graph_replay_under_cfg_and_in_a_repaint(gpu):
    pipe, r = random_repaint_pipe(gpu, 921)
    multistep(pipe)
    kw = dict(two_line_repaint_call(r), **negatives(r), true_cfg_scale=2.0)
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == (4, 1)          # begin index 1 + 3 steps
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, eager)
        assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == (4, 1)
    keys = graph_keys(pipe)
    assert len(keys) == 1 and solver_entries(keys[0]) == [("solver", 2)] and ("cfg", 2.0) in keys[0]
    # the background is still the source, bit for bit
    mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, gpu)
    assert torch.equal(eager[mask == 0], kw["image"][mask == 0])


# ------------------------------------------------------------------------------------------------------------------ 3. order 1
def test_solver_order_one_is_the_euler_call(gpu):
    pipe, r = random_pipe(gpu, 931)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, steps=4), **negatives(r), true_cfg_scale=2.0)
    want = pipe(**kw).images.clone()
    multistep(pipe, solver_order=1)
    assert torch.equal(pipe(**kw).images, want)
    multistep(pipe, solver_order=2)
    assert not torch.equal(pipe(**kw).images, want)
    pipe.capture_graphs = True
    keys_before = graph_keys(pipe)
    multistep(pipe, solver_order=1)
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw).images, want)
        assert (pipe.scheduler._step_index, pipe.scheduler._history_len) == (4, 0)          # what the Euler methods leave
    new = [k for k in graph_keys(pipe) if k not in keys_before]
    assert len(new) == 1 and not solver_entries(new[0])                     # order 1 builds the Euler key


# ------------------------------------------------------------------------------------------------------------------ 4. batch
def test_batch_of_two_is_two_calls(gpu):
    pipe, r = random_pipe(gpu, 941)
    multistep(pipe)
    pipe.capture_graphs = False
    kw = two_line_call(r, steps=4, B=2)
    kw["control_mask"] = [torch.cat([token_mask(a), token_mask(b)]).to(gpu, BF16) for a, b in
                          (((48, 96, 30, 200), (64, 112, 10, 120)), ((100, 150, 60, 240), (90, 140, 100, 250)))]
    both = pipe(**kw).images.clone()
    assert not torch.equal(both[0], both[1])
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k in ("control_image", "control_mask") else v)
               for k, v in kw.items()}
        assert torch.equal(pipe(**one).images, both[b : b + 1]), b


# ------------------------------------------------------------------------------------------------------------------ 5. toggles
def test_overlap_and_row_window_are_bitwise_neutral(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 951)
    multistep(pipe)
    pipe.capture_graphs = False
    kw = two_line_call(r, steps=4, cn_steps=3)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    serial = pipe(**kw).images.clone()
    assert pipe._tower_window_used is not None
    monkeypatch.setattr(P, "OVERLAP_TOWER", True)
    assert torch.equal(pipe(**kw).images, serial)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    for overlap in (False, True):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        assert torch.equal(pipe(**kw).images, serial)
        assert pipe._tower_window_used is None


# ------------------------------------------------------------------------------------------------------------------ 6. callback
def test_a_callback_that_returns_the_latents_makes_the_next_step_first_order(gpu):
    """The callback at step 1 hands the (bf16) latents back: the loop takes them as its new state and empties the history, so step 2 is
    first order. The reference is the same call with a scheduler that ignores the loop's ``reset_history`` and is told to take step 2
    with w = 0; the same scheduler without that instruction — step 2 second order on the velocity of step 1 — gives another result."""
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    class Deaf(FlowMatchMultistepScheduler):
        first_order_at = ()

        def reset_history(self):
            if self._step_index is None:                 # from set_timesteps, before the loop: as usual
                super().reset_history()

        def _advance_weight(self):
            sigma, sigma_next, w = super()._advance_weight()
            return sigma, sigma_next, 0.0 if self._step_index - 1 in self.first_order_at else w

    pipe, r = random_pipe(gpu, 961)
    kw = two_line_call(r, steps=4)
    calls = []

    def hand_back(p, i, t, env):
        calls.append(i)
        return {"latents": env["latents"]} if i == 1 else {}

    multistep(pipe)
    got = pipe(**kw, callback_on_step_end=hand_back).images.clone()
    assert calls == [0, 1, 2, 3] and (pipe.scheduler._step_index, pipe.scheduler._history_len) == (4, 1)
    pipe.scheduler = Deaf.from_config(pipe.scheduler.config)
    pipe.scheduler.first_order_at = (2,)
    want = pipe(**kw, callback_on_step_end=hand_back).images.clone()
    pipe.scheduler.first_order_at = ()
    stale = pipe(**kw, callback_on_step_end=hand_back).images.clone()
    assert torch.equal(got, want) and not torch.equal(got, stale)
    # a callback that returns nothing changes nothing
    multistep(pipe)
    pipe.capture_graphs = False
    plain = pipe(**kw).images.clone()
    assert torch.equal(pipe(**kw, callback_on_step_end=lambda p, i, t, env: {}).images, plain) and not torch.equal(plain, got)
