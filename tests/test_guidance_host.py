"""The host side of a guider on a true-CFG call (reptext_amd/guidance.py): the interval's known answers, the refusals, the two
properties, the three entries in the header and their refusals without a device, the rule on hand-made vectors in fp64, the reference
loop's two identities (tests/loop_reference.py) and what ``_generate`` hands to the loop. No kernel runs here."""
import ctypes as C
import math

import pytest
import torch

from oracle import flux_oracle as orc

from loop_reference import denoise_loop_reference, projected_velocity

BF16 = torch.bfloat16
SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_layers=2, num_single_layers=1, extra_condition_channels=64)


# ------------------------------------------------------------------------------------------------------------------ 1. the dataclass
def test_guided_steps_known_answers():
    from reptext_amd.guidance import TrueCFGGuider, guided_steps
    from reptext_amd.pipeline import union_active_steps

    assert guided_steps(4, TrueCFGGuider(0.0, 0.5)) == (0, 1)
    assert guided_steps(28, TrueCFGGuider(0.0, 0.6)) == tuple(range(16))
    assert guided_steps(4, TrueCFGGuider(0.0, 0.0)) == ()
    assert guided_steps(4, TrueCFGGuider(0.5, 1.0)) == (2, 3)
    assert guided_steps(4, TrueCFGGuider()) == (0, 1, 2, 3)
    for n, a, b in ((7, 0.2, 0.9), (28, 0.33, 0.34), (1, 0.0, 1.0), (5, 0.4, 0.4)):
        assert guided_steps(n, TrueCFGGuider(a, b)) == union_active_steps(n, a, b)


@pytest.mark.parametrize("bad", [dict(start=-0.1), dict(stop=1.1), dict(start=1.5, stop=2.0), dict(start=0.6, stop=0.5), dict(norm_threshold=-1.0),
                                 dict(eta=math.nan), dict(eta=math.inf), dict(start=math.nan), dict(stop=math.nan), dict(norm_threshold=math.inf),
                                 dict(momentum=math.nan), dict(momentum=1.0), dict(momentum=-1.0), dict(momentum=-3.0)])
def test_post_init_refuses(bad):
    from reptext_amd.guidance import TrueCFGGuider

    with pytest.raises(ValueError):
        TrueCFGGuider(**bad)


def test_projected_and_whole():
    from reptext_amd.guidance import TrueCFGGuider

    g = TrueCFGGuider()
    assert (g.start, g.stop, g.eta, g.norm_threshold, g.momentum) == (0.0, 1.0, 1.0, 0.0, 0.0)
    assert not g.projected and g.whole
    for dev in (dict(eta=0.0), dict(eta=1.5), dict(norm_threshold=2.5), dict(momentum=-0.5), dict(momentum=0.25)):
        assert TrueCFGGuider(**dev).projected and TrueCFGGuider(**dev).whole, dev
    for dev in (dict(start=0.1), dict(stop=0.9), dict(stop=0.0)):
        assert not TrueCFGGuider(**dev).projected and not TrueCFGGuider(**dev).whole, dev
    with pytest.raises(Exception):
        g.eta = 0.0                                                   # frozen


def test_loop_guidance_is_none_unless_the_guider_changes_a_cfg_call():
    from reptext_amd.guidance import Guidance, TrueCFGGuider, loop_guidance

    assert loop_guidance(None, True, 4) is None
    assert loop_guidance(TrueCFGGuider(), True, 4) is None
    assert loop_guidance(TrueCFGGuider(stop=0.5, eta=0.0), False, 4) is None          # no negative prompt: ignored
    assert loop_guidance(TrueCFGGuider(stop=0.5), True, 4) == Guidance(TrueCFGGuider(stop=0.5), (0, 1))
    assert loop_guidance(TrueCFGGuider(eta=0.0), True, 3) == Guidance(TrueCFGGuider(eta=0.0), (0, 1, 2))
    with pytest.raises(ValueError):
        loop_guidance("apg", True, 4)


# ------------------------------------------------------------------------------------------------------------------ 2. the attribute
def test_the_guider_is_a_plain_attribute():
    import inspect

    from reptext_amd.pipeline import CallExtensions, FluxControlNetPipeline, LoopExtras
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, None, None)
    assert pipe.guider is None and "guider" not in pipe.components
    assert "guider" not in inspect.signature(FluxControlNetPipeline.__init__).parameters
    assert "guider" not in inspect.signature(FluxControlNetPipeline.__call__).parameters
    assert len(CallExtensions.__dataclass_fields__) == 13
    assert LoopExtras().guidance is None


def test_the_inpaint_pipeline_refuses_a_guider_before_any_device_work():
    from reptext_amd.guidance import TrueCFGGuider
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as Inpaint
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    pipe = Inpaint(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, None, None, None)
    pipe.guider = TrueCFGGuider(stop=0.5)
    with pytest.raises(ValueError, match="guider"):
        pipe(prompt_embeds=torch.zeros(1, 8, 256), pooled_prompt_embeds=torch.zeros(1, 64), height=64, width=64, num_inference_steps=1)


# ------------------------------------------------------------------------------------------------------------------ 3. binding, refusals
def test_the_header_declares_the_three_entries():
    from reptext_amd import native

    P, F, I64, I32 = C.c_void_p, C.c_float, C.c_int64, C.c_int32
    assert native.SIGNATURES["rt_guidance_ws_bytes"] == [I32, I64] and native.RESTYPES["rt_guidance_ws_bytes"] is I64
    # v_uncond, v_text, diff | beta | partials | B, n_s | stream
    assert native.SIGNATURES["rt_guidance_reduce_f32"] == [P, P, P, F, P, I32, I64, P]
    # x, v_uncond, v_text, x_bf16, diff, partials | s − 1, eta, tau | hist | w | src, noise, mask | dsigma, sigma_next | B, n_s, n_mask | stream
    assert native.SIGNATURES["rt_projected_step_f32"] == [P] * 6 + [F] * 3 + [P, F] + [P] * 3 + [F, F] + [I32, I64, I64, P]
    assert native.RESTYPES["rt_guidance_reduce_f32"] is C.c_int and native.RESTYPES["rt_projected_step_f32"] is C.c_int
    assert native.RT_GUIDE_CHUNK == 4096 and native.ABI_VERSION == 15


def test_entry_point_refusals():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                       # never dereferenced: every call is refused first
    ws = lib.rt_guidance_ws_bytes
    assert (ws(1, 64), ws(2, 4096), ws(3, 4160), ws(2, 12289), ws(1, 16384 * 4), ws(0, 64), ws(1, 0)) == (12, 24, 72, 96, 16 * 12, 0, 0)

    def reduce(u=P, t=P, diff=P, part=P, B=2, n_s=64):
        return lib.rt_guidance_reduce_f32(u, t, diff, 0.0, part, B, n_s, None)

    for name in ("u", "t", "diff", "part"):
        assert reduce(**{name: None}) == native.RT_E_BADARG == -1, name
    assert reduce(B=0) == -1 and reduce(n_s=0) == -1 and reduce(B=-1) == -1
    assert reduce(B=65536) == native.RT_E_SHAPE

    def step(x=P, u=P, t=P, xb=None, diff=P, part=P, hist=None, src=None, noise=None, mask=None, B=2, n_s=64, n_mask=128):
        return lib.rt_projected_step_f32(x, u, t, xb, diff, part, 1.0, 0.0, 0.0, hist, 0.5, src, noise, mask, -0.01, 0.5, B, n_s, n_mask, None)

    for name in ("x", "u", "t", "diff", "part"):
        assert step(**{name: None}) == -1, name
        assert step(**{name: None}, xb=P, hist=P, src=P, noise=P, mask=P) == -1, name
    assert step(B=0) == -1 and step(n_s=0) == -1 and step(n_mask=0) == -1
    assert step(mask=P) == -1 and step(mask=P, src=P) == -1 and step(mask=P, noise=P) == -1
    assert step(mask=P, src=P, noise=P, n_mask=48) == native.RT_E_SHAPE and step(n_mask=100) == native.RT_E_SHAPE
    assert step(B=65536, n_mask=65536 * 64) == native.RT_E_SHAPE
    with pytest.raises(native.NativeCallError, match="rt_projected_step_f32 failed: RT_E_BADARG"):
        native.call("rt_projected_step_f32", P, P, P, None, None, P, 1.0, 0.0, 0.0, None, 0.0, None, None, None, 0.0, 0.0, 1, 8, 8, None)
    with pytest.raises(native.NativeCallError, match="rt_guidance_reduce_f32 failed: RT_E_BADARG"):
        native.call("rt_guidance_reduce_f32", P, P, P, 0.0, None, 1, 8, None)


def test_ops_refuse_shapes_that_do_not_fit():
    """Argument checks of ops.projected_step_f32_: raised before the device is touched."""
    from reptext_amd import ops

    assert ops.guidance_partials_shape(2, 4096) == (2, 1, 3) and ops.guidance_partials_shape(3, 4097) == (3, 2, 3)
    x, v = torch.zeros(2, 8), torch.zeros(2, 8, dtype=BF16)
    ok = dict(x32=x, v_uncond=v, v_text=v.clone(), diff32=x.clone(), partials=torch.zeros(2, 1, 3), s=2.0, eta=0.0, norm_threshold=1.0, beta=0.0,
              dsigma=-0.1)
    rp = dict(sigma_next=0.5, src32=x.clone(), noise32=x.clone(), mask=torch.zeros(1, 8))
    for bad in (dict(v_uncond=torch.zeros(2, 4, dtype=BF16)), dict(v_text=torch.zeros(1, 8, dtype=BF16)), dict(diff32=torch.zeros(2, 4)),
                dict(diff32=torch.zeros(8, 2).t()), dict(partials=torch.zeros(2, 3)), dict(partials=torch.zeros(1, 1, 3)), dict(partials=torch.zeros(2, 2, 3)),
                dict(x32=torch.zeros(16), v_uncond=torch.zeros(16, dtype=BF16), v_text=torch.zeros(16, dtype=BF16), diff32=torch.zeros(16)),
                dict(hist32=torch.zeros(2, 4)), dict(x_bf16=torch.zeros(2, 4, dtype=BF16)),
                dict(rp, mask=torch.zeros(2, 4)), dict(rp, mask=torch.zeros(8)), dict(rp, src32=torch.zeros(2, 4)), dict(rp, src32=None), dict(rp, noise32=None)):
        with pytest.raises(ValueError):
            ops.projected_step_f32_(**{**ok, **bad})
    for good in (ok, {**ok, **rp}, dict(ok, hist32=x.clone(), w=0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.projected_step_f32_(**good)


def test_step_master_projected_needs_true_cfg():
    from reptext_amd.guidance import ProjectedStep
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    x = torch.zeros(1, 8)
    rec = ProjectedStep(0.0, 0.0, -0.5, x.clone(), torch.zeros(1, 1, 3))
    for sc, kw in ((FlowMatchEulerDiscreteScheduler(), {}), (FlowMatchMultistepScheduler(), dict(history=x.clone()))):
        sc.set_timesteps(sigmas=[1.0, 0.5], mu=1.0)
        with pytest.raises(ValueError, match="v_text"):
            sc.step_master_(torch.zeros(1, 8, dtype=BF16), x, projected=rec, **kw)


# ------------------------------------------------------------------------------------------------------------------ 4. the rule, fp64
def rule_by_hand(p, u, r_prev, beta, s, eta, tau):
    """The block of the issue's §1 on Python lists, one sample."""
    d = [pi - ui + (beta * ri if beta else 0.0) for pi, ui, ri in zip(p, u, r_prev or [0.0] * len(p))]
    a, b, c = sum(x * x for x in d), sum(x * y for x, y in zip(d, p)), sum(y * y for y in p)
    k = tau / math.sqrt(a) if tau > 0 and a > tau * tau else 1.0
    alpha = k * b / c if c > 0 else 0.0
    e = (eta - 1.0) * alpha
    return [pi + (s - 1.0) * (k * di + e * pi) for pi, di in zip(p, d)], d


def test_the_rule_on_hand_made_vectors():
    t64 = lambda v: torch.tensor([v], dtype=torch.float64)
    # d ⟂ p: v = p + (s − 1)·k·d, whatever eta
    p, d = [1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 3.0, -4.0]
    u = [pi - di for pi, di in zip(p, d)]
    for eta in (0.0, 1.0, 0.3):
        for tau, k in ((0.0, 1.0), (10.0, 1.0), (2.5, 0.5)):               # ‖d‖ = 5
            v, dd = projected_velocity(t64(p), t64(u), None, 0.0, 3.0, eta, tau)
            assert torch.allclose(v, t64([pi + 2.0 * k * di for pi, di in zip(p, d)]), rtol=0, atol=1e-15) and torch.equal(dd, t64(d))
            assert torch.allclose(v, t64(rule_by_hand(p, u, None, 0.0, 3.0, eta, tau)[0]), rtol=0, atol=1e-15)
    # d = p / 2 and eta = 0: all of d is parallel to p and is dropped, v = p
    p = [1.0, -2.0, 0.5, 4.0]
    u = [pi / 2 for pi in p]
    for tau in (0.0, 0.25):
        v, _ = projected_velocity(t64(p), t64(u), None, 0.0, 4.0, 0.0, tau)
        assert torch.allclose(v, t64(p), rtol=0, atol=1e-15)
    # eta = 1, no clamp, no momentum: the plain mix u + s·(p − u)
    g = torch.Generator().manual_seed(5)
    P_, U_ = torch.randn(3, 40, generator=g, dtype=torch.float64), torch.randn(3, 40, generator=g, dtype=torch.float64)
    v, d = projected_velocity(P_, U_, None, 0.0, 2.5, 1.0, 0.0)
    assert torch.allclose(v, U_ + 2.5 * (P_ - U_), rtol=0, atol=1e-14)
    # momentum: d = (p − u) + beta·r_prev, per sample against the list version
    R_ = torch.randn(3, 40, generator=g, dtype=torch.float64)
    v, d = projected_velocity(P_, U_, R_, -0.5, 2.5, 0.25, 3.0)
    for b in range(3):
        hv, hd = rule_by_hand(P_[b].tolist(), U_[b].tolist(), R_[b].tolist(), -0.5, 2.5, 0.25, 3.0)
        assert torch.allclose(v[b], torch.tensor(hv, dtype=torch.float64), rtol=0, atol=1e-13)
        assert torch.allclose(d[b], torch.tensor(hd, dtype=torch.float64), rtol=0, atol=1e-15)
    # p = 0: alpha = 0, no division
    v, _ = projected_velocity(torch.zeros(1, 4, dtype=torch.float64), t64([1.0, 0.0, 0.0, 0.0]), None, 0.0, 2.0, 0.0, 0.0)
    assert torch.equal(v, t64([-1.0, 0.0, 0.0, 0.0]))


# ------------------------------------------------------------------------------------------------------------------ 5. the reference loop
def test_the_reference_loop_reduces_to_the_cfg_loop_and_to_the_plain_loop():
    from reptext_amd.guidance import TrueCFGGuider

    N, T = 64, 16
    tp = orc.init_mmdit_params(SMALL_T, seed=901)
    cp = orc.init_mmdit_params(SMALL_CN, seed=902, controlnet=True)
    g = torch.Generator().manual_seed(903)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).float()
    pe, pooled, npe, npooled, hint, lat0 = r(1, T, 256), r(1, 64), r(1, T, 256), r(1, 64), r(1, N, 128), r(1, N, 64)
    rm = (torch.arange(N) % 3 == 0).float().reshape(1, N, 1)
    sig = orc.flow_sigmas(2, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    ids = orc.latent_image_ids(16, 16)
    args = (tp, SMALL_T, cp, SMALL_CN, lat0, pe, pooled, [hint], [rm], sig, ids, torch.zeros(T, 3), 3.5)
    kw = dict(conditioning_step=1, negative=dict(prompt_embeds=npe, pooled=npooled, scale=2.0))
    with orc.stored_as(BF16):
        cfg = denoise_loop_reference(*args, **kw)
        same = denoise_loop_reference(*args, **kw, guider=TrueCFGGuider())
        plain = orc.denoise_loop(*args, conditioning_step=1)
        empty = denoise_loop_reference(*args, **kw, guider=TrueCFGGuider(stop=0.0, eta=0.0, momentum=-0.5))
        info = {}
        half = denoise_loop_reference(*args, **kw, guider=TrueCFGGuider(stop=0.5, eta=0.0), info=info)
    assert torch.equal(same, cfg) and torch.equal(empty, plain)
    assert not torch.equal(cfg, plain) and not torch.equal(half, cfg) and not torch.equal(half, plain)
    assert len(info["norm_d"]) == 1 and float(info["norm_d"][0]) > 0
