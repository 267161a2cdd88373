"""Host side of the second-order multistep scheduler (reptext_amd.scheduler.FlowMatchMultistepScheduler): the weights' known answers,
the convergence order of the rule on a problem with an exact velocity, the config and the loader / saver, the derived binding of
rt_multistep_step_f32 and the op's refusals. No kernel runs here.

The convergence test integrates the flow-matching ODE of a 1-D mixture of two Gaussians, whose velocity is known in closed form, in
fp64 on the FLUX grid (mu = 1.15) and compares with a 4096-step run of the same rule. With x_σ = (1 − σ)·x0 + σ·ε, ε ~ N(0, 1) and
x0 ~ Σ_k π_k N(m_k, s_k²), the marginal at σ is Σ_k π_k N((1 − σ)·m_k, (1 − σ)²·s_k² + σ²) and the velocity dx/dσ = E[ε − x0 | x_σ] is
the responsibility-weighted sum of the per-component conditional means. A first-order rule halves its error when the steps double
(ratio 2 in the limit), a second-order one quarters it; the bounds asked are 3 from below for the second-order rule and 2.5 from
above for Euler, and the second-order rule at 14 steps is to lie below Euler at 56.

The mixture is the one those conditions were first checked on, recovered from the six figures recorded with them (Euler 2.07e-1,
1.24e-1, 7.14e-2 and AB2 4.30e-2, 8.43e-3, 1.75e-3 at 14, 28 and 56 steps): only the weights, the distance between the means and the
widths matter (a common shift of the means changes nothing that is measured, so the means are centred), and on a grid of weights
0.2 .. 0.5, distances 1 .. 6 and widths 0.1 .. 1.0 the closest point is weights 0.3 / 0.7, means -1.75 / +1.75, widths 0.3 / 0.4. It
gives Euler 2.07e-1, 1.24e-1, 7.63e-2 (ratios 1.67, 1.62) and AB2 4.81e-2, 8.43e-3, 2.08e-3 (ratios 5.71, 4.05) over the 4096 start
points drawn here; what is left of the difference is the draw. A mixture with the modes closer together (distance 2.5, widths 0.3 /
0.5) keeps the orders (4.94, 4.73 and 1.83, 1.91) but is smooth enough for Euler to reach its asymptotic rate early, and there the
second-order rule at 14 steps (4.56e-2) is NOT below Euler at 56 (3.28e-2): the last condition is a statement about this mixture, not
about every one."""
import ctypes as C
import functools
import json
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_reference as lref  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402
from test_union_tower_host import call_kwargs, make_pipe  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------ 1. the weights
def test_weights_on_a_uniform_grid_are_zero_then_one_half():
    from reptext_amd.scheduler import multistep_weights

    sig = torch.linspace(1.0, 0.0, 9, dtype=F32)                # 1/8 steps: exact in fp32
    assert multistep_weights(sig) == [0.0] + [0.5] * 7
    assert multistep_weights(sig.tolist()) == [0.0] + [0.5] * 7


def test_weights_on_the_flux_grid_and_with_a_begin_index():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, calculate_shift, multistep_weights

    sc = FlowMatchEulerDiscreteScheduler()
    mu = calculate_shift(256, 256, 4096, 0.5, 1.15)
    assert mu == 0.5
    sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=mu)
    s = [float(x) for x in sc.sigmas]
    # σ = e^µ / (e^µ + 1/t − 1) at t = 1, 3/4, 1/2, 1/4 and the trailing 0, from the formula in fp64: the fp32 table is within 2^-24 of it
    e = math.exp(0.5)
    exact = [e / (e + 1.0 / t - 1.0) for t in (1.0, 0.75, 0.5, 0.25)] + [0.0]
    assert len(s) == 5 and all(abs(a - b) <= 2.0 ** -24 for a, b in zip(s, exact))
    w = multistep_weights(sc.sigmas)
    want = [0.0] + [(s[i + 1] - s[i]) / (2.0 * (s[i] - s[i - 1])) for i in (1, 2, 3)]
    assert w == want == lref.weights(sc.sigmas)
    # against the closed form: each dσ carries two table roundings of 2^-24 against a difference of at least 0.16
    for i in (1, 2, 3):
        assert abs(w[i] - (exact[i + 1] - exact[i]) / (2.0 * (exact[i] - exact[i - 1]))) < 1e-5
    assert all(0.3 < x < 1.1 for x in w[1:]) and len({round(x, 3) for x in w[1:]}) == 3          # a non-uniform grid: three weights
    # begin = 1: the run starts at step 1, which is first order; step 0 does not run
    assert multistep_weights(sc.sigmas, begin=1) == [0.0, 0.0] + want[2:] == lref.weights(sc.sigmas, 1)
    assert multistep_weights(sc.sigmas, begin=3) == [0.0] * 4


def test_order_one_is_all_zero_and_other_orders_are_refused():
    from reptext_amd.scheduler import FlowMatchMultistepScheduler, multistep_weights

    sig = [1.0, 0.7, 0.3, 0.0]
    assert multistep_weights(sig, order=1) == [0.0] * 3 == lref.weights(sig, order=1)
    for order in (0, 3, 4):
        with pytest.raises(ValueError, match="order"):
            multistep_weights(sig, order=order)
    with pytest.raises(ValueError, match="solver_order"):
        FlowMatchMultistepScheduler(solver_order=3)


# ------------------------------------------------------------------------------------------------------------------ 2. convergence order
PI, MEAN, STD = (0.3, 0.7), (-1.75, 1.75), (0.3, 0.4)


def toy_velocity(x, sigma):
    """dx/dσ of the two-Gaussian flow: Σ_k r_k(x)·E[ε − x0 | x_σ = x, k], fp64."""
    a = 1.0 - sigma
    logp, cond = [], []
    for p, m, s in zip(PI, MEAN, STD):
        var = a * a * s * s + sigma * sigma
        d = x - a * m
        logp.append(math.log(p) - 0.5 * torch.log(torch.tensor(var, dtype=torch.float64)) - 0.5 * d * d / var)
        cond.append(-m + (sigma - a * s * s) / var * d)           # E[ε | ·] − E[x0 | ·] = σ·d/var − (m + a·s²·d/var)
    r = torch.softmax(torch.stack(logp), dim=0)
    return (r * torch.stack(cond)).sum(0)


def flux_grid(n, mu=1.15):
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    sc = FlowMatchEulerDiscreteScheduler()
    sc.set_timesteps(sigmas=torch.linspace(1.0, 1.0 / n, n).tolist(), mu=mu)
    return sc.sigmas.double()


@functools.lru_cache(maxsize=None)
def toy_errors():
    """(AB2, Euler): RMS error over 4096 start points drawn from N(0, 1) at 14, 28 and 56 steps against the 4096-step AB2 run."""
    x0 = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    exact = lref.integrate(toy_velocity, x0, flux_grid(4096))
    assert bool(torch.isfinite(exact).all()) and float(exact.std()) > 0.5
    rms = lambda x: float((x - exact).pow(2).mean().sqrt())
    ab2 = {n: rms(lref.integrate(toy_velocity, x0, flux_grid(n))) for n in (14, 28, 56)}
    euler = {n: rms(lref.integrate(toy_velocity, x0, flux_grid(n), order=1)) for n in (14, 28, 56)}
    print(f"[multistep toy] AB2 {ab2}, ratios {ab2[14] / ab2[28]:.2f} {ab2[28] / ab2[56]:.2f}; Euler {euler}, ratios "
          f"{euler[14] / euler[28]:.2f} {euler[28] / euler[56]:.2f}")
    return ab2, euler


def test_the_rule_is_second_order_on_the_flux_grid():
    ab2, euler = toy_errors()
    assert ab2[14] / ab2[28] >= 3 and ab2[28] / ab2[56] >= 3
    assert euler[14] / euler[28] <= 2.5 and euler[28] / euler[56] <= 2.5


def test_fourteen_multistep_steps_are_below_fifty_six_euler_steps():
    ab2, euler = toy_errors()
    assert ab2[14] < euler[56]


def test_the_scheduler_walks_the_rule_of_the_reference(monkeypatch):
    """The scheduler's host side — index, weight, history count — against ``integrate`` with the op replaced by its fp32 formula on the
    CPU: the op itself is tested on the GPU."""
    from reptext_amd import ops
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    seen = []

    def op(name, x32, v, v_text, s, dsigma, x_bf16=None, *, hist, w, **kw):
        assert kw.get("mask") is None and v_text is None
        vel = v.float()
        x32 += dsigma * (vel + w * (vel - hist) if w != 0.0 else vel)
        hist.copy_(vel)
        seen.append(w)

    monkeypatch.setattr(ops, "_master_step_f32", op)                # the one body every step of ``step_master_`` goes through
    sc = FlowMatchMultistepScheduler()
    sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=0.5)
    x = torch.randn(2, 16, generator=torch.Generator().manual_seed(1))
    field = lambda x, sigma: torch.sin(3.0 * x) + sigma
    hist = torch.full_like(x, float("nan"))
    state = x.clone()
    for i in range(4):
        sc.step_master_(field(state, float(sc.sigmas[i])), state, history=hist)
        assert sc.step_index == i + 1
    assert seen == lref.weights(sc.sigmas) and bool(torch.isfinite(state).all())
    want = lref.integrate(field, x.double(), sc.sigmas)
    assert float((state.double() - want).abs().max()) < 1e-5
    # step_master_ without a history is refused; reset_history, set_begin_index and set_timesteps make the next step first order
    with pytest.raises(ValueError, match="history"):
        sc.step_master_(x.to(BF16), state)
    for reset in (sc.reset_history, lambda: sc.set_begin_index(1), lambda: sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=0.5)):
        sc._step_index, sc._history_len = 2, 1
        reset()
        assert sc._history_len == 0
        sc._step_index = 2
        seen.clear()
        sc.step_master_(x.to(BF16), state, history=hist)
        sc.step_master_(x.to(BF16), state, history=hist)
        assert seen == [0.0, lref.weights(sc.sigmas)[3]]


# ------------------------------------------------------------------------------------------------------------------ 3. config, loader, saver
def test_class_attributes_and_from_config():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    assert issubclass(FlowMatchMultistepScheduler, FlowMatchEulerDiscreteScheduler) and FlowMatchMultistepScheduler.order == 1
    ms = FlowMatchMultistepScheduler()
    assert ms.config.solver_order == 2 == ms.solver_order and not hasattr(FlowMatchEulerDiscreteScheduler(), "solver_order")
    euler = FlowMatchEulerDiscreteScheduler(max_shift=1.3)
    swapped = FlowMatchMultistepScheduler.from_config(euler.config)              # pipe.scheduler = X.from_config(pipe.scheduler.config)
    assert swapped.config == dict(euler.config, solver_order=2) and swapped.config.max_shift == 1.3
    # keys of other diffusers schedulers and private keys are ignored
    other = dict(euler.config, _class_name="DPMSolverMultistepScheduler", algorithm_type="dpmsolver++", use_karras_sigmas=False, solver_order=1)
    assert FlowMatchMultistepScheduler.from_config(other).config == dict(euler.config, solver_order=1)
    # the grid is the Euler scheduler's, and so is what retrieve_timesteps inspects
    import inspect
    assert inspect.signature(swapped.set_timesteps) == inspect.signature(euler.set_timesteps)
    assert inspect.signature(swapped.set_begin_index) == inspect.signature(euler.set_begin_index)
    for sc in (euler, swapped):
        sc.set_timesteps(sigmas=[1.0, 0.6, 0.3], mu=0.7)
    assert torch.equal(euler.sigmas, swapped.sigmas) and torch.equal(euler.timesteps, swapped.timesteps)
    x, nz = torch.randn(4), torch.randn(4)
    assert torch.equal(euler.scale_noise(x, 0.4, nz), swapped.scale_noise(x, 0.4, nz))


def _fake_vae():
    return SimpleNamespace(config=SimpleNamespace(block_out_channels=[1] * 4))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_save_and_load_keep_the_class_and_the_order(tmp_path, capfd):
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    pipe = make_pipe(union=None)
    load = lambda d: FluxControlNetPipeline.from_pretrained(str(d), transformer=pipe.transformer, vae=_fake_vae(), controlnet=pipe.controlnet)
    # the Euler pipeline writes what it wrote: the bytes of the parent commit's saver, restated
    pipe.save_pretrained(str(tmp_path / "euler"))
    want = json.dumps(dict(_class_name="FlowMatchEulerDiscreteScheduler", **dict(pipe.scheduler.config)), indent=2).encode()
    assert _read(tmp_path / "euler" / "scheduler" / "scheduler_config.json") == want
    assert want == (b'{\n  "_class_name": "FlowMatchEulerDiscreteScheduler",\n  "num_train_timesteps": 1000,\n  "shift": 3.0,\n'
                    b'  "use_dynamic_shifting": true,\n  "base_shift": 0.5,\n  "max_shift": 1.15,\n  "base_image_seq_len": 256,\n'
                    b'  "max_image_seq_len": 4096\n}')
    index = json.loads(_read(tmp_path / "euler" / "model_index.json"))
    assert index["scheduler"] == ["reptext_amd", "FlowMatchEulerDiscreteScheduler"]
    assert type(load(tmp_path / "euler").scheduler) is FlowMatchEulerDiscreteScheduler
    # the multistep pipeline: class name in both files, solver_order kept
    for order in (2, 1):
        pipe.scheduler = FlowMatchMultistepScheduler.from_config(dict(pipe.scheduler.config, solver_order=order, max_shift=1.2))
        d = tmp_path / f"multi{order}"
        pipe.save_pretrained(str(d))
        saved = json.loads(_read(d / "scheduler" / "scheduler_config.json"))
        assert saved["_class_name"] == "FlowMatchMultistepScheduler" and saved["solver_order"] == order
        assert json.loads(_read(d / "model_index.json"))["scheduler"] == ["reptext_amd", "FlowMatchMultistepScheduler"]
        back = load(d).scheduler
        assert type(back) is FlowMatchMultistepScheduler and back.config == pipe.scheduler.config and back.solver_order == order
    assert "not available" not in capfd.readouterr().err
    # an unknown class name keeps the Euler class, with a line on stderr
    saved["_class_name"] = "DPMSolverMultistepScheduler"
    with open(d / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(saved, f)
    back = load(d).scheduler
    assert type(back) is FlowMatchEulerDiscreteScheduler and back.config.max_shift == 1.2 and "solver_order" not in back.config
    assert "DPMSolverMultistepScheduler" in capfd.readouterr().err


def test_the_pipeline_module_exports_the_class():
    import reptext_amd.pipeline as P
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    assert P.FlowMatchMultistepScheduler is FlowMatchMultistepScheduler


# ------------------------------------------------------------------------------------------------------------------ 4. binding and op
def test_the_header_declares_the_entry():
    from reptext_amd import native

    sig = native.SIGNATURES["rt_multistep_step_f32"]
    # x, v, v_text, x_bf16, hist | w | src, noise, mask | s, dsigma, sigma_next | n, n_mask | stream
    assert sig == [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_int64] * 2 + [C.c_void_p]
    assert native.RESTYPES["rt_multistep_step_f32"] is C.c_int and native.ABI_VERSION == 15


def test_ops_refuse_shapes_that_do_not_fit():
    """Argument checks of ops.multistep_step_f32_, as the three other steps make them: raised before the device is touched."""
    from reptext_amd import ops

    x, v = torch.zeros(2, 8), torch.zeros(2, 8, dtype=BF16)
    ok = dict(x32=x, v=v, hist32=x.clone(), w=0.5, dsigma=-0.1)
    rp = dict(sigma_next=0.5, src32=x.clone(), noise32=x.clone(), mask=torch.zeros(1, 8))
    for bad in (dict(v=torch.zeros(2, 4, dtype=BF16)), dict(hist32=torch.zeros(2, 4)), dict(hist32=torch.zeros(8, 2).t()), dict(hist32=torch.zeros(16)),
                dict(v_text=torch.zeros(1, 8, dtype=BF16)), dict(x_bf16=torch.zeros(2, 4, dtype=BF16)),
                dict(rp, mask=torch.zeros(2, 4)), dict(rp, mask=torch.zeros(8)), dict(rp, src32=torch.zeros(2, 4)), dict(rp, src32=None),
                dict(rp, noise32=None)):
        with pytest.raises(ValueError):
            ops.multistep_step_f32_(**{**ok, **bad})
    for good in (ok, {**ok, **rp}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.multistep_step_f32_(**good)


def test_entry_point_refusals():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                       # never dereferenced: every call is refused first

    def call(x=P, v=P, vt=None, xb=None, hist=P, src=None, noise=None, mask=None, n=64, n_mask=64):
        return lib.rt_multistep_step_f32(x, v, vt, xb, hist, 0.5, src, noise, mask, 3.5, -0.01, 0.5, n, n_mask, None)

    for name in ("x", "v", "hist"):
        assert call(**{name: None}) == native.RT_E_BADARG == -1, name
        assert call(**{name: None}, vt=P, xb=P, src=P, noise=P, mask=P) == -1, name
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n_mask=0) == -1
    assert call(mask=P) == -1 and call(mask=P, src=P) == -1 and call(mask=P, noise=P) == -1
    assert call(mask=P, src=P, noise=P, n_mask=48) == native.RT_E_SHAPE and call(n=65, n_mask=64) == native.RT_E_SHAPE
    with pytest.raises(native.NativeCallError, match="rt_multistep_step_f32 failed: RT_E_BADARG"):
        native.call("rt_multistep_step_f32", P, P, None, None, None, 0.5, None, None, None, 1.0, 0.0, 0.0, 8, 8, None)
    with pytest.raises(native.NativeCallError, match="rt_multistep_step_f32 failed: RT_E_SHAPE"):
        native.call("rt_multistep_step_f32", P, P, None, None, P, 0.5, P, P, P, 1.0, 0.0, 0.0, 8, 3, None)


# ------------------------------------------------------------------------------------------------------------------ 5. the call
def test_a_call_starts_with_an_empty_history_and_leaves_nothing_on_the_pipeline():
    """The loop replaced by a recorder, as test_repaint_host.py does it: when the loop starts the scheduler's history is empty, even
    if the call before left it full, and after the call nothing of the history is on the pipeline."""
    from reptext_amd.scheduler import FlowMatchMultistepScheduler

    pipe = make_pipe(union=None, controlnet=False)
    pipe.scheduler = FlowMatchMultistepScheduler.from_config(pipe.scheduler.config)
    pipe.set_progress_bar_config(disable=True)
    seen = []

    def recorder(latents, *args, **kwargs):
        seen.append((pipe.scheduler._history_len, pipe.scheduler.solver_order))
        pipe._master_latents = latents.float()
        return latents

    pipe._denoise_eager = recorder
    before = set(pipe.__dict__)
    for _ in range(2):
        pipe.scheduler._history_len = 1
        pipe(**call_kwargs(control_image_union=None))
    assert seen == [(0, 2), (0, 2)]
    assert_no_call_state(pipe)
    assert not [k for k in set(pipe.__dict__) - before if "hist" in k or "solver" in k]
    assert not [k for k in pipe.scheduler.__dict__ if isinstance(pipe.scheduler.__dict__[k], torch.Tensor) and k not in ("timesteps", "sigmas")]
