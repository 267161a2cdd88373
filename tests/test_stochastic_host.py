"""Stochastic flow-match sampling without a device: the numpy restatement of the generator against Random123's known answers, the
scheduler's two config keys and refusals, the host function that names a call's noise streams, the rule on a 1-D flow in float64, the
binding and the ops' argument checks, and what a call hands to the loop. The kernels: tests/test_stochastic_step_kernel_gpu.py; the
pipelines: tests/test_stochastic_gpu.py."""
import ctypes as C
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as ph  # noqa: E402
from test_true_cfg_host import _kw, _pipe, assert_no_call_state  # noqa: E402
from test_union_tower_host import call_kwargs, make_pipe  # noqa: E402

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("counter, key, words", [
    ([0] * 4, [0] * 2, [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])])
def test_philox_known_answers(counter, key, words):
    """Random123's kat_vectors for philox4x32-10."""
    assert ph.philox4x32_10(counter, key).tolist() == words
    batch = ph.philox4x32_10([counter, [1, 2, 3, 4]], key)                   # vectorised: row 0 is the same call
    assert batch.shape == (2, 4) and batch[0].tolist() == words and batch[1].tolist() != words


def test_counter_and_key_layout():
    """counter = (g low, g high, step, subsequence), key = (seed low, seed high ^ DOMAIN): written out against the raw function."""
    seed, sub, step = 0x1234567890ABCDEF, 7, 11
    got = ph.group_words(seed, sub, step, 3, first_group=(1 << 32) - 1)
    for j, g in enumerate(((1 << 32) - 1, 1 << 32, (1 << 32) + 1)):
        want = ph.philox4x32_10([g & 0xFFFFFFFF, g >> 32, step, sub], [0x90ABCDEF, 0x12345678 ^ ph.DOMAIN])
        assert got[j].tolist() == want.tolist()
    assert ph.DOMAIN != 0                                                     # torch's own stream for the seed keys with the seed as it is
    # a negative int64 seed is its two's-complement bits
    assert ph.group_words(-1, 0, 0, 1).tolist() == ph.philox4x32_10([0, 0, 0, 0], [0xFFFFFFFF, 0xFFFFFFFF ^ ph.DOMAIN])[None].tolist()


def test_uniforms_and_normals_of_the_edge_words():
    u = ph.uniforms(np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2.0 ** 23 - 0.5) * 2.0 ** -24)                            # the last sum that is exact
    assert u[4] == np.float32((2.0 ** 23 + 2) * 2.0 ** -24) and u[5] == np.float32(1.0)  # 2^23 + 1.5 and 2^24 − 0.5: ties, to even
    z = ph.normals(np.array([[0, 0, 0xFFFFFFFF, 0x40000000]], dtype=np.uint32))
    assert abs(z[0, 0]) <= math.sqrt(2.0 * math.log(2.0 ** 25)) and abs(z[0, 0] - math.sqrt(2.0 * math.log(2.0 ** 25))) < 1e-6
    assert z[0, 2] == 0.0 and z[0, 3] == 0.0 and np.isfinite(z).all()                    # u = 1: r = 0, a finite draw


def test_moments_of_the_restatement():
    n = 4096 * 64
    z, z4 = ph.sample_normals(42, 0, 3, n), ph.sample_normals(42, 0, 4, n)
    stats = [abs(z.mean()) * math.sqrt(n), abs(z.var() - 1.0) * math.sqrt(n / 2), abs((z ** 4).mean() - 3.0) * math.sqrt(n / 96),
             abs((z[1:] * z[:-1]).sum()) / math.sqrt(n - 1), abs((z * z4).sum()) / math.sqrt(n)]
    assert max(stats) <= 1.5 and np.abs(z).max() <= math.sqrt(2.0 * math.log(2.0 ** 25))
    assert np.array_equal(ph.sample_normals(42, 0, 3, 1030), z[:1030])                   # an element does not depend on n_s


# ------------------------------------------------------------------------------------------------------------------ 2. config and refusals
def _fake_vae():
    return SimpleNamespace(config=SimpleNamespace(block_out_channels=[1] * 4))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_defaults_and_from_config():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    plain = FlowMatchEulerDiscreteScheduler()
    assert plain.stochastic_sampling is False and plain.stochastic_eta == 1.0
    assert "stochastic_sampling" not in plain.config and "stochastic_eta" not in plain.config          # a config as it always was
    assert FlowMatchEulerDiscreteScheduler(stochastic_sampling=False, stochastic_eta=1.0).config == plain.config
    on = FlowMatchEulerDiscreteScheduler(stochastic_sampling=True, stochastic_eta=0.5, max_shift=1.3)
    assert on.stochastic_sampling is True and on.stochastic_eta == 0.5 and on.config.stochastic_sampling is True and on.config.stochastic_eta == 0.5
    back = FlowMatchEulerDiscreteScheduler.from_config(on.config)
    assert back.config == on.config and back.stochastic_sampling and back.stochastic_eta == 0.5 and back.config.max_shift == 1.3
    # diffusers' saved config: its key alone
    theirs = FlowMatchEulerDiscreteScheduler.from_config(dict(plain.config, _class_name="FlowMatchEulerDiscreteScheduler", stochastic_sampling=True))
    assert theirs.stochastic_sampling and theirs.stochastic_eta == 1.0 and "stochastic_eta" not in theirs.config
    st = on.stochastic_step("rng")
    assert (st.rng, st.eta, st.sqrt_1m_eta2) == ("rng", 0.5, math.sqrt(0.75)) and theirs.stochastic_step(None).sqrt_1m_eta2 == 0.0
    # order 1 of the multistep class is the Euler scheduler's behaviour; order 2 refuses
    one = FlowMatchMultistepScheduler.from_config(dict(on.config, solver_order=1))
    assert one.stochastic_sampling and one.stochastic_eta == 0.5 and one.solver_order == 1
    with pytest.raises(ValueError, match="solver_order=1"):
        FlowMatchMultistepScheduler(stochastic_sampling=True)
    with pytest.raises(ValueError, match="solver_order=1"):
        FlowMatchMultistepScheduler.from_config(on.config)
    assert FlowMatchMultistepScheduler(stochastic_sampling=False).solver_order == 2


@pytest.mark.parametrize("eta", [0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")])
def test_eta_outside_its_interval_is_refused(eta):
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    with pytest.raises(ValueError, match="stochastic_eta"):
        FlowMatchEulerDiscreteScheduler(stochastic_sampling=True, stochastic_eta=eta)
    with pytest.raises(ValueError, match="stochastic_eta"):
        FlowMatchEulerDiscreteScheduler(stochastic_eta=eta)
    with pytest.raises(ValueError, match="stochastic_sampling"):
        FlowMatchEulerDiscreteScheduler(stochastic_sampling="yes")


def test_save_and_load_keep_the_keys_and_a_plain_config_keeps_its_bytes(tmp_path):
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    pipe = make_pipe(union=None)
    load = lambda d: FluxControlNetPipeline.from_pretrained(str(d), transformer=pipe.transformer, vae=_fake_vae(), controlnet=pipe.controlnet)
    pipe.save_pretrained(str(tmp_path / "euler"))
    assert _read(tmp_path / "euler" / "scheduler" / "scheduler_config.json") == (
        b'{\n  "_class_name": "FlowMatchEulerDiscreteScheduler",\n  "num_train_timesteps": 1000,\n  "shift": 3.0,\n'
        b'  "use_dynamic_shifting": true,\n  "base_shift": 0.5,\n  "max_shift": 1.15,\n  "base_image_seq_len": 256,\n'
        b'  "max_image_seq_len": 4096\n}')
    assert not load(tmp_path / "euler").scheduler.stochastic_sampling
    for cls, extra in ((FlowMatchEulerDiscreteScheduler, {}), (FlowMatchMultistepScheduler, dict(solver_order=1))):
        pipe.scheduler = cls.from_config(dict(pipe.scheduler.config, stochastic_sampling=True, stochastic_eta=0.25, **extra))
        d = tmp_path / cls.__name__
        pipe.save_pretrained(str(d))
        saved = json.loads(_read(d / "scheduler" / "scheduler_config.json"))
        assert saved["stochastic_sampling"] is True and saved["stochastic_eta"] == 0.25 and saved["_class_name"] == cls.__name__
        back = load(d).scheduler
        assert type(back) is cls and back.config == pipe.scheduler.config and back.stochastic_sampling and back.stochastic_eta == 0.25


# ------------------------------------------------------------------------------------------------------------------ 3. the rng function
def test_stochastic_rng_of_the_three_generator_forms():
    from reptext_amd.pipeline import stochastic_rng

    gens = [torch.Generator().manual_seed(s) for s in (11, 2 ** 63 + 5, 13)]
    for g in gens:
        torch.randn(3, generator=g)                                          # advanced: the INITIAL seed names the stream
    states = [g.get_state().clone() for g in gens]
    many = stochastic_rng(gens, 3)
    assert many.dtype == torch.int64 and many.shape == (3, 2) and many.device.type == "cpu" and many.is_contiguous()
    assert many.tolist() == [[11, 0], [2 ** 63 + 5 - 2 ** 64, 0], [13, 0]]            # a seed past 2^63: its bits as an int64
    for b, g in enumerate(gens):
        assert stochastic_rng(g, 1).tolist() == many[b : b + 1].tolist() == stochastic_rng([g], 1).tolist()      # sample b of a list is its own call
    assert stochastic_rng(gens[0], 3).tolist() == [[11, 0], [11, 1], [11, 2]]
    assert all(torch.equal(g.get_state(), s) for g, s in zip(gens, states))         # read, never advanced
    with pytest.raises(ValueError, match="generators"):
        stochastic_rng(gens, 2)
    # None: one draw from torch's default CPU generator, the same seed for every sample, a subsequence each
    torch.manual_seed(123)
    a = stochastic_rng(None, 2)
    after = torch.get_rng_state().clone()
    torch.manual_seed(123)
    b = stochastic_rng(None, 2)
    assert a.tolist() == b.tolist() and a[0, 0] == a[1, 0] >= 0 and a[:, 1].tolist() == [0, 1]
    torch.manual_seed(123)
    assert not torch.equal(torch.get_rng_state(), after)                             # the default generator moved
    torch.manual_seed(124)
    assert stochastic_rng(None, 2)[0, 0] != a[0, 0]


# ------------------------------------------------------------------------------------------------------------------ 4. the rule on a toy
M, SD = 1.5, 0.5          # the data: N(M, SD²) in one dimension; the state at sigma is (1 − σ)·x0 + σ·ε


def _velocity(x, sigma):
    """E[ε − x0 | x_σ = x] of the Gaussian flow, in closed form."""
    var = (1.0 - sigma) ** 2 * SD ** 2 + sigma ** 2
    centred = x - (1.0 - sigma) * M
    return sigma / var * centred - (M + (1.0 - sigma) * SD ** 2 / var * centred)


def _run(x, sigmas, eta, seed=42):
    """eta None: the Euler steps; else the stochastic rule, sample k drawing element k of the stream at every step."""
    for i in range(len(sigmas) - 1):
        s, sn = float(sigmas[i]), float(sigmas[i + 1])
        v = _velocity(x, s)
        x = x + (sn - s) * v if eta is None else ph.stochastic_rule(x, v, ph.sample_normals(seed, 0, i, x.size), s, sn, eta)
    return x


def test_the_rule_on_a_gaussian_flow_in_float64():
    """20 000 samples, 16 steps on a uniform sigma grid, float64.
    1. eta -> 0 is the Euler step: with ê in the noise's place r = x + (σ' − σ)·v algebraically, and the rule differs from it by
       σ'·(eta·z − (1 − sqrt(1 − eta²))·ê) per step: |x_eta − x_euler| is linear in eta. Asserted: the distance falls with eta, tenfold
       per decade within 5 % below eta = 0.1, and stays below 1.5·eta from eta = 0.01 down to 1e-12 (the restatement gives 1.146·eta:
       sixteen independent draws, each entering with its σ' and carried on by the flow's contraction).
    2. The order: distance(Euler, eta = 1e-3) < distance(Euler, eta = 0.3) < distance(Euler, eta = 1), per sample in the mean.
    Nothing is asserted about the law of the result: the rule re-noises the posterior MEAN, which is no sample of the data."""
    n, steps = 20000, 16
    sigmas = np.linspace(1.0, 0.0, steps + 1)
    x_start = ph.sample_normals(7, 0, 0, n)                                    # the state at sigma = 1 is the noise
    euler = _run(x_start, sigmas, None)
    dist = {eta: float(np.abs(_run(x_start, sigmas, eta) - euler).mean()) for eta in (1.0, 0.3, 0.1, 1e-2, 1e-3, 1e-4, 1e-12)}
    print("mean |x_eta - x_euler|:", dist)
    assert dist[1e-3] < dist[0.3] < dist[1.0]
    assert all(dist[a] > dist[b] for a, b in zip(list(dist), list(dist)[1:]))
    for a, b in ((0.1, 1e-2), (1e-2, 1e-3), (1e-3, 1e-4)):
        assert abs(dist[a] / dist[b] / 10.0 - 1.0) < 0.05, (a, b)
    assert all(dist[eta] < 1.5 * eta for eta in (1e-2, 1e-3, 1e-4, 1e-12))
    # the last step draws nothing: its result is the predicted clean image, whatever the noise
    x, v = x_start[:8], _velocity(x_start[:8], 0.25)
    assert np.array_equal(ph.stochastic_rule(x, v, np.full(8, np.nan), 0.25, 0.0, 0.5), x - 0.25 * v)


# ------------------------------------------------------------------------------------------------------------------ 5. binding and ops
def test_the_header_declares_the_entries():
    from reptext_amd import native

    p, f, i32, i64 = C.c_void_p, C.c_float, C.c_int32, C.c_int64
    # x, v, v_text, x_bf16, src, noise, mask, rng | s, sigma, sigma_next, eta, sqrt_1m_eta2 | step, B | n_s, n_mask | stream
    assert native.SIGNATURES["rt_stochastic_step_f32"] == [p] * 8 + [f] * 5 + [i32] * 2 + [i64] * 2 + [p]
    # x, v_uncond, v_text, x_bf16, diff, partials | s − 1, eta_guidance, tau | src, noise, mask, rng | sigma .. sqrt_1m_eta2 | step, B | ...
    assert native.SIGNATURES["rt_projected_stochastic_step_f32"] == [p] * 6 + [f] * 3 + [p] * 4 + [f] * 4 + [i32] * 2 + [i64] * 2 + [p]
    assert native.SIGNATURES["rt_normal_fill_f32"] == [p, p, i32, i64, i32, p]
    assert all(native.RESTYPES[n] is C.c_int for n in ("rt_stochastic_step_f32", "rt_projected_stochastic_step_f32", "rt_normal_fill_f32"))
    assert native.ABI_VERSION == 15                                          # added entries only


def test_entry_point_refusals():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                       # never dereferenced: every call is refused first
    BAD, SHAPE = native.RT_E_BADARG, native.RT_E_SHAPE

    def step(x=P, v=P, vt=None, xb=None, src=None, noise=None, mask=None, rng=P, sn=0.5, eta=1.0, step=0, B=2, n_s=64, n_mask=128):
        return lib.rt_stochastic_step_f32(x, v, vt, xb, src, noise, mask, rng, 3.5, 0.7, sn, eta, 0.0, step, B, n_s, n_mask, None)

    def proj(x=P, u=P, t=P, diff=P, part=P, mask=None, src=None, noise=None, rng=P, sn=0.5, eta=1.0, step=0, B=2, n_s=64, n_mask=128):
        return lib.rt_projected_stochastic_step_f32(x, u, t, None, diff, part, 2.5, 0.5, 0.0, src, noise, mask, rng, 0.7, sn, eta, 0.0, step, B,
                                                    n_s, n_mask, None)

    for name in ("x", "v", "rng"):
        assert step(**{name: None}) == BAD, name
    for name in ("x", "u", "t", "diff", "part", "rng"):
        assert proj(**{name: None}) == BAD, name
    for call in (step, proj):
        assert call(B=0) == BAD and call(n_s=0) == BAD and call(n_mask=0) == BAD and call(step=-1) == BAD
        assert call(eta=0.0) == BAD and call(eta=1.5) == BAD and call(eta=float("nan")) == BAD and call(eta=-0.5) == BAD
        assert call(mask=P) == BAD and call(mask=P, src=P) == BAD
        assert call(B=65536) == SHAPE and call(mask=P, src=P, noise=P, n_mask=48) == SHAPE
    assert lib.rt_normal_fill_f32(None, P, 2, 64, 0, None) == BAD and lib.rt_normal_fill_f32(P, None, 2, 64, 0, None) == BAD
    assert lib.rt_normal_fill_f32(P, P, 0, 64, 0, None) == BAD and lib.rt_normal_fill_f32(P, P, 2, 0, 0, None) == BAD
    assert lib.rt_normal_fill_f32(P, P, 2, 64, -1, None) == BAD and lib.rt_normal_fill_f32(P, P, 65536, 64, 0, None) == SHAPE


def test_ops_refuse_what_does_not_fit():
    """Raised before the device is touched; what fits reaches the device check."""
    from reptext_amd import ops

    x, v = torch.zeros(2, 8), torch.zeros(2, 8, dtype=BF16)
    rng = torch.zeros(2, 2, dtype=torch.int64)
    args = lambda **over: ops.StochasticArgs(**{**dict(rng=rng, sigma=0.7, eta=0.5, sqrt_1m_eta2=math.sqrt(0.75), step=3), **over})
    for bad in (args(rng=torch.zeros(1, 2, dtype=torch.int64)), args(rng=torch.zeros(2, 2, dtype=torch.int32)), args(rng=torch.zeros(2, 2)),
                args(rng=torch.zeros(2, 3, dtype=torch.int64)), args(rng=None), args(eta=0.0), args(eta=1.5), args(step=-1)):
        with pytest.raises(ValueError):
            ops.stochastic_step_f32_(x, v, bad, 0.5)
    with pytest.raises(ValueError, match="batch"):
        ops.stochastic_step_f32_(torch.zeros(8), torch.zeros(8, dtype=BF16), args(), 0.5)
    with pytest.raises(ValueError, match="history"):
        ops._master_step_f32("stochastic_step_f32_", x, v, None, 0.0, 0.0, None, 0.5, hist=x.clone(), stochastic=args())
    with pytest.raises(ValueError, match="history"):
        ops.projected_step_f32_(x, v, v, x.clone(), torch.zeros(ops.guidance_partials_shape(2, 8)), 2.0, 0.5, 0.0, 0.0, 0.0, hist32=x.clone(),
                                sigma_next=0.5, stochastic=args())
    with pytest.raises(ValueError):
        ops.normal_fill_f32(torch.zeros(2, 3, dtype=torch.int64), 8, 0)
    for good in (args(), args(eta=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.stochastic_step_f32_(x, v, good, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stochastic_step_f32_(x, v, args(rng=None), 0.0)                  # the last step needs no rng
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normal_fill_f32(rng, 8, 0)


def test_scheduler_refusals_need_no_device():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    sc = FlowMatchEulerDiscreteScheduler(stochastic_sampling=True)
    sc.set_timesteps(sigmas=[1.0, 0.5], mu=0.5)
    x, v = torch.zeros(1, 8), torch.zeros(1, 8, dtype=BF16)
    with pytest.raises(ValueError, match="stochastic="):
        sc.step_master_(v, x)
    assert sc.step_index is None                                             # refused before the index moved
    ms = FlowMatchMultistepScheduler()
    ms.set_timesteps(sigmas=[1.0, 0.5], mu=0.5)
    with pytest.raises(ValueError, match="exclude"):
        ms.step_master_(v, x, history=x.clone(), stochastic=sc.stochastic_step(torch.zeros(1, 2, dtype=torch.int64)))


# ------------------------------------------------------------------------------------------------------------------ 6. the call
def test_a_call_builds_the_noise_streams_only_under_the_switch():
    """The loop replaced by a recorder: without the switch the extras hold no ``step_noise`` and the default generator is where a call
    without the feature leaves it; with it, ``rng`` is ``stochastic_rng`` of the call's generator at the latents' batch and the key gets
    ("stochastic", eta) as its last entry."""
    from reptext_amd.pipeline import LoopExtras, StepNoise, stochastic_rng
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    import dataclasses
    assert LoopExtras().step_noise is None and "step_noise" in [f.name for f in dataclasses.fields(LoopExtras)]
    assert LoopExtras().signature(None, None, None) == () and list(StepNoise(torch.zeros(1, 2)).tensors()) == ["step_noise_rng"]
    pipe = make_pipe(union=None, controlnet=False)
    pipe.set_progress_bar_config(disable=True)
    seen = []

    def recorder(latents, *args, extras=None, **kwargs):
        seen.append(extras)
        pipe._master_latents = latents.float()
        return latents

    pipe._denoise_eager = recorder
    kw = call_kwargs(control_image_union=None)
    torch.manual_seed(5)
    pipe(**kw)
    plain_state = torch.get_rng_state().clone()
    assert seen[-1].step_noise is None
    pipe.scheduler = FlowMatchEulerDiscreteScheduler.from_config(dict(pipe.scheduler.config, stochastic_sampling=True, stochastic_eta=0.5))
    g = torch.Generator().manual_seed(77)
    pipe(**dict(kw, generator=g))
    noise = seen[-1].step_noise
    B = noise.rng.shape[0]
    assert isinstance(noise, StepNoise) and noise.rng.tolist() == stochastic_rng(g, B).tolist() == [[77, b] for b in range(B)]
    assert seen[-1].tensors()["step_noise_rng"] is noise.rng
    bound = seen[-1].rebound(dict(step_noise_rng=noise.rng.clone()))
    assert bound.step_noise.rng is not noise.rng and torch.equal(bound.step_noise.rng, noise.rng)
    # no generator: the seed is one draw from the default generator, taken after the start state's
    torch.manual_seed(5)
    pipe(**kw)
    assert not torch.equal(torch.get_rng_state(), plain_state) and seen[-1].step_noise.rng[:, 1].tolist() == list(range(B))
    assert_no_call_state(pipe)
    # the key: the Euler key plus one entry at its end
    base = dict(latents=torch.zeros(1, 4, 64), prompt_embeds=torch.zeros(1, 4, 8), pooled=torch.zeros(1, 8), text_ids=torch.zeros(4, 3),
                image_ids=torch.zeros(4, 3), hints=[], masks=[])
    pipe.scheduler.set_timesteps(sigmas=[1.0, 0.5], mu=0.5)
    stub = SimpleNamespace(reference_bf16_scalars=False, transformer=None, controlnet=None, scheduler=pipe.scheduler)      # no model to plan
    signature = lambda extras: type(pipe)._graph_signature(stub, base, extras, [1000.0, 500.0], 3.5, 1.0, 30, 2)
    (on, ins), (off, ins_off) = signature(LoopExtras(step_noise=noise)), signature(LoopExtras())
    assert on == off + (("stochastic", 0.5),) and ins["step_noise_rng"] is noise.rng and "step_noise_rng" not in ins_off


def test_the_inpaint_pipeline_refuses_the_switch_by_name():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    pipe = _pipe(inpaint=True)
    pipe.scheduler = FlowMatchEulerDiscreteScheduler.from_config(dict(pipe.scheduler.config, stochastic_sampling=True))
    with pytest.raises(ValueError, match="inpaint pipeline does not support stochastic sampling"):
        pipe(**_kw())
    assert_no_call_state(pipe)
