"""rt_multistep_step_f32 (csrc/norm_elem.hip): the second-order multistep form of the fp32 master step. Per element

    vel  = v_text ? u + s·(t − u) : v            u = v, t = v_text, bf16 widened
    vel2 = w != 0 ? vel + w·(vel − h) : vel      h: the velocity of the step before, fp32
    r    = x + dσ·vel2
    keep = (1 − σn)·src + σn·noise
    o    = mask ? (1 − m)·keep + m·r : r,   m = mask[i % n_mask]
    h'   = vel

against fp64 on the values the kernel reads (inputs rounded on the CPU to bf16 / fp32, the scalars to C floats):

    |o − o64| <= R · 2^-24 · M,      M = |x| + |dσ|·(V + |w|·(V + |h|)) [+ |src| + |noise| with a mask]

V bounds every partial result of the velocity: V = |u| without the mix (the widening is exact), V = |u| + |s|·(|t| + |u|) with it
(|t − u|, |s·(t − u)| and |vel| all lie below it). Then |vel − h| <= V + |h|, |w·(vel − h)| and |vel2| <= V + |w|·(V + |h|), and every
partial result of r, carried through the factors that follow it, lies below |x| + |dσ|·(V + |w|·(V + |h|)); with m and σn in [0, 1] the
partial results of the blend lie below |r| + |src| + |noise|. R counts the fp32 roundings, each relative 2^-24 of its partial result:
vel − h, w·(·), vel + ·, dσ·vel2, x + · — R = 5; the mix adds t − u, s·(·), u + · — R = 8; the blend adds 1 − σn, (1 − σn)·src,
σn·noise, their sum, 1 − m, (1 − m)·keep, m·r and the last sum — R = 13, and 16 with the mix. Where the compiler fuses a multiply-add a
rounding disappears, none is added. The written history: without the mix it is the widened bf16 velocity bit for bit, with it
|h' − vel64| <= 3 · 2^-24 · V.

The sizes: a per-sample length of 64, 67 and 16384·3 + 64 at batch 1 and 3 — 67 is no multiple of 4: the vector path leaves a tail of
3 (batch 1) or 1 (batch 3) elements, and one mask of period 67 for a batch of 3 sends every element down the one-element path — with
and without the mix, without a mask, with one mask for the batch and with one per sample, with and without the bf16 copy; and one
size past 4 · 4096 · 256 elements with three left over, where the 16-byte loop's grid stride wraps and the tail runs after it.

The bitwise edges: w = 0 with a NaN-filled history is rt_euler_step_f32 / rt_cfg_euler_step_f32 / rt_repaint_euler_step_f32 and
leaves the velocity in the history; the scheduler's chained steps are the op with ``multistep_weights``' values, from a begin index
too; ``reset_history`` makes the next step first order; ``solver_order=1`` is the Euler scheduler. The entry's refusals on null
pointers and the derived binding need no device: tests/test_multistep_host.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SIZES = [64, 67, 16384 * 3 + 64]
MASKS = [None, "shared", "per_sample"]
DS, SN, S, W = -0.0116, 0.6543, 3.5, 0.4321
WRAP = 4 * (4096 * 256 + 1000)                          # 1000 groups of four more than one pass of the largest grid takes


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _inputs(B, n, seed, mask):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, u, t, h, src, noise = rn(B, n), rn(B, n).to(BF16), rn(B, n).to(BF16), rn(B, n), rn(B, n), rn(B, n)
    m = None if mask is None else torch.rand(1 if mask == "shared" else B, n, generator=g)
    return x, u, t, h, src, noise, m


def _fp64(x, u, t, h, src, noise, mask, s, ds, sn, w):
    """(o64, M, vel64, V) of the expression; ``t`` None: no CFG mix, ``mask`` None: no blend."""
    d = lambda a: a.double()
    vel = d(u) if t is None else d(u) + s * (d(t) - d(u))
    V = d(u).abs() if t is None else d(u).abs() + abs(s) * (d(t).abs() + d(u).abs())
    vel2 = vel + w * (vel - d(h)) if w != 0.0 else vel
    r = d(x) + ds * vel2
    M = d(x).abs() + abs(ds) * (V + abs(w) * (V + d(h).abs()))
    if mask is None:
        return r, M, vel, V
    keep = (1.0 - sn) * d(src) + sn * d(noise)
    m = d(mask).expand_as(x)
    return (1.0 - m) * keep + m * r, M + d(src).abs() + d(noise).abs(), vel, V


def _run(ops, gpu, x, u, t, h, src, noise, mask, with_bf16, s=S, ds=DS, sn=SN, w=W):
    x32, h32 = x.to(gpu), h.to(gpu)
    xb = torch.full(x.shape, 12345.0, dtype=BF16, device=gpu) if with_bf16 else None
    rp = {} if mask is None else dict(sigma_next=sn, src32=src.to(gpu), noise32=noise.to(gpu), mask=mask.to(gpu))
    out = ops.multistep_step_f32_(x32, u.to(gpu), h32, w, ds, xb, v_text=None if t is None else t.to(gpu), s=s, **rp)
    assert out is x32
    return x32.cpu(), h32.cpu(), None if xb is None else xb.cpu()


def _check_against_fp64(ops, gpu, B, n, mask, cfg, with_bf16, seed):
    x, u, t, h, src, noise, m = _inputs(B, n, seed, mask)
    t = t if cfg else None
    ds, sn, s, w = _f32(DS), _f32(SN), _f32(S), _f32(W)
    ref, M, vel, V = _fp64(x, u, t, h, src, noise, m, s, ds, sn, w)
    R = (5 if m is None else 13) + (3 if cfg else 0)
    got, gh, gb = _run(ops, gpu, x, u, t, h, src, noise, m, with_bf16)
    again, ah, ab = _run(ops, gpu, x, u, t, h, src, noise, m, with_bf16)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(gh.view(torch.int32), ah.view(torch.int32))
    ratio = float(((got.double() - ref).abs() / (2.0 ** -24 * M).clamp_min(1e-300)).max())
    print(f"[multistep step] B={B} n={n} mask={mask} cfg={cfg} bf16={with_bf16}: worst |o - o64| / (2^-24 M) = {ratio:.3f} (bound {R})")
    assert bool(((got.double() - ref).abs() <= R * 2.0 ** -24 * M).all()), ratio
    assert not torch.equal(got, x)
    # the history is this step's velocity
    if cfg:
        assert bool(((gh.double() - vel).abs() <= 3 * 2.0 ** -24 * V).all())
    else:
        assert torch.equal(gh.view(torch.int32), u.float().view(torch.int32))
    assert not torch.equal(gh, h)
    if with_bf16:
        assert torch.equal(gb.view(torch.int16), got.to(BF16).view(torch.int16))  # bf16 of the kernel's own fp32 result
        assert torch.equal(gb.view(torch.int16), ab.view(torch.int16))
    # the second-order term is felt: the first-order step lies outside the bound (almost everywhere; somewhere is asserted)
    first, _, _, _ = _fp64(x, u, t, h, src, noise, m, s, ds, sn, 0.0)
    assert bool(((first - ref).abs() > R * 2.0 ** -24 * M).any())


@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_multistep_step_against_fp64_per_element(gpu, n, B, cfg, mask, with_bf16):
    from reptext_amd import ops

    seed = n % 1000 + 10 * B + 4 * MASKS.index(mask) + 2 * cfg + with_bf16
    _check_against_fp64(ops, gpu, B, n, mask, cfg, with_bf16, seed)


def test_multistep_step_where_the_grid_stride_loop_wraps(gpu):
    """4096 blocks of 256 threads are the launch's cap: with more than 4096 · 256 groups of four a thread of the 16-byte loop takes a
    second group, of the history as of the state; the three elements after the last group take the one-element tail of the same launch."""
    from reptext_amd import ops

    assert (WRAP + 3) // 4 > 4096 * 256 and (WRAP + 3) % 4 == 3
    _check_against_fp64(ops, gpu, 1, WRAP + 3, "per_sample", True, True, seed=6)


# ------------------------------------------------------------------------------------------------------------------ bitwise edges
@pytest.mark.parametrize("form", ["plain", "cfg", "repaint", "repaint_cfg", "repaint_shared"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_weight_never_reads_the_history_and_is_the_euler_step_bit_for_bit(gpu, n, form):
    """w = 0 with a history full of NaN: the state and its bf16 copy get the bits of the entry without a history that the other
    arguments select, no NaN reaches them, and the history holds the velocity afterwards — the one a step with w != 0 writes."""
    from reptext_amd import ops

    cfg, mask = form.endswith("cfg"), {"repaint": "per_sample", "repaint_cfg": "per_sample", "repaint_shared": "shared"}.get(form)
    x, u, t, h, src, noise, m = _inputs(3, n, 100 + n % 1000 + len(form), mask)
    t = t if cfg else None
    nan = torch.full_like(h, float("nan"))
    got, gh, gb = _run(ops, gpu, x, u, t, nan, src, noise, m, True, w=0.0)
    a32, ab = x.to(gpu), torch.zeros(3, n, dtype=BF16, device=gpu)
    dev = lambda v: None if v is None else v.to(gpu)
    if m is not None:
        ops.repaint_euler_step_f32_(a32, dev(u), dev(t), S, DS, SN, dev(src), dev(noise), dev(m), ab)
    elif cfg:
        ops.cfg_euler_step_f32_(a32, dev(u), dev(t), S, DS, ab)
    else:
        ops.euler_step_f32_(a32, dev(u), DS, ab)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gh).all())
    assert torch.equal(got.view(torch.int32), a32.cpu().view(torch.int32))
    assert torch.equal(gb.view(torch.int16), ab.cpu().view(torch.int16))
    _, second_order_hist, _ = _run(ops, gpu, x, u, t, h, src, noise, m, False)
    assert torch.equal(gh.view(torch.int32), second_order_hist.view(torch.int32))
    if not cfg:
        assert torch.equal(gh.view(torch.int32), u.float().view(torch.int32))


SIGMAS = [1.0, 0.75, 0.5, 0.25]


def _scheduler(cls, **config):
    sc = cls(**config)
    sc.set_timesteps(sigmas=SIGMAS, mu=0.5)
    return sc


@pytest.mark.parametrize("begin", [None, 1])
@pytest.mark.parametrize("form", ["plain", "cfg", "repaint_cfg"])
def test_chained_scheduler_steps_are_the_op_with_the_weights(gpu, form, begin):
    from reptext_amd import ops
    from reptext_amd.pipeline import Repaint
    from reptext_amd.scheduler import FlowMatchMultistepScheduler, multistep_weights

    cfg, rep = form.endswith("cfg"), form.startswith("repaint")
    x, _, _, _, src, noise, mask = _inputs(2, 1000, 7, "shared")
    g = torch.Generator().manual_seed(8)
    vs = [(torch.randn(2, 1000, generator=g).to(gpu, BF16), torch.randn(2, 1000, generator=g).to(gpu, BF16)) for _ in range(4)]
    dev = lambda a: a.to(gpu)
    sc = _scheduler(FlowMatchMultistepScheduler)
    first = 0
    if begin is not None:
        sc.set_begin_index(begin)
        first = begin
    w = multistep_weights(sc.sigmas, begin=first)
    assert w[first] == 0.0 and all(v != 0.0 for v in w[first + 1:])
    a32, ab, ah = dev(x), torch.zeros(2, 1000, dtype=BF16, device=gpu), torch.full((2, 1000), float("nan"), device=gpu)
    b32, bb, bh = dev(x), torch.zeros(2, 1000, dtype=BF16, device=gpu), torch.full((2, 1000), float("nan"), device=gpu)
    rp = dict(src32=dev(src), noise32=dev(noise), mask=dev(mask)) if rep else {}
    for i in range(first, 4):
        u, t = vs[i]
        sc.step_master_(u, a32, ab, v_text=t if cfg else None, s=2.0 if cfg else None, repaint=Repaint(**rp) if rep else None, history=ah)
        ops.multistep_step_f32_(b32, u, bh, w[i], float(sc.sigmas[i + 1] - sc.sigmas[i]), bb, v_text=t if cfg else None, s=2.0 if cfg else 0.0,
                                sigma_next=float(sc.sigmas[i + 1]) if rep else 0.0, **rp)
        assert sc.step_index == i + 1
        assert torch.equal(a32, b32) and torch.equal(ab, bb) and torch.equal(ah, bh) and torch.equal(ab, a32.to(BF16))
        assert bool(torch.isfinite(a32).all())
    # and it is not the Euler walk
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    eu = _scheduler(FlowMatchEulerDiscreteScheduler)
    if begin is not None:
        eu.set_begin_index(begin)
    e32 = dev(x)
    for i in range(first, 4):
        eu.step_master_(vs[i][0], e32, v_text=vs[i][1] if cfg else None, s=2.0 if cfg else None, repaint=Repaint(**rp) if rep else None)
    assert not torch.equal(e32, a32)


def test_reset_history_makes_the_next_step_first_order(gpu):
    from reptext_amd import ops
    from reptext_amd.scheduler import FlowMatchMultistepScheduler, multistep_weights

    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 67, generator=g).to(gpu)
    vs = [torch.randn(3, 67, generator=g).to(gpu, BF16) for _ in range(4)]
    sc = _scheduler(FlowMatchMultistepScheduler)
    w = multistep_weights(sc.sigmas)
    a32, ah = x.clone(), torch.empty_like(x)
    b32, bh = x.clone(), torch.empty_like(x)
    for i in range(4):
        if i == 2:
            sc.reset_history()
            ah.fill_(float("nan"))                       # and what the history held is not read
        sc.step_master_(vs[i], a32, history=ah)
        ops.multistep_step_f32_(b32, vs[i], bh, 0.0 if i == 2 else w[i], float(sc.sigmas[i + 1] - sc.sigmas[i]))
        assert torch.equal(a32, b32), i
    assert sc.step_index == 4 and bool(torch.isfinite(a32).all())


def test_solver_order_one_is_the_euler_scheduler_bit_for_bit(gpu):
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler

    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 1000, generator=g)
    vs = [torch.randn(2, 1000, generator=g).to(gpu, BF16) for _ in range(4)]
    one, eu = _scheduler(FlowMatchMultistepScheduler, solver_order=1), _scheduler(FlowMatchEulerDiscreteScheduler)
    a32, e32 = x.to(gpu), x.to(gpu)
    ab, eb = torch.zeros(2, 1000, dtype=BF16, device=gpu), torch.zeros(2, 1000, dtype=BF16, device=gpu)
    nan = torch.full((2, 1000), float("nan"), device=gpu)
    for i in range(4):
        one.step_master_(vs[i], a32, ab, history=nan)          # a history may be passed: order 1 neither reads nor writes it
        eu.step_master_(vs[i], e32, eb)
        assert torch.equal(a32, e32) and torch.equal(ab, eb) and one.step_index == eu.step_index == i + 1
    assert bool(torch.isnan(nan).all())
    # step(), the diffusers contract: bf16 in, bf16 out, at order 1 the Euler scheduler's result
    one, eu = _scheduler(FlowMatchMultistepScheduler, solver_order=1), _scheduler(FlowMatchEulerDiscreteScheduler)
    xa = xe = x.to(gpu, BF16)
    for i in range(4):
        xa = one.step(vs[i], one.timesteps[i], xa).prev_sample
        xe = eu.step(vs[i], eu.timesteps[i], xe, return_dict=False)[0]
        assert xa.dtype == BF16 and torch.equal(xa, xe)


def test_step_keeps_a_history_of_its_own_and_goes_through_the_op(gpu):
    """``step`` (the diffusers contract): the sample comes and goes in the model dtype, the step itself is the op on an fp32 temporary
    with an fp32 history that the scheduler keeps; ``reset_history`` and ``set_timesteps`` drop it."""
    from reptext_amd import ops
    from reptext_amd.scheduler import FlowMatchMultistepScheduler, multistep_weights

    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 67, generator=g).to(gpu, BF16)
    vs = [torch.randn(2, 67, generator=g).to(gpu, BF16) for _ in range(4)]
    sc = _scheduler(FlowMatchMultistepScheduler)
    w = multistep_weights(sc.sigmas)
    got, want, hist = x, x, torch.empty(2, 67, device=gpu)
    for i in range(4):
        before = got.clone()
        got = sc.step(vs[i], sc.timesteps[i], got).prev_sample
        tmp = want.float()
        ops.multistep_step_f32_(tmp, vs[i], hist, w[i], float(sc.sigmas[i + 1] - sc.sigmas[i]))
        want = tmp.to(BF16)
        assert got.dtype == BF16 and torch.equal(got, want) and torch.equal(sc._step_history, hist) and sc.step_index == i + 1
        assert got.data_ptr() != before.data_ptr()
    sc.reset_history()
    assert sc._step_history is None
    sc.set_timesteps(sigmas=SIGMAS, mu=0.5)
    first = sc.step(vs[0], sc.timesteps[0], x, return_dict=False)[0]
    tmp = x.float()
    ops.euler_step_f32_(tmp, vs[0], float(sc.sigmas[1] - sc.sigmas[0]))
    assert torch.equal(first, tmp.to(BF16))
