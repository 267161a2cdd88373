"""rt_normal_fill_f32, rt_stochastic_step_f32 and rt_projected_stochastic_step_f32 (csrc/norm_elem.hip, csrc/philox.h): the device
generator of the stochastic master step and the step itself.

The generator, against tests/philox_reference.py (Philox4x32-10 words, u in fp32 as the kernel rounds it, then fp64 normals). With
U = 2^-24 (one fp32 rounding, relative) and an error of k ulp read as 2·k·U relative:

    L = logf(u)          <= 1 ulp                     2U      (−2·L is exact)
    r = sqrtf(−2L)       halves what it inherits       U  +  <= 1 ulp of its own: 2U
    c, s = sincospif(2u) <= 2 ulp                     4U      (2·u is exact; the reduction of sincospi is exact, so the error is
                                                               relative to the result also next to its zeros)
    z = r·c              one rounding                  U

    |z − z64| <= 8·U·|z64| + 1e-15·r64

the last term for the fp64 reference's own θ = 2π·u, whose rounding moves cos and sin by 2π·2^-53 absolutely.

The step, against fp64 formed from the values the kernel reads and from the kernel's OWN z (bit for bit, from the fill entry):

    x0 = x − σ·v;   ê = x0 + v;   n = η < 1 ? c·ê + η·z : z;   r = (1 − σ')·x0 + σ'·n;   o = mask ? (1 − m)·keep + m·r : r

    |o − o64| <= R·U·M,    M = X0 + N [+ |src| + |noise|],  X0 = |x| + σ·V,  N = η < 1 ? c·(X0 + V) + η·|z| : |z|

V bounds every partial result of the velocity, as in tests/test_multistep_step_kernel_gpu.py. The rule is compiled without fused
multiply-adds, R counts its roundings: σ·v, x − ·, x0 + v, c·ê, η·z, their sum, 1 − σ', (1 − σ')·x0, σ'·n, the last sum: 10 (6 at
η = 1, the bound keeps 10). The mix adds 3 (t − u, s·(·), u + ·), whose error reaches o through factors below σ + 1, inside M. The blend
adds 8. The projected form is compared with the rule on the velocity that rt_projected_step_f32 itself forms for the same inputs (a
step from x = 0 with dσ = 1 returns it exactly: the sums, k and e are then the same bits); the two kernels may fuse the velocity's 5
operations differently, 5·U·V each: R = 10 + 10.

Shapes: B = 2 with n_s in {4, 7, 64·64, 1030} — one group, no 16-byte path (n_s % 4 != 0: a group would straddle the samples), more
than one block, a length with two elements past the last group — and every tensor at an element offset of 1, where no pointer is
aligned for the 16-byte path. The bitwise properties follow below."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_reference as ph  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
SIZES = [4, 7, 64 * 64, 1030]
FORMS = ["plain", "cfg", "repaint", "repaint_cfg_shared", "projected", "projected_repaint"]
SEEDS = [(42, 0), (-7046029254386353131, 3)]            # (seed, subsequence) of the two samples; the second seed has its high bits set
SIGMA, SIGMA_NEXT, S, STEP = 0.7321, 0.5543, 3.5, 5


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _place(t, gpu, off):
    """t on the device, contiguous, its first element ``off`` elements into a fresh allocation."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=gpu)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def _rng(gpu, rows=SEEDS):
    return torch.tensor(rows, dtype=torch.int64, device=gpu).reshape(len(rows), 2)


def _fill(ops, gpu, rows, n_s, step, off=0):
    out = _place(torch.full((len(rows), n_s), float("nan")), gpu, off)
    got = ops.normal_fill_f32(_rng(gpu, rows), n_s, step, out=out)
    assert got is out
    return out.cpu()


# ------------------------------------------------------------------------------------------------------------------ the fill entry
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n_s", SIZES)
def test_fill_against_the_restatement_per_element(gpu, n_s, off):
    from reptext_amd import ops

    got = _fill(ops, gpu, SEEDS, n_s, STEP, off).double().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b, (seed, sub) in enumerate(SEEDS):
        words = ph.group_words(seed, sub, STEP, (n_s + 3) // 4)
        ref = ph.normals(words).reshape(-1)[:n_s]
        u = ph.uniforms(words).astype(np.float64)
        r = np.repeat(np.sqrt(-2.0 * np.log(u[:, [0, 2]])), 2, axis=1).reshape(-1)[:n_s]
        bound = 8 * U * np.abs(ref) + 1e-15 * r
        err = np.abs(got[b] - ref)
        worst = max(worst, float((err / np.maximum(U * np.abs(ref), 1e-300)).max()))
        assert (err <= bound).all(), (b, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"[normal fill] n_s={n_s} off={off}: worst |z - z64| / (2^-24 |z64|) = {worst:.3f} (bound 8)")


@pytest.mark.parametrize("n_s", SIZES)
def test_group_path_and_tail_path_give_the_same_bits(gpu, n_s):
    """An aligned buffer with n_s % 4 == 0 takes 16-byte groups; the same at an element offset of 1 takes every element through the
    tail. For n_s % 4 != 0 both are the tail; the prefix property below ties them to the group path of a longer sample."""
    from reptext_amd import ops

    a, b = _fill(ops, gpu, SEEDS, n_s, STEP, 0), _fill(ops, gpu, SEEDS, n_s, STEP, 1)
    assert torch.equal(_bits(a), _bits(b))
    longer = _fill(ops, gpu, SEEDS, 4 * ((n_s + 3) // 4) + 4, STEP, 0)          # a multiple of 4: the group path
    assert torch.equal(_bits(a), _bits(longer[:, :n_s].contiguous()))             # an element's value does not depend on n_s


@pytest.mark.parametrize("n_s", SIZES)
def test_a_sample_of_a_batch_is_its_own_fill(gpu, n_s):
    from reptext_amd import ops

    both = _fill(ops, gpu, SEEDS, n_s, STEP)
    for b in range(2):
        assert torch.equal(_bits(both[b : b + 1].contiguous()), _bits(_fill(ops, gpu, SEEDS[b : b + 1], n_s, STEP)))
    assert torch.equal(_bits(_fill(ops, gpu, SEEDS[::-1], n_s, STEP)), _bits(both.flip(0).contiguous()))


def test_seed_subsequence_and_step_each_change_every_group(gpu):
    from reptext_amd import ops

    n_s = 64 * 64
    base = _fill(ops, gpu, [(42, 0)], n_s, 3)
    others = {"seed": _fill(ops, gpu, [(43, 0)], n_s, 3), "seed high": _fill(ops, gpu, [(42 + (1 << 32), 0)], n_s, 3),
              "subsequence": _fill(ops, gpu, [(42, 1)], n_s, 3), "step": _fill(ops, gpu, [(42, 0)], n_s, 4)}
    for name, other in others.items():
        differs = (_bits(base) != _bits(other)).view(-1, 4)
        assert bool(differs.any(dim=1).all()), name


def test_moments_of_one_large_fill(gpu):
    """n = 4096·64 draws of seed 42, subsequence 0, step 3: mean, variance, fourth moment, lag-1 product and the product with step 4,
    each standardised by its standard deviation under the normal law, below 4 (the restatement gives at most 1.5 for these)."""
    from reptext_amd import ops

    n = 4096 * 64
    z = _fill(ops, gpu, [(42, 0)], n, 3).double().reshape(-1)
    z4 = _fill(ops, gpu, [(42, 0)], n, 4).double().reshape(-1)
    stats = {"mean": abs(float(z.mean())) * math.sqrt(n), "var": abs(float(z.var(unbiased=False)) - 1.0) * math.sqrt(n / 2),
             "m4": abs(float((z ** 4).mean()) - 3.0) * math.sqrt(n / 96), "lag1": abs(float((z[1:] * z[:-1]).sum())) / math.sqrt(n - 1),
             "step3 x step4": abs(float((z * z4).sum())) / math.sqrt(n)}
    print("[normal fill] standardised moments:", {k: round(v, 3) for k, v in stats.items()}, "max |z|", float(z.abs().max()))
    assert all(v < 4.0 for v in stats.values()), stats
    assert float(z.abs().max()) <= math.sqrt(2.0 * math.log(2.0 ** 25))


# ------------------------------------------------------------------------------------------------------------------ the step
def _inputs(B, n, seed, form):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, u, t, src, noise = rn(B, n), rn(B, n).to(BF16), rn(B, n).to(BF16), rn(B, n), rn(B, n)
    mask = torch.rand(1 if "shared" in form else B, n, generator=g) if "repaint" in form else None
    return x, u, t, src, noise, mask


def _step(ops, gpu, form, x, u, t, src, noise, mask, rng, eta, sigma_next, off=0, with_bf16=True, step=STEP):
    """One stochastic step of ``form`` on device copies -> (state, bf16 copy) on the CPU."""
    x32 = _place(x, gpu, off)
    xb = _place(torch.full(x.shape, 12345.0, dtype=BF16), gpu, off) if with_bf16 else None
    st = ops.StochasticArgs(rng, _f32(SIGMA), eta, math.sqrt(max(0.0, 1.0 - eta * eta)), step)
    rp = {} if mask is None else dict(src32=_place(src, gpu, off), noise32=_place(noise, gpu, off), mask=_place(mask, gpu, off))
    if form.startswith("projected"):
        B, n = x.shape
        diff = _place(torch.full(x.shape, float("nan")), gpu, off)
        part = torch.full(ops.guidance_partials_shape(B, n), float("nan"), device=gpu, dtype=F32)
        out = ops.projected_step_f32_(x32, _place(u, gpu, off), _place(t, gpu, off), diff, part, S, 0.25, 0.0, 0.0, 0.0, xb,
                                      sigma_next=sigma_next, stochastic=st, **rp)
    else:
        out = ops.stochastic_step_f32_(x32, _place(u, gpu, off), st, sigma_next, xb, v_text=_place(t, gpu, off) if "cfg" in form else None,
                                       s=S, **rp)
    assert out is x32
    return x32.cpu(), None if xb is None else xb.cpu()


def _velocity(ops, gpu, form, u, t, off):
    """(v64, V, R_v): the velocity in fp64, the bound of its partial results, the roundings it adds to the rule's 10."""
    d = lambda a: a.double()
    if form.startswith("projected"):
        B, n = u.shape
        x0 = _place(torch.zeros(B, n), gpu, off)
        diff = _place(torch.full((B, n), float("nan")), gpu, off)
        part = torch.full(ops.guidance_partials_shape(B, n), float("nan"), device=gpu, dtype=F32)
        ops.projected_step_f32_(x0, _place(u, gpu, off), _place(t, gpu, off), diff, part, S, 0.25, 0.0, 0.0, 1.0)       # 0 + 1·v
        v = x0.cpu().double()
        # every partial result of p + (s − 1)·(k·d + e·p) with k = 1 (no clamp) lies below |p| + |s − 1|·(|d| + |e p|) <= this
        return v, d(t).abs() + abs(S - 1.0) * (d(t).abs() * 2 + d(u).abs()) + v.abs(), 10
    if "cfg" in form:
        return d(u) + S * (d(t) - d(u)), d(u).abs() + abs(S) * (d(t).abs() + d(u).abs()), 3
    return d(u), d(u).abs(), 0


def _fp64(x, v, V, z, src, noise, mask, sigma, sigma_next, eta):
    d = lambda a: a.double()
    c = math.sqrt(max(0.0, 1.0 - eta * eta))
    r = ph.stochastic_rule(d(x), v, d(z), sigma, sigma_next, eta)
    X0 = d(x).abs() + sigma * V
    M = X0 + (c * (X0 + V) + eta * d(z).abs() if eta < 1.0 else d(z).abs())
    if mask is None:
        return r, M
    keep = (1.0 - sigma_next) * d(src) + sigma_next * d(noise)
    m = d(mask).expand_as(x)
    return (1.0 - m) * keep + m * r, M + d(src).abs() + d(noise).abs()


@pytest.mark.parametrize("eta", [1.0, 0.5])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_s", SIZES)
def test_step_against_fp64_from_the_kernels_own_noise(gpu, n_s, form, off, eta):
    from reptext_amd import ops

    x, u, t, src, noise, mask = _inputs(2, n_s, n_s + 7 * FORMS.index(form) + off, form)
    rng = _rng(gpu)
    z = _fill(ops, gpu, SEEDS, n_s, STEP)
    sigma, sn = _f32(SIGMA), _f32(SIGMA_NEXT)
    v, V, Rv = _velocity(ops, gpu, form, u, t, off)
    ref, M = _fp64(x, v, V, z, src, noise, mask, sigma, sn, _f32(eta))
    R = 10 + Rv + (8 if mask is not None else 0)
    got, gb = _step(ops, gpu, form, x, u, t, src, noise, mask, rng, _f32(eta), sn, off)
    again, ab = _step(ops, gpu, form, x, u, t, src, noise, mask, rng, _f32(eta), sn, off)
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(gb), _bits(ab))
    err = (got.double() - ref).abs()
    ratio = float((err / (U * M).clamp_min(1e-300)).max())
    print(f"[stochastic step] n_s={n_s} {form} off={off} eta={eta}: worst |o - o64| / (2^-24 M) = {ratio:.3f} (bound {R})")
    assert bool(torch.isfinite(got).all()) and bool((err <= R * U * M).all()), ratio
    assert torch.equal(_bits(gb), _bits(got.to(BF16)))                       # the bf16 copy of the kernel's own fp32 result
    # the noise is felt: the same rule with other noise (the next step's) lies outside the bound somewhere, and so does the Euler step
    other, _ = _fp64(x, v, V, _fill(ops, gpu, SEEDS, n_s, STEP + 1), src, noise, mask, sigma, sn, _f32(eta))
    assert bool(((other - ref).abs() > R * U * M).any())
    # the 16-byte path and the tail: the aligned launch and the one at an element offset agree bit for bit
    if off == 1:
        aligned, _ = _step(ops, gpu, form, x, u, t, src, noise, mask, rng, _f32(eta), sn, 0)
        assert torch.equal(_bits(got), _bits(aligned))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_s", [7, 64 * 64])
def test_the_last_step_is_the_clean_image_and_reads_no_noise(gpu, n_s, form):
    """sigma_next = 0: r = x0 = x − σ·v (2 roundings, plus the velocity's), whatever rng holds — two tables with nothing in common
    give the same bits — and at any eta; under a mask the kept region is the source."""
    from reptext_amd import ops

    x, u, t, src, noise, mask = _inputs(2, n_s, 50 + n_s + FORMS.index(form), form)
    sigma = _f32(SIGMA)
    v, V, Rv = _velocity(ops, gpu, form, u, t, 0)
    ref, M = _fp64(x, v, V, torch.zeros_like(x), src, noise, mask, sigma, 0.0, 1.0)
    a, ab = _step(ops, gpu, form, x, u, t, src, noise, mask, _rng(gpu), 1.0, 0.0)
    poisoned = _rng(gpu, [(-1, -1), (0x7FFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF)])
    b, bb = _step(ops, gpu, form, x, u, t, src, noise, mask, poisoned, _f32(0.5), 0.0, step=9)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ab), _bits(bb)) and bool(torch.isfinite(a).all())
    R = 2 + Rv + (8 if mask is not None else 0)
    assert bool(((a.double() - ref).abs() <= R * U * M).all())
    assert torch.equal(_bits(ab), _bits(a.to(BF16)))


def test_existing_entries_return_their_bits_before_and_after(gpu):
    """The Euler, CFG, repaint and multistep entries around stochastic launches: the same bits as before them."""
    from reptext_amd import ops

    x, u, t, src, noise, mask = _inputs(2, 1030, 99, "repaint")
    dev = lambda a: a.to(gpu)

    def old_entries():
        outs = []
        for run in (lambda a, b: ops.euler_step_f32_(a, dev(u), -0.0116, b), lambda a, b: ops.cfg_euler_step_f32_(a, dev(u), dev(t), S, -0.0116, b),
                    lambda a, b: ops.repaint_euler_step_f32_(a, dev(u), dev(t), S, -0.0116, 0.6543, dev(src), dev(noise), dev(mask), b),
                    lambda a, b: ops.multistep_step_f32_(a, dev(u), dev(noise), 0.4321, -0.0116, b)):
            a, b = dev(x), torch.zeros(x.shape, dtype=BF16, device=gpu)
            run(a, b)
            outs += [a.cpu(), b.cpu()]
        return outs

    before = old_entries()
    for form in FORMS:
        _step(ops, gpu, form, x, u, t, src, noise, mask, _rng(gpu), _f32(0.5), _f32(SIGMA_NEXT))
    after = old_entries()
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(before, after))


def test_scheduler_step_master_and_step_go_through_the_op(gpu):
    """``step_master_(stochastic=)`` is the op with the scheduler's sigmas, eta and ABSOLUTE step index, from a begin index too;
    ``step`` (the diffusers contract) is the same op on an fp32 temporary, rounded to the model dtype."""
    from reptext_amd import ops
    from reptext_amd.pipeline import stochastic_rng
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 1030, generator=g)
    vs = [torch.randn(2, 1030, generator=g).to(gpu, BF16) for _ in range(4)]
    gens = [torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)]
    rng = stochastic_rng(gens, 2).to(gpu)
    for begin in (None, 1):
        sc = FlowMatchEulerDiscreteScheduler(stochastic_sampling=True, stochastic_eta=0.5)
        sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=0.5)
        first = 0
        if begin is not None:
            sc.set_begin_index(begin)
            first = begin
        a32, ab = x.to(gpu), torch.zeros(2, 1030, dtype=BF16, device=gpu)
        b32, bb = x.to(gpu), torch.zeros(2, 1030, dtype=BF16, device=gpu)
        with pytest.raises(ValueError, match="stochastic="):
            sc.step_master_(vs[0], a32, ab)
        sc._step_index = None
        for i in range(first, 4):
            sc.step_master_(vs[i], a32, ab, stochastic=sc.stochastic_step(rng))
            ops.stochastic_step_f32_(b32, vs[i], ops.StochasticArgs(rng, float(sc.sigmas[i]), 0.5, math.sqrt(0.75), i), float(sc.sigmas[i + 1]), bb)
            assert sc.step_index == i + 1 and torch.equal(a32, b32) and torch.equal(ab, bb) and bool(torch.isfinite(a32).all())
    sc = FlowMatchEulerDiscreteScheduler(stochastic_sampling=True)
    sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=0.5)
    got = want = x.to(gpu, BF16)
    for i in range(4):
        got = sc.step(vs[i], sc.timesteps[i], got, generator=gens).prev_sample
        tmp = want.float()
        ops.stochastic_step_f32_(tmp, vs[i], ops.StochasticArgs(rng, float(sc.sigmas[i]), 1.0, 0.0, i), float(sc.sigmas[i + 1]))
        want = tmp.to(BF16)
        assert got.dtype == BF16 and torch.equal(got, want)
    assert gens[0].initial_seed() == 5 and torch.equal(gens[0].get_state(), torch.Generator().manual_seed(5).get_state())
