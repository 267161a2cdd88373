"""rt_guidance_reduce_f32 + rt_projected_step_f32 (csrc/norm_elem.hip): projected guidance in the fp32 master step. Per sample of
n_s elements, p = v_text and u = v_uncond (bf16, widened), r the guidance difference of the step before (fp32):

    d = (p − u) + β·r;   a = Σ d², b = Σ d·p, c = Σ p²;   k = τ > 0 and a > τ² ? τ/√a : 1;   e = (η − 1)·(c > 0 ? k·b/c : 0)
    v = p + (s − 1)·(k·d + e·p);   vel2 = w != 0 ? v + w·(v − h) : v;   r' = x + dσ·vel2;   o = mask ? (1 − m)·keep + m·r' : r'

against fp64 (tests/loop_reference.py: ``projected_velocity``) on the values the kernels read. With U = 2^-24 and γ(R) = R·U/(1 − R·U):

The sums. d takes R_d roundings, 1 without momentum and 3 with it (p − u, β·r, their sum), each relative to a partial result below
D = |p − u| + |β·r|. A term d², d·p, p² takes one more for the product, after the 2·R_d, R_d, 0 it inherits from d. A term then goes
through at most 15 additions in its thread (16 terms per thread: 4 groups of 4), 6 in the wave's xor butterfly and 3 across the four
waves: 24. So

    |a − a64| <= γ(2·R_d + 25)·Σ D²,   |b − b64| <= γ(R_d + 25)·Σ D·|p|,   |c − c64| <= γ(25)·Σ p²

relative to Σ |term|, not to the sum (b may cancel to nothing). The launch-boundary sum of at most 144 partials and k, e are formed
in double, 2^-53 per operation: 150·2^-53·Σ |term| is added to each bound for them.

k and e. With ε = (bound of a)/a64: |k − k64| <= δk = k64·(ε/(2·(1 − ε)) + U) where the clamp is active (τ stays well away from ‖d‖ in
every case here), 0 where it is not (k = 1 exactly). |e − e64| <= δe = |η − 1|·(δk·(|b| + Δb)/(c − Δc) + k·Δb/(c − Δc) + k·|b|·Δc/(c·(c − Δc))) + U·|e|.

v and the state. v takes 5 roundings (k·d, e·p, their sum, the product with s − 1, p + ·) of partial results below
V = |p| + |s − 1|·(k·D + |e|·|p|), and inherits d's R_d·U·D·|s − 1|·k <= R_d·U·V:

    |v − v64| <= γ(5 + R_d)·V + |s − 1|·(D·δk + |p|·δe)  =: Ev

and then, exactly as in tests/test_multistep_step_kernel_gpu.py, with M = |x| + |dσ|·(V + |w|·(V + |h|)) [+ |src| + |noise|]:

    |o − o64| <= γ(10 + R_d [+ 8])·M + |dσ|·(1 + |w|)·|s − 1|·(D·δk + |p|·δe)

The cases: generic; d ⟂ p by disjoint supports (b is exactly 0); u = p/2 with η = 0 (every element cancels: v = p up to the bound, which
is absolute in k·|d| + |e|·|p|); the clamp active and inactive; a second step with β = −0.5 on the difference the first one wrote.
The shapes (B, n_s): (1, 64) less than a chunk; (2, 4032) and (2, 4096) just below and at one chunk; (3, 4160) a second chunk of 64;
(1, 16384) four full chunks; (2, 12289) an odd length: no 16-byte path, a last chunk of one element; (2, 4096) with every tensor taken at
an element offset of 1, so that no pointer is aligned for the 16-byte path. The bitwise properties follow below."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from loop_reference import projected_velocity  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
SHAPES = [(1, 64, 0), (2, 4032, 0), (2, 4096, 0), (3, 4160, 0), (1, 16384, 0), (2, 12289, 0), (2, 4096, 1)]
IDS = [f"{b}x{n}" + ("+1" if off else "") for b, n, off in SHAPES]
CASES = ["generic", "orthogonal", "cancel", "clamp_on", "clamp_off", "momentum"]
FORMS = ["plain", "multi", "repaint", "repaint_shared_multi"]
DS, SN, S1, W = -0.0116, 0.6543, 2.5, 0.4321            # S1 = s − 1, a C float exactly


def gamma(R):
    return R * U / (1.0 - R * U)


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _place(t, gpu, off):
    """t on the device, contiguous, its first element ``off`` elements into a fresh allocation."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=gpu)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def _inputs(B, n, seed, case, form):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, p, u, h, src, noise = rn(B, n), rn(B, n).to(BF16), rn(B, n).to(BF16), rn(B, n), rn(B, n), rn(B, n)
    if case == "orthogonal":                                  # p lives on even elements, d = p − u on odd ones
        even = (torch.arange(n) % 2 == 0)
        d = torch.where(even, torch.zeros(()), u.float())
        p = torch.where(even, p.float(), torch.zeros(())).to(BF16)
        u = (p.float() - d).to(BF16)                           # exact: one of the two is zero
    elif case == "cancel":
        u = (p.float() / 2).to(BF16)                           # exact
    mask = None
    if form.startswith("repaint"):
        mask = torch.rand(1 if "shared" in form else B, n, generator=g)
    return x, p, u, h, src, noise, mask


def _launch(ops, gpu, x, p, u, diff_dev, s, eta, tau, beta, h=None, w=0.0, mask=None, src=None, noise=None, sn=SN, off=0, with_bf16=True):
    """One projected step on device copies; (state, bf16 copy, diff, partials, hist) on the CPU, and the device diff for a next step."""
    B, n = x.shape
    x32 = _place(x, gpu, off)
    xb = _place(torch.full(x.shape, 12345.0, dtype=BF16), gpu, off) if with_bf16 else None
    if diff_dev is None:
        diff_dev = _place(torch.full(x.shape, float("nan")), gpu, off)
    part = torch.full(ops.guidance_partials_shape(B, n), float("nan"), device=gpu, dtype=F32)
    kw = {}
    if h is not None:
        kw.update(hist32=_place(h, gpu, off), w=w)
    if mask is not None:
        kw.update(sigma_next=sn, src32=_place(src, gpu, off), noise32=_place(noise, gpu, off), mask=_place(mask, gpu, off))
    out = ops.projected_step_f32_(x32, _place(u, gpu, off), _place(p, gpu, off), diff_dev, part, s, eta, tau, beta, DS, xb, **kw)
    assert out is x32
    return x32.cpu(), None if xb is None else xb.cpu(), diff_dev.cpu(), part.cpu(), kw["hist32"].cpu() if h is not None else None, diff_dev


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _check(ops, gpu, B, n, off, case, form, seed):
    x, p, u, h, src, noise, mask = _inputs(B, n, seed, case, form)
    multi = "multi" in form
    ds, sn, w = _f32(DS), _f32(SN), _f32(W) if multi else 0.0
    s = 1.0 + S1
    eta = {"generic": 0.25, "orthogonal": 0.0, "cancel": 0.0, "clamp_on": 0.5, "clamp_off": 0.5, "momentum": 0.25}[case]
    norm = (p.double() - u.double()).flatten(1).norm(dim=1)
    tau = {"clamp_on": _f32(0.5 * float(norm.min())), "clamp_off": _f32(2.0 * float(norm.max())), "momentum": _f32(0.5 * float(norm.min()))}.get(case, 0.0)
    beta, r_prev = 0.0, None
    if case == "momentum":                                    # a first step with other halves leaves its difference in the buffer
        g = torch.Generator().manual_seed(seed + 1)
        p0, u0 = torch.randn(B, n, generator=g).to(BF16), torch.randn(B, n, generator=g).to(BF16)
        r_prev = _launch(ops, gpu, x, p0, u0, None, s, eta, tau, 0.0, off=off)[2]
        assert torch.equal(r_prev, p0.float() - u0.float())    # β = 0: one fp32 subtraction of the widened halves, on both sides
        beta = -0.5
    run = lambda: _launch(ops, gpu, x, p, u, None if r_prev is None else _place(r_prev, gpu, off), s, eta, tau, beta, h if multi else None, w, mask, src,
                          noise, sn, off)
    got, gb, gd, part, gh, _ = run()
    again = run()
    for a_, b_ in zip((got, gb, gd, part, gh), again[:5]):     # a repeated launch repeats its bits
        assert a_ is None or torch.equal(_bits(a_), _bits(b_))
    # ---- the sums
    P, D_ = p.double(), (p.double() - u.double()).abs() + (abs(beta) * r_prev.double().abs() if r_prev is not None else 0.0)
    v64, d64 = projected_velocity(p, u, r_prev, beta, s, eta, tau)
    Rd = 3 if beta != 0.0 else 1
    sums = part.double().sum(dim=1)                           # [B, 3]: the partials in index order, as the step's prologue adds them
    a64, b64, c64 = (d64 * d64).sum(1), (d64 * P).sum(1), (P * P).sum(1)
    Sa, Sb, Sc = (D_ * D_).sum(1), (D_ * P.abs()).sum(1), (P * P).sum(1)
    dbl = 150 * 2.0 ** -53
    Da, Db, Dc = (gamma(2 * Rd + 25) + dbl) * Sa, (gamma(Rd + 25) + dbl) * Sb, (gamma(25) + dbl) * Sc
    for name, gpu_sum, ref, bound, scale in (("a", sums[:, 0], a64, Da, Sa), ("b", sums[:, 1], b64, Db, Sb), ("c", sums[:, 2], c64, Dc, Sc)):
        worst = float(((gpu_sum - ref).abs() / (U * scale).clamp_min(1e-300)).max())
        print(f"[projected step] {case} {form} B={B} n={n}+{off}: sum {name} worst |Δ| / (2^-24 Σ|term|) = {worst:.3f} (bound {float((bound / (U * scale).clamp_min(1e-300)).max()):.1f})")
        assert bool(((gpu_sum - ref).abs() <= bound).all()), (name, worst)
    if case == "orthogonal":
        assert bool((sums[:, 1] == 0).all()) and bool((part[:, :, 1] == 0).all())
    # ---- k, e and their propagated error
    active = (a64 > tau * tau) & (tau > 0)
    assert bool(active.all()) == (case in ("clamp_on", "momentum")) and bool(active.any()) == bool(active.all())
    k64 = torch.where(active, tau / a64.sqrt(), torch.ones_like(a64))
    eps = Da / a64
    dk = torch.where(active, k64 * (eps / (2 * (1 - eps)) + U), torch.zeros_like(a64))
    e64 = (eta - 1.0) * k64 * b64 / c64
    de = abs(eta - 1.0) * (dk * (b64.abs() + Db) / (c64 - Dc) + k64 * Db / (c64 - Dc) + k64 * b64.abs() * Dc / (c64 * (c64 - Dc))) + U * e64.abs()
    col = lambda t: t[:, None]
    prop = abs(S1) * (D_ * col(dk) + P.abs() * col(de))
    V = P.abs() + abs(S1) * (col(k64) * D_ + col(e64.abs()) * P.abs())
    Ev = gamma(5 + Rd) * V + prop
    # ---- the difference, the velocity (through the history) and the state
    assert bool(((gd.double() - d64).abs() <= gamma(Rd) * D_).all())
    H = h.double() if multi else torch.zeros_like(P)
    vel2 = v64 + w * (v64 - H) if w != 0.0 else v64
    r = x.double() + ds * vel2
    M = x.double().abs() + abs(ds) * (V + abs(w) * (V + H.abs()))
    R = 10 + Rd
    if mask is not None:
        keep = (1.0 - sn) * src.double() + sn * noise.double()
        m = mask.double().expand_as(x)
        r, M, R = (1.0 - m) * keep + m * r, M + src.double().abs() + noise.double().abs(), R + 8
    bound = gamma(R) * M + abs(ds) * (1 + abs(w)) * prop
    ratio = float(((got.double() - r).abs() / bound.clamp_min(1e-300)).max())
    rounding = float(((got.double() - r).abs() / (U * M).clamp_min(1e-300)).max())
    print(f"[projected step] {case} {form} B={B} n={n}+{off}: state worst |o - o64| = {ratio:.3f} of its bound, {rounding:.3f} x 2^-24 M (R = {R})")
    assert bool(((got.double() - r).abs() <= bound).all()), ratio
    assert not torch.equal(got, x)
    if multi:
        vr = float(((gh.double() - v64).abs() / Ev.clamp_min(1e-300)).max())
        print(f"[projected step] {case} {form} B={B} n={n}+{off}: v worst |v - v64| = {vr:.3f} of its bound")
        assert bool(((gh.double() - v64).abs() <= Ev).all()), vr
    assert torch.equal(_bits(gb), _bits(got.to(BF16)))         # bf16 of the kernel's own fp32 result
    if case == "cancel":
        assert torch.equal(v64, P)                              # k·p/2 − (k/2)·p = 0 in any precision: the reference's v is p itself
    elif case != "orthogonal":                                  # (d ⟂ p without a clamp: the projection leaves the plain mix as it is)
        # the projection is felt: the plain mix u + s·(p − u) lies outside the bound somewhere
        mix = u.double() + s * (p.double() - u.double())
        assert bool(((mix - v64).abs() > Ev).any())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_projected_step_against_fp64_generic(gpu, shape, form):
    from reptext_amd import ops

    B, n, off = shape
    _check(ops, gpu, B, n, off, "generic", form, seed=n % 1000 + 10 * B + FORMS.index(form) + 100 * off)


@pytest.mark.parametrize("case", CASES[1:])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_projected_step_against_fp64_cases(gpu, shape, case):
    from reptext_amd import ops

    B, n, off = shape
    _check(ops, gpu, B, n, off, case, "multi", seed=n % 1000 + 10 * B + 7 * CASES.index(case) + 100 * off)


# ------------------------------------------------------------------------------------------------------------------ bitwise properties
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_equal_halves_are_the_euler_step_on_p_bit_for_bit(gpu, shape):
    """u == p: d = 0, so k = 1, e = 0 and v = p + (s − 1)·0 = p for any s, η, τ — the state and its bf16 copy are rt_euler_step_f32's."""
    from reptext_amd import ops

    B, n, off = shape
    x, p, _, _, _, _, _ = _inputs(B, n, 300 + n % 1000, "generic", "plain")
    a32, ab = _place(x, gpu, off), _place(torch.zeros(B, n, dtype=BF16), gpu, off)
    ops.euler_step_f32_(a32, _place(p, gpu, off), DS, ab)
    for s, eta, tau in ((3.5, 0.0, 0.0), (7.0, 0.5, 0.125), (1.5, 1.0, 1000.0), (2.0, -1.0, 1e-3)):
        got, gb, gd, part, _, _ = _launch(ops, gpu, x, p, p.clone(), None, s, eta, tau, 0.0, off=off)
        assert torch.equal(_bits(got), _bits(a32.cpu())) and torch.equal(_bits(gb), _bits(ab.cpu())), (s, eta, tau)
        assert bool((gd == 0).all()) and bool((part[:, :, :2] == 0).all())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_zero_momentum_never_reads_the_difference(gpu, shape):
    """β = 0 with a diff buffer full of NaN (what ``_launch`` allocates): no NaN reaches the sums, the state or the history, and the
    buffer holds d afterwards — the same bits as with a buffer of zeros and β = 0."""
    from reptext_amd import ops

    B, n, off = shape
    x, p, u, h, _, _, _ = _inputs(B, n, 400 + n % 1000, "generic", "multi")
    got, gb, gd, part, gh, _ = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 1.0, 0.0, h, W, off=off)
    for t in (got, gd, part, gh):
        assert bool(torch.isfinite(t).all())
    zeros = _place(torch.zeros(B, n), gpu, off)
    other = _launch(ops, gpu, x, p, u, zeros, 3.5, 0.25, 1.0, 0.0, h, W, off=off)
    for a_, b_ in zip((got, gb, gd, part, gh), other[:5]):
        assert torch.equal(_bits(a_), _bits(b_))
    assert torch.equal(gd, p.float() - u.float())


@pytest.mark.parametrize("n", [4032, 4160, 12289])
def test_a_sample_does_not_depend_on_the_batch(gpu, n):
    """Sample 1 of a B = 2 launch equals the B = 1 launch on that sample: sums, difference, state, history (one mask per sample)."""
    from reptext_amd import ops

    x, p, u, h, src, noise, mask = _inputs(2, n, 500 + n % 1000, "generic", "repaint_multi")
    both = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, h, W, mask, src, noise)
    one = _launch(ops, gpu, x[1:], p[1:], u[1:], None, 3.5, 0.25, 20.0, 0.0, h[1:], W, mask[1:], src[1:], noise[1:])
    for a_, b_ in zip(both[:5], one[:5]):
        assert torch.equal(_bits(a_[1:]), _bits(b_))


@pytest.mark.parametrize("n", [64, 4096, 16384])
def test_aligned_and_misaligned_runs_agree(gpu, n):
    """The same data through the 16-byte path and, at an element offset of 1, through the one-element path: the same sums, the same
    difference, the same state, bf16 copy and history; with momentum too."""
    from reptext_amd import ops

    x, p, u, h, src, noise, mask = _inputs(2, n, 600 + n, "generic", "repaint_shared_multi")
    outs = []
    for off in (0, 1):
        first = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, h, W, mask, src, noise, off=off)
        second = _launch(ops, gpu, first[0], u, p, first[5], 3.5, 0.25, 20.0, -0.5, first[4], W, mask, src, noise, off=off)
        outs.append(first[:5] + second[:5])
    for a_, b_ in zip(*outs):
        assert torch.equal(_bits(a_), _bits(b_))


@pytest.mark.parametrize("shape", SHAPES[1:4], ids=IDS[1:4])
def test_a_mask_of_ones_is_the_form_without_a_mask(gpu, shape):
    from reptext_amd import ops

    B, n, off = shape
    x, p, u, h, src, noise, _ = _inputs(B, n, 700 + n % 1000, "generic", "repaint_multi")
    want = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, h, W, off=off)
    for ones in (torch.ones(B, n), torch.ones(1, n)):
        got = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, h, W, ones, src, noise, off=off)
        for a_, b_ in zip(want[:5], got[:5]):
            assert torch.equal(_bits(a_), _bits(b_))


@pytest.mark.parametrize("shape", SHAPES[1:4], ids=IDS[1:4])
def test_zero_weight_is_the_form_without_history_and_writes_the_velocity(gpu, shape):
    """w = 0 with a history full of NaN: the state of the launch without a history, and hist = v — the bits a launch with w != 0 writes."""
    from reptext_amd import ops

    B, n, off = shape
    x, p, u, h, _, _, _ = _inputs(B, n, 800 + n % 1000, "generic", "multi")
    want = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, off=off)
    got = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, torch.full_like(h, float("nan")), 0.0, off=off)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    assert bool(torch.isfinite(got[4]).all())
    second_order = _launch(ops, gpu, x, p, u, None, 3.5, 0.25, 20.0, 0.0, h, W, off=off)
    assert torch.equal(_bits(got[4]), _bits(second_order[4])) and not torch.equal(second_order[0], want[0])


def test_scheduler_step_master_projected_is_the_op(gpu):
    """Both schedulers' ``step_master_(projected=)``: the op with the schedule's dσ (and the multistep weight), momentum 0 on a first step."""
    from reptext_amd import ops
    from reptext_amd.guidance import ProjectedStep
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler, multistep_weights

    B, n = 2, 4160
    x, p, u, h, _, _, _ = _inputs(B, n, 900, "generic", "multi")
    dev = lambda t: t.to(gpu)
    for cls in (FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler):
        sc = cls()
        sc.set_timesteps(sigmas=[1.0, 0.75, 0.5], mu=1.0)
        multi = cls is FlowMatchMultistepScheduler
        wts = multistep_weights(sc.sigmas) if multi else [0.0, 0.0]
        a32, ab, ah = dev(x), torch.zeros(B, n, dtype=BF16, device=gpu), torch.empty(B, n, device=gpu)
        b32, bb, bh = dev(x), torch.zeros(B, n, dtype=BF16, device=gpu), torch.empty(B, n, device=gpu)
        rec = ProjectedStep(0.25, 20.0, -0.5, torch.empty(B, n, device=gpu), torch.empty(ops.guidance_partials_shape(B, n), device=gpu))
        diff, part = torch.empty(B, n, device=gpu), torch.empty(ops.guidance_partials_shape(B, n), device=gpu)
        for i, (pp, uu) in enumerate(((p, u), (u, p))):
            sc.step_master_(dev(uu), a32, ab, v_text=dev(pp), s=3.5, projected=rec, **(dict(history=ah) if multi else {}))
            rec.first = False
            ops.projected_step_f32_(b32, dev(uu), dev(pp), diff, part, 3.5, 0.25, 20.0, 0.0 if i == 0 else -0.5, float(sc.sigmas[i + 1] - sc.sigmas[i]), bb,
                                    **(dict(hist32=bh, w=wts[i]) if multi else {}))
            assert torch.equal(a32, b32) and torch.equal(ab, bb) and torch.equal(rec.diff, diff)
        assert sc._step_index == 2
