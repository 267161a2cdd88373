"""rt_repaint_euler_step_f32 (csrc/norm_elem.hip): the latent blend of a repaint fused into the fp32 master Euler step. Per element

    vel  = v_text ? u + s·(t − u) : v            u = v, t = v_text, bf16 widened
    r    = x + dσ·vel
    keep = (1 − σn)·src + σn·noise
    o    = (1 − m)·keep + m·r,   m = mask[i % n_mask]

against fp64 on the values the kernel reads (inputs rounded on the CPU to bf16 / fp32, the scalars to C floats):

    |o − o64| <= R · 2^-24 · (|x| + |dσ·vel| + |src| + |noise|)

R counts the fp32 roundings of the expression: dσ·vel, x + ·, 1 − σn, (1 − σn)·src, σn·noise, their sum, 1 − m, (1 − m)·keep, m·r and
the last sum — R = 10; the CFG mix adds t − u, s·(·) and u + · — R = 13. Each is relative 2^-24 of a partial result that the
magnitude bounds for m and σn in [0, 1]; where the compiler fuses a multiply-add a rounding disappears, none is added.

The sizes: a per-sample length n of 64, 16384 and 16384·3 + 64 at batch 1 and at batch 3 (n_mask = the whole length, and n_mask = the
per-sample length: one mask for the batch), all on the 4-element vector path; 67 per sample, no multiple of 4: with a mask of the
state's length (67, or 201 at batch 3) the vector path runs and leaves a tail of 3 or 1 elements, with one mask of period 67 for a
batch of 3 a group of four could straddle the period and every element takes the one-element path; and two sizes past
4 · 4096 · 256 elements, where the 16-byte loop's grid stride wraps (4096 blocks of 256 threads are the launch's cap): one whose
shared mask's period is a multiple of 4, so that ``(4g) % n_mask`` wraps in the vector loop too, and one with three elements left
over for the tail. The bitwise edges: m = 1 is rt_euler_step_f32 / rt_cfg_euler_step_f32, m = 0 gives keep as torch computes it, and with σn = 0
the source; a [1, n] mask is the same mask repeated. The refusals and the derived binding need no device and are not marked gpu."""
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
SIZES = [64, 67, 16384, 16384 * 3 + 64]
LAYOUTS = [(1, False), (3, False), (3, True)]            # (batch, one mask for the batch)
DS, SN, S = -0.0116, 0.6543, 3.5


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _inputs(B, n, seed, shared_mask):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, u, t, src, noise = rn(B, n), rn(B, n).to(BF16), rn(B, n).to(BF16), rn(B, n), rn(B, n)
    mask = torch.rand(1 if shared_mask else B, n, generator=g)
    return x, u, t, src, noise, mask


def _fp64(x, u, t, src, noise, mask, s, ds, sn):
    """(o64, magnitude) of the expression; ``t`` None: no CFG mix."""
    d = lambda a: a.double()
    vel = d(u) if t is None else d(u) + s * (d(t) - d(u))
    r = d(x) + ds * vel
    keep = (1.0 - sn) * d(src) + sn * d(noise)
    m = d(mask).expand_as(x)
    return (1.0 - m) * keep + m * r, d(x).abs() + (ds * vel).abs() + d(src).abs() + d(noise).abs()


def _run(ops, gpu, x, u, t, src, noise, mask, with_bf16, s=S, ds=DS, sn=SN):
    x32 = x.to(gpu)
    xb = torch.full(x.shape, 12345.0, dtype=BF16, device=gpu) if with_bf16 else None
    out = ops.repaint_euler_step_f32_(x32, u.to(gpu), None if t is None else t.to(gpu), s, ds, sn, src.to(gpu), noise.to(gpu), mask.to(gpu), xb)
    assert out is x32
    return x32.cpu(), None if xb is None else xb.cpu()


def _check_against_fp64(ops, gpu, B, n, shared_mask, cfg, with_bf16, seed):
    x, u, t, src, noise, mask = _inputs(B, n, seed, shared_mask)
    t = t if cfg else None
    ds, sn, s = _f32(DS), _f32(SN), _f32(S)
    ref, M = _fp64(x, u, t, src, noise, mask, s, ds, sn)
    R = 13 if cfg else 10
    got, gb = _run(ops, gpu, x, u, t, src, noise, mask, with_bf16)
    again, ab = _run(ops, gpu, x, u, t, src, noise, mask, with_bf16)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))          # twice: the same bits
    ratio = float(((got.double() - ref).abs() / (2.0 ** -24 * M).clamp_min(1e-300)).max())
    print(f"[repaint step] B={B} n={n} shared_mask={shared_mask} cfg={cfg} bf16={with_bf16}: worst |o - o64| / (2^-24 M) = {ratio:.3f} (bound {R})")
    assert bool(((got.double() - ref).abs() <= R * 2.0 ** -24 * M).all()), ratio
    assert not torch.equal(got, x)
    if with_bf16:
        assert torch.equal(gb.view(torch.int16), got.to(BF16).view(torch.int16))  # bf16 of the kernel's own fp32 result
        assert torch.equal(gb.view(torch.int16), ab.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("B,shared_mask", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_repaint_step_against_fp64_per_element(gpu, n, B, shared_mask, cfg, with_bf16):
    from reptext_amd import ops

    _check_against_fp64(ops, gpu, B, n, shared_mask, cfg, with_bf16, seed=n % 1000 + 10 * B + 4 * shared_mask + 2 * cfg + with_bf16)


WRAP = 4 * (4096 * 256 + 1000)                          # 1000 groups of four more than one pass of the largest grid takes


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,shared_mask", [(3, WRAP // 2, True), (1, WRAP + 3, False)])
def test_repaint_step_where_the_grid_stride_loop_wraps(gpu, B, n, shared_mask):
    """4096 blocks of 256 threads are the launch's cap: with more than 4096 · 256 groups of four a thread of the 16-byte loop takes a
    second group. Batch 3 with one mask of WRAP / 2 elements (a multiple of 4): 1.5 passes of the grid, the mask's index wraps twice
    inside the vector loop. Batch 1 with a mask of the state's length, WRAP + 3: the vector loop wraps and the three elements after the
    last group take the one-element tail of the same launch."""
    from reptext_amd import ops

    assert (B * n) // 4 > 4096 * 256 and (n % 4 == 0 or not shared_mask)          # the vector path, past one pass of the grid
    _check_against_fp64(ops, gpu, B, n, shared_mask, True, True, seed=5 + B)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_mask_of_ones_is_the_plain_step_bit_for_bit(gpu, n, cfg):
    from reptext_amd import ops

    x, u, t, src, noise, _ = _inputs(3, n, 100 + n % 1000, False)
    t = t if cfg else None
    got, gb = _run(ops, gpu, x, u, t, src, noise, torch.ones(3, n), True)
    a32, ab = x.to(gpu), torch.zeros(3, n, dtype=BF16, device=gpu)
    if cfg:
        ops.cfg_euler_step_f32_(a32, u.to(gpu), t.to(gpu), S, DS, ab)
    else:
        ops.euler_step_f32_(a32, u.to(gpu), DS, ab)
    assert torch.equal(got.view(torch.int32), a32.cpu().view(torch.int32))
    assert torch.equal(gb.view(torch.int16), ab.cpu().view(torch.int16))
    assert not torch.equal(got, x)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_mask_of_zeros_gives_the_renoised_source_and_at_sigma_zero_the_source(gpu, n, cfg):
    """m = 0: the state is keep = (1 − σn)·src + σn·noise, each product and the sum rounded once — what torch computes, and what
    FlowMatchEulerDiscreteScheduler.scale_noise(src, σn, noise) returns; at σn = 0 it is the source."""
    from reptext_amd import ops
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    x, u, t, src, noise, _ = _inputs(3, n, 200 + n % 1000, False)
    t = t if cfg else None
    zeros = torch.zeros(1, n)
    got, gb = _run(ops, gpu, x, u, t, src, noise, zeros, True)
    sn = _f32(SN)
    keep = (1.0 - sn) * src + sn * noise
    assert torch.equal(got, keep) and torch.equal(gb, keep.to(BF16))
    assert torch.equal(got, FlowMatchEulerDiscreteScheduler().scale_noise(src, sn, noise))
    on_device = FlowMatchEulerDiscreteScheduler().scale_noise(src.to(gpu), sn, noise.to(gpu))
    assert torch.equal(got, on_device.cpu())
    got0, gb0 = _run(ops, gpu, x, u, t, src, noise, zeros, True, sn=0.0)
    assert torch.equal(got0, src) and torch.equal(gb0, src.to(BF16))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_one_mask_for_the_batch_is_the_mask_repeated(gpu, n):
    from reptext_amd import ops

    x, u, t, src, noise, mask = _inputs(3, n, 300 + n % 1000, True)
    one, oneb = _run(ops, gpu, x, u, t, src, noise, mask, True)
    rep, repb = _run(ops, gpu, x, u, t, src, noise, mask.expand(3, n).contiguous(), True)
    assert torch.equal(one.view(torch.int32), rep.view(torch.int32)) and torch.equal(oneb.view(torch.int16), repb.view(torch.int16))
    assert not torch.equal(one[0], one[1])


@pytest.mark.gpu
def test_scheduler_step_master_repaint_takes_both_sigmas_and_honours_the_begin_index(gpu):
    from reptext_amd import ops
    from reptext_amd.pipeline import Repaint
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    x, u, t, src, noise, mask = _inputs(2, 1000, 7, True)
    dev = lambda a: a.to(gpu)
    for begin in (None, 1):
        for cfg in (False, True):
            sc = FlowMatchEulerDiscreteScheduler()
            sc.set_timesteps(sigmas=[1.0, 0.6, 0.3], mu=0.5)
            first = 0
            if begin is not None:
                sc.set_begin_index(begin)
                first = begin
            a32, ab, b32 = dev(x), torch.zeros(2, 1000, dtype=BF16, device=gpu), dev(x)
            for i in range(first, 3):
                sc.step_master_(dev(u), a32, ab, v_text=dev(t) if cfg else None, s=2.0 if cfg else None, repaint=Repaint(dev(src), dev(noise), dev(mask)))
                ops.repaint_euler_step_f32_(b32, dev(u), dev(t) if cfg else None, 2.0, float(sc.sigmas[i + 1] - sc.sigmas[i]), float(sc.sigmas[i + 1]),
                                            dev(src), dev(noise), dev(mask))
                assert sc.step_index == i + 1
                assert torch.equal(a32, b32) and torch.equal(ab, a32.to(BF16))
            plain = FlowMatchEulerDiscreteScheduler()
            plain.set_timesteps(sigmas=[1.0, 0.6, 0.3], mu=0.5)
            if begin is not None:
                plain.set_begin_index(begin)
            plain.step_master_(dev(u), dev(x))
            assert plain.step_index == first + 1


def test_ops_refuse_shapes_that_do_not_fit():
    """Argument checks of ops.repaint_euler_step_f32_, as cfg_euler_step_f32_ makes them: raised before the device is touched."""
    from reptext_amd import ops

    x, v = torch.zeros(2, 8), torch.zeros(2, 8, dtype=BF16)
    ok = dict(x32=x, v=v, v_text=None, s=1.0, dsigma=-0.1, sigma_next=0.5, src32=x.clone(), noise32=x.clone(), mask=torch.zeros(1, 8))
    for bad in (dict(v=torch.zeros(2, 4, dtype=BF16)), dict(src32=torch.zeros(2, 4)), dict(noise32=torch.zeros(8, 2).t()),
                dict(v_text=torch.zeros(1, 8, dtype=BF16)), dict(mask=torch.zeros(2, 4)), dict(mask=torch.zeros(8)),
                dict(x_bf16=torch.zeros(2, 4, dtype=BF16))):
        with pytest.raises(ValueError):
            ops.repaint_euler_step_f32_(**{**ok, **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.repaint_euler_step_f32_(**ok)


def test_entry_point_refuses_null_pointers_and_masks_that_do_not_divide():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                       # never dereferenced: every call is refused first

    def call(x=P, v=P, vt=None, xb=None, src=P, noise=P, mask=P, n=64, n_mask=64):
        return lib.rt_repaint_euler_step_f32(x, v, vt, xb, src, noise, mask, 3.5, -0.01, 0.5, n, n_mask, None)

    for name in ("x", "v", "src", "noise", "mask"):
        assert call(**{name: None}) == native.RT_E_BADARG == -1, name
        assert call(**{name: None}, vt=P, xb=P) == -1, name
    assert call(n=0) == -1 and call(n=-5) == -1
    assert call(n_mask=0) == -1 and call(n_mask=-64) == -1
    assert call(n_mask=48) == native.RT_E_SHAPE and call(n_mask=128) == native.RT_E_SHAPE and call(n=65, n_mask=64, vt=P) == native.RT_E_SHAPE
    with pytest.raises(native.NativeCallError, match="rt_repaint_euler_step_f32 failed: RT_E_BADARG"):
        native.call("rt_repaint_euler_step_f32", None, None, None, None, None, None, None, 1.0, 0.0, 0.0, 8, 8, None)
    with pytest.raises(native.NativeCallError, match="rt_repaint_euler_step_f32 failed: RT_E_SHAPE"):
        native.call("rt_repaint_euler_step_f32", P, P, None, None, P, P, P, 1.0, 0.0, 0.0, 8, 3, None)
    C = __import__("ctypes")
    assert native.SIGNATURES["rt_repaint_euler_step_f32"] == [C.c_void_p] * 7 + [C.c_float] * 3 + [C.c_int64, C.c_int64, C.c_void_p]
