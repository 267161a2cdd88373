"""rt_cfg_euler_step_f32 (csrc/norm_elem.hip): the true-CFG mix fused into the fp32 master Euler step,
x[i] += dsigma · (u + s·(t − u)), u / t bf16, everything in fp32.

Per element against fp64 on the values the kernel reads (inputs rounded on the CPU to bf16 / fp32, the scalars to C floats):

    |got − ref| <= 5 · 2^-24 · M,    M = |x| + |ds|·(|u| + |s|·(|u| + |t|))

At most five fp32 roundings (t − u, s·(..), u + .., ds·v, x + ..; fewer where the compiler fuses a multiply-add), each relative 2^-24 of
a partial result that is bounded by its share of M. The bf16 copy is exactly bf16 of the kernel's own fp32 result, and with t == u the
kernel is rt_euler_step_f32 on u bit for bit, for any s. The refusals need no device and are not marked gpu."""
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
WRAP = 4 * (4096 * 256 + 1000)                 # 1000 groups of four more than one pass of the largest grid (4096 blocks of 256) takes
# the kernel takes groups of four (16-byte accesses), then what is left one at a time: no group; a tail alone; one group; a group and a
# tail; 16 groups and 3; around a block's worth; two 256x64 latents' worth plus a tail; the vector loop's grid stride wraps, then 3
SIZES = [1, 3, 4, 5, 67, 255, 257, 2 * 256 * 64 + 3, WRAP + 3]
SCALES = [0.0, 1.0, 3.5]
DS = -0.0116


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g).to(BF16), torch.randn(n, generator=g).to(BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("n", SIZES)
def test_cfg_euler_step_against_fp64_per_element(gpu, n, s, with_bf16):
    from reptext_amd import ops

    x, u, t = _inputs(n, n % 1000 + int(10 * s) + with_bf16)
    ds, sc = _f32(DS), _f32(s)
    ref = x.double() + ds * (u.double() + sc * (t.double() - u.double()))
    M = x.double().abs() + abs(ds) * (u.double().abs() + abs(sc) * (u.double().abs() + t.double().abs()))
    du, dt = u.to(gpu), t.to(gpu)
    outs = []
    for _ in range(2):                                                # twice: the same bits
        x32 = x.to(gpu)
        xb = torch.full((n,), 12345.0, dtype=BF16, device=gpu) if with_bf16 else None
        assert ops.cfg_euler_step_f32_(x32, du, dt, s, DS, xb) is x32
        outs.append((x32.cpu(), None if xb is None else xb.cpu()))
    got = outs[0][0]
    assert torch.equal(got.view(torch.int32), outs[1][0].view(torch.int32))
    ratio = float(((got.double() - ref).abs() / (2.0 ** -24 * M).clamp_min(1e-300)).max())
    print(f"[cfg step] n={n} s={s} bf16={with_bf16}: worst |got - ref| / (2^-24 M) = {ratio:.3f} (bound 5)")
    assert bool(((got.double() - ref).abs() <= 5 * 2.0 ** -24 * M).all()), ratio
    assert torch.equal(du.cpu().view(torch.int16), u.view(torch.int16)) and torch.equal(dt.cpu().view(torch.int16), t.view(torch.int16))
    if with_bf16:
        assert torch.equal(outs[0][1].view(torch.int16), got.to(BF16).view(torch.int16))      # bf16 of the kernel's own fp32 result
        assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [0.0, 1.0, 3.5, -2.0])
@pytest.mark.parametrize("n", SIZES)
def test_equal_halves_are_the_plain_step_bit_for_bit(gpu, n, s):
    """t holds u's values (another tensor): u + s·(t − u) = u exactly, and the step is rt_euler_step_f32's, fp32 state and bf16 copy."""
    from reptext_amd import ops

    x, u, _ = _inputs(n, 77 + n % 1000)
    du, dt = u.to(gpu), u.clone().to(gpu)
    a32, ab = x.to(gpu), torch.zeros(n, dtype=BF16, device=gpu)
    b32, bb = x.to(gpu), torch.zeros(n, dtype=BF16, device=gpu)
    ops.euler_step_f32_(a32, du, DS, ab)
    ops.cfg_euler_step_f32_(b32, du, dt, s, DS, bb)
    assert torch.equal(a32.view(torch.int32), b32.view(torch.int32))
    assert torch.equal(ab.view(torch.int16), bb.view(torch.int16))
    assert not torch.equal(a32.cpu(), x)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("n", [67, 16384])
@pytest.mark.parametrize("cfg", [False, True])
def test_vector_and_one_element_paths_agree_bit_for_bit(gpu, cfg, n, with_bf16):
    """The same values through aligned tensors (the 16-byte path, at n = 67 with its tail) and through contiguous views that start one
    element into their buffers (4 bytes off for fp32, 2 for bf16): there no 16-byte access is possible and every element takes the
    one-element path. Both entries, rt_euler_step_f32 and rt_cfg_euler_step_f32."""
    from reptext_amd import ops

    x, u, t = _inputs(n, 900 + n % 1000 + 2 * cfg + with_bf16)
    outs = []
    for off in (0, 1):
        place = lambda a: torch.cat([a[:off], a]).to(gpu)[off:]
        dx, du, dt = place(x), place(u), place(t)
        xb = place(torch.full((n,), 12345.0, dtype=BF16)) if with_bf16 else None
        assert all(a.is_contiguous() and (a.data_ptr() % 16 == 0) == (off == 0) for a in (dx, du, dt) + (() if xb is None else (xb,)))
        if cfg:
            ops.cfg_euler_step_f32_(dx, du, dt, 3.5, DS, xb)
        else:
            ops.euler_step_f32_(dx, du, DS, xb)
        outs.append((dx.cpu(), None if xb is None else xb.cpu()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert not torch.equal(outs[0][0], x)
    if with_bf16:
        assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
        assert torch.equal(outs[0][1].view(torch.int16), outs[0][0].to(BF16).view(torch.int16))


@pytest.mark.gpu
def test_scheduler_step_master_cfg_advances_like_step_master(gpu):
    from reptext_amd import ops
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    x, u, t = _inputs(1000, 5)
    scheds = [FlowMatchEulerDiscreteScheduler(), FlowMatchEulerDiscreteScheduler()]
    for sc in scheds:
        sc.set_timesteps(sigmas=[1.0, 0.6, 0.3], mu=0.5)
    a32, ab = x.to(gpu), torch.zeros(1000, dtype=BF16, device=gpu)
    b32 = x.to(gpu)
    for i in range(3):
        scheds[0].step_master_(u.to(gpu), a32, ab, v_text=t.to(gpu), s=2.0)
        ds = float(scheds[1].sigmas[i + 1] - scheds[1].sigmas[i])
        ops.cfg_euler_step_f32_(b32, u.to(gpu), t.to(gpu), 2.0, ds)
        scheds[1].step_master_(u.to(gpu), torch.zeros(1000, device=gpu))
        assert scheds[0].step_index == scheds[1].step_index == i + 1
        assert torch.equal(a32, b32) and torch.equal(ab, a32.to(BF16))


def test_entry_point_refuses_null_pointers_and_empty_sizes():
    from reptext_amd import native

    lib = native.load()
    P = 0x10000                                                       # never dereferenced: every call is refused first

    def call(x=P, u=P, t=P, xb=None, n=64):
        return lib.rt_cfg_euler_step_f32(x, u, t, xb, 3.5, -0.01, n, None)

    for name in ("x", "u", "t"):
        assert call(**{name: None}) == native.RT_E_BADARG == -1, name
    assert call(n=0) == -1 and call(n=-5) == -1
    assert call(xb=P, n=0) == -1
    with pytest.raises(native.NativeCallError, match="rt_cfg_euler_step_f32 failed: RT_E_BADARG"):
        native.call("rt_cfg_euler_step_f32", None, None, None, None, 1.0, 0.0, 8, None)
    C = __import__("ctypes")
    assert native.SIGNATURES["rt_cfg_euler_step_f32"] == [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_int64, C.c_void_p]
