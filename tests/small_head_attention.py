"""The harness the GPU tests of rt_attention_hd64 and rt_attention_hd72 share (csrc/attention_small_head.hip): seeded inputs inside
NaN guards with their fp64 result and a CPU emulation of the kernel's roundings, and the launches that must all give the same bits.
A plain helper module, imported by tests/test_image_encoder_gpu.py (heads of 64) and tests/test_siglip_encoder_gpu.py (heads of 72)."""
import functools
import os

import torch

PAD_COLS, PAD_ROWS = 64, 3


def _seed(hd, B, Sq, Sk, H):
    """The seeds each test file has used since its kernel was added, so the errors recorded in their docstrings stay comparable."""
    return 1000 * Sk + 10 * H + B if hd == 64 else 100000 * Sq + 100 * Sk + 10 * H + B


@functools.lru_cache(maxsize=None)
def case(hd, B, Sq, Sk, H, shared, q_gain):
    """(fused q|k|v buffer bf16 [B, Sk + 3, 3·hd·H + 64] on the CPU whose extra rows and columns are NaN; fp64 softmax(scale·qkᵀ)v
    from its bf16 values; the same through a CPU emulation of the kernel's roundings; the largest scale·score). The queries are
    rows < Sq of the q columns, of batch entry 0 alone when they are shared."""
    g = torch.Generator().manual_seed(_seed(hd, B, Sq, Sk, H))
    d, scale = H * hd, hd ** -0.5
    vals = torch.randn(B, Sk, 3 * d, generator=g)
    vals[..., :d] *= q_gain
    buf = torch.full((B, Sk + PAD_ROWS, 3 * d + PAD_COLS), float("nan"), dtype=torch.bfloat16)
    buf[:, :Sk, :3 * d] = vals.to(torch.bfloat16)
    heads = lambda t: t.reshape(t.shape[0], t.shape[1], H, hd).transpose(1, 2)
    q = heads(buf[:1 if shared else B, :Sq, :d])
    k, v = heads(buf[:, :Sk, d:2 * d]), heads(buf[:, :Sk, 2 * d:3 * d])
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    ref = (torch.softmax(s, dim=-1) @ v.double()).transpose(1, 2).reshape(B, Sq, d)
    # the kernel's roundings: fp32 scores, exp against the row maximum, the row sum from the unrounded P, P rounded to bf16 before the
    # second product, o rounded to bf16
    s32 = q.float() @ k.float().transpose(-1, -2)
    p = torch.exp((s32 - s32.amax(dim=-1, keepdim=True)) * scale)
    emu = ((p.to(torch.bfloat16).float() @ v.float()) / p.sum(dim=-1, keepdim=True)).to(torch.bfloat16)
    emu = emu.expand(B, -1, -1, -1).transpose(1, 2).reshape(B, Sq, d)
    return buf, ref, emu, float(s.amax(dim=-1).max())


def fused(gpu, hd, buf, B, Sq, Sk, H, shared):
    """rt_attention_hd<hd> on views of the fused buffer, into a wider and taller buffer of sentinels: twice as the host would launch
    it and once per forced workgroup size. Checks what must not be written and that every launch gives the same bits."""
    from reptext_amd import ops

    d, env = H * hd, f"RT_HD{hd}_WAVES"
    attention = ops.attention_hd64 if hd == 64 else ops.attention_hd72
    dev = buf.to(gpu)
    q = dev[:1 if shared else B, :Sq, :d]
    ldo, rows = d + 64, Sq + 3
    sentinel = torch.full((B, rows, ldo), -7.0, dtype=torch.bfloat16)
    outs = []
    try:
        for force in (None, None, "1", "2", "4"):
            if force is not None:
                os.environ[env] = force
            o = sentinel.to(gpu)
            attention(q, dev[:, :Sk, d:2 * d], dev[:, :Sk, 2 * d:3 * d], o[:, :Sq, :d], H, hd ** -0.5)
            torch.cuda.synchronize()
            outs.append(o.cpu())
    finally:
        os.environ.pop(env, None)
    out = outs[0]
    assert torch.equal(out[:, :, d:], sentinel[:, :, d:]) and torch.equal(out[:, Sq:], sentinel[:, Sq:])    # columns >= hd·H, rows >= Sq
    assert torch.isfinite(out.float()).all()                                     # a read of a guard row or column would be a NaN
    for other in outs[1:]:
        assert torch.equal(out, other)                                           # a second launch, and every workgroup size: the same bits
    assert torch.equal(dev.cpu().view(torch.int16), buf.view(torch.int16))      # the inputs are not modified
    return out[:, :Sq, :d]


def is_v(out, buf, hd, B, Sq, H):
    """With one key the output is v, bit for bit."""
    d = H * hd
    return torch.equal(out.view(torch.int16), buf[:, :1, 2 * d:3 * d].expand(B, Sq, d).contiguous().view(torch.int16))
