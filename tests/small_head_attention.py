"""The harness the GPU tests of rt_attention_hd64 and rt_attention_hd72 share (csrc/attention_small_head.hip): seeded inputs inside
NaN guards with their fp64 result and a CPU emulation of the kernel's roundings, and the launches that must all give the same bits.
A plain helper module, imported by tests/test_image_encoder_gpu.py (heads of 64) and tests/test_siglip_encoder_gpu.py (heads of 72).
Further down, for tests/test_small_head_attention_edges_gpu.py and tests/test_small_head_refs_host.py: guarded(), the general launcher
(any Sq and Sk, q in the fused buffer or in one of its own, a q shared by the batch, any scale), and the key-selection construction."""
import functools
import os

import torch

from support_kernels import BF16, NAN, SENT, same_bits

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


KV_PAD_ROWS, Q_PAD_ROWS, Q_PAD_COLS, O_PAD_ROWS, O_PAD_COLS = 70, 20, 8, 3, 8
WAVES = (None, None, "1", "2", "4")


def _launches(gpu, hd, q, k, v, H, own_q, scale, forces):
    """One launch per entry of `forces` on freshly guarded buffers; returns the whole output buffers on the CPU. See guarded()."""
    from reptext_amd import ops

    (Bq, Sq, d), (B, Sk, _) = q.shape, k.shape
    assert d == H * hd and k.shape == v.shape == (B, Sk, d) and Bq in (1, B) and q.dtype == k.dtype == v.dtype == BF16
    attention = ops.attention_hd64 if hd == 64 else ops.attention_hd72
    if own_q:
        kvbuf = torch.full((B, Sk + KV_PAD_ROWS, 2 * d + PAD_COLS), NAN, dtype=BF16)
        kvbuf[:, :Sk, :d], kvbuf[:, :Sk, d:2 * d] = k, v
        qbuf = torch.full((Bq, Sq + Q_PAD_ROWS, d + Q_PAD_COLS), NAN, dtype=BF16)
        qbuf[:, :Sq, :d] = q
        kvdev, qdev = kvbuf.to(gpu), qbuf.to(gpu)
        qv, kv, vv = qdev[:, :Sq, :d], kvdev[:, :Sk, :d], kvdev[:, :Sk, d:2 * d]
        assert qv.stride(1) != kv.stride(1) and (Bq == 1 or qv.stride(0) != kv.stride(0))
    else:
        assert q.shape == k.shape, "the fused layout is self-attention: q rows are the key rows"
        kvbuf = torch.full((B, Sk + KV_PAD_ROWS, 3 * d + PAD_COLS), NAN, dtype=BF16)
        kvbuf[:, :Sk, :d], kvbuf[:, :Sk, d:2 * d], kvbuf[:, :Sk, 2 * d:3 * d] = q, k, v
        qbuf = qdev = None
        kvdev = kvbuf.to(gpu)
        qv, kv, vv = kvdev[:, :Sk, :d], kvdev[:, :Sk, d:2 * d], kvdev[:, :Sk, 2 * d:3 * d]
    sentinel = torch.full((B, Sq + O_PAD_ROWS, d + O_PAD_COLS), SENT, dtype=BF16)
    env = f"RT_HD{hd}_WAVES"
    before, outs = os.environ.get(env), []
    try:
        for force in forces:
            if force is None:
                os.environ.pop(env, None)
            else:
                os.environ[env] = force
            o = sentinel.to(gpu)
            attention(qv, kv, vv, o[:, :Sq, :d], H, scale)
            torch.cuda.synchronize()
            outs.append(o.cpu())
    finally:
        if before is None:
            os.environ.pop(env, None)
        else:
            os.environ[env] = before
    assert same_bits(kvdev.cpu(), kvbuf) and (qbuf is None or same_bits(qdev.cpu(), qbuf)), "the kernel wrote to its inputs"
    for o in outs:
        assert same_bits(o[:, :, d:], sentinel[:, :, d:]) and same_bits(o[:, Sq:], sentinel[:, Sq:]), "wrote outside [:, :Sq, :H*hd]"
        assert torch.isfinite(o.float()).all(), "non-finite output: a guard row or column was read"
    return outs


def guarded(gpu, hd, q, k, v, H, own_q=False, scale=None):
    """rt_attention_hd<hd> on CPU bf16 q [Bq, Sq, H·hd] (Bq = B, or 1: one q shared by the batch), k and v [B, Sk, H·hd], the general
    launcher beside fused(). On the device k and v are views of one NaN-filled [B, Sk + 70, row] buffer (70 NaN rows behind Sk: more
    than a key tile; the row is wider than its operands by 64 NaN columns; a padded batch stride). own_q False: the fused layout,
    q | k | v side by side in that buffer (Sq = Sk; the only form rt_attention_hd64 takes). own_q True: q is a view of its own
    NaN-filled [Bq, Sq + 20, H·hd + 8] buffer, so ldq != ldkv and the batch strides differ. The output is a view of a
    [B, Sq + 3, H·hd + 8] buffer of sentinels. Launched twice as the host would and once per forced workgroup size; every launch
    must give the same bits, leave the sentinels and the inputs as they were and write finite values; and entry b of a B > 1 launch
    must have the bits of the batch-1 launch of that entry. Returns the [B, Sq, H·hd] output on the CPU."""
    (Bq, Sq, d), B = q.shape, k.shape[0]
    outs = _launches(gpu, hd, q, k, v, H, own_q, scale, WAVES)
    for n, other in enumerate(outs[1:], 1):
        assert same_bits(outs[0], other), f"launch {n} (RT_HD{hd}_WAVES = {WAVES[n]}) differs from the first"
    if B > 1:
        for b in range(B):
            one = _launches(gpu, hd, q[b:b + 1] if Bq == B else q, k[b:b + 1], v[b:b + 1], H, own_q, scale, (None,))[0]
            assert same_bits(one[0], outs[0][b]), f"entry {b} differs from its batch-1 launch"
    return outs[0][:, :Sq, :d]


# ------------------------------------------------------------------------------------------------------ key selection, bit for bit
def selection_case(hd, B, Sq, Sk, H, seed):
    """Inputs whose softmax picks ONE key per query row, so that the output row has the bits of that key's v row. CPU bf16
    q [B, Sq, H·hd], k, v [B, Sk, H·hd] and pi [B, H, Sq] (long):
      k   rows of random signs, entries ±2
      q   row i of (b, h) = 4 · k[b, pi[b, h, i], h]: scale · score is 16 sqrt(hd) for the chosen key and 32 / sqrt(hd) lower per
          sign in which another key differs from it
      v   sign · uniform[0.5, 2), rounded to bf16
    Sq == Sk: pi is a permutation of the keys, one per (b, h). Otherwise it is a random map into the keys in which, spread over
    the B·H·Sq rows of the case (one head's Sq rows can be fewer than these keys), every one of key 0, key Sk - 1 and keys 64j,
    64j + 63 (= 64(j + 1) - 1) of every key tile j that has them is chosen at least once.
    Every tensor here is exact in bf16. selection_gap() states the precondition, selection_expected() the answer."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.randint(0, 2, (B, Sk, H, hd), generator=g) * 4 - 2).float()
    v = (torch.rand(B, Sk, H, hd, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (B, Sk, H, hd), generator=g) * 2 - 1)
    v = v.to(torch.bfloat16)
    if Sq == Sk:
        pi = torch.stack([torch.randperm(Sk, generator=g) for _ in range(B * H)]).reshape(B, H, Sq)
    else:
        need = sorted({0, Sk - 1} | {key for j in range((Sk + 63) // 64) for key in (64 * j, 64 * j + 63) if key < Sk})
        assert B * H * Sq >= len(need)
        pi = torch.randint(0, Sk, (B * H * Sq,), generator=g)
        pi[torch.randperm(B * H * Sq, generator=g)[:len(need)]] = torch.tensor(need)
        pi = pi.reshape(B, H, Sq)
    q = 4.0 * torch.gather(k.transpose(1, 2), 2, pi[..., None].expand(B, H, Sq, hd)).transpose(1, 2)      # [B, Sq, H, hd]
    bf = lambda t, S: t.reshape(B, S, H * hd).to(torch.bfloat16)
    return bf(q, Sq), bf(k, Sk), v.reshape(B, Sk, H * hd), pi


# (hd, B, Sq, Sk, H, q in its own buffer, seed): every shape the key-selection tests use, the two admitted maxima last. The seeds are
# part of the construction: tests/test_small_head_refs_host.py checks the precondition of each on the CPU.
SELECTION_CASES = [(64, 2, 65, 65, 2, False, 1), (64, 2, 257, 257, 2, False, 2), (72, 2, 65, 65, 2, False, 3), (72, 2, 729, 729, 2, False, 4),
                   (72, 2, 130, 63, 2, True, 5), (72, 2, 17, 729, 2, True, 6)]
SELECTION_MAXIMA = [(64, 1, 4096, 4096, 1, False, 7), (72, 1, 1024, 1024, 1, False, 8)]
MIN_GAP = 40.0


def selection_gap(q, k, pi, hd, scale=None):
    """(the smallest distance, over every query row, between scale · score of the row's chosen key and of the best other key, from
    the fp64 scores; whether the k rows of every (b, h) are pairwise distinct). A gap of 40 puts every other key's weight below
    e^-40 = 4e-18: Sk <= 4096 of them stay under 2e-14, far inside half an fp32 ulp (6e-8 relative) of the row sum and of
    any |v| >= 0.5."""
    (B, Sq, d), Sk = q.shape, k.shape[1]
    H = d // hd
    sc = hd ** -0.5 if scale is None else float(scale)
    qh, kh = q.double().reshape(B, Sq, H, hd), k.double().reshape(B, Sk, H, hd)
    gap, distinct = float("inf"), True
    for b in range(B):
        for h in range(H):
            s = qh[b, :, h] @ kh[b, :, h].t() * sc
            idx = pi[b, h][:, None]
            chosen = s.gather(1, idx)
            if Sk > 1:
                gap = min(gap, float((chosen - s.scatter(1, idx, float("-inf")).amax(dim=1, keepdim=True)).min()))
            distinct = distinct and torch.unique(kh[b, :, h], dim=0).shape[0] == Sk
    return gap, distinct


def selection_expected(v, pi, hd, swap=None):
    """[B, Sq, H·hd]: row i of head h of entry b is v[b, pi[b, h, i]] of that head.
    swap = (c0, c1): those two columns of every head exchanged — a deliberately wrong answer for the tests of the comparison."""
    B, Sk, d = v.shape
    H, Sq = d // hd, pi.shape[2]
    out = torch.gather(v.reshape(B, Sk, H, hd).transpose(1, 2), 2, pi[..., None].expand(B, H, Sq, hd)).transpose(1, 2).contiguous()
    if swap is not None:
        out[..., [swap[0], swap[1]]] = out[..., [swap[1], swap[0]]]
    return out.reshape(B, Sq, d)


def is_v(out, buf, hd, B, Sq, H):
    """With one key the output is v, bit for bit."""
    d = H * hd
    return torch.equal(out.view(torch.int16), buf[:, :1, 2 * d:3 * d].expand(B, Sq, d).contiguous().view(torch.int16))
