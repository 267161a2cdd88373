"""rt_attention_fwd_grouped (through ops.attention(groups=)): joint attention whose keys fall into tile-aligned groups and whose query
rows each carry a bit set of the groups they see. The harness of test_attention_edges_gpu.py — guarded q|k|v buffer (NaN behind S and in
the pad columns), sentinel around the output, two launches with the same bits, out of place and in place over q — against an fp64
softmax with -inf on the hidden keys, judged PER ELEMENT with that file's bound
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
p the fp64 MASKED softmax row. A row that sees no key has ref = 0 and p = 0 and must be exactly zero.

What can go wrong that the dense kernel cannot: a running maximum of -inf meeting a hidden tile (exp2(NaN)), a split run that saw nothing
(its record must weigh exactly 0), 1 / l with l = 0, and a tile given to the wrong group."""
import numpy as np
import pytest
import torch

from support_kernels import BF16, check_bound, same_bits, twice
from test_attention_edges_gpu import DH, fused_buffer, guards_intact, make_qkv, new_o, variant

pytestmark = pytest.mark.gpu

# Worst excess of |got - ref| over the first two terms of the bound across every case of this file, measured on an MI355X (run with -s:
# each case prints its own): 0.0 everywhere. With nothing measured to multiply by 4 the slack is 2^-20 max|v| of the case's data.
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


def tile_ends(S):
    """Ends at every multiple of 64 below S, then S."""
    return tuple(range(64, S, 64)) + (S,)


def words(table, device):
    """[B, S] python-int / uint32 table -> int32 device tensor with the same bits (bit 31 included)."""
    return torch.from_numpy(np.asarray(table, dtype=np.uint32).view(np.int32).copy()).to(device)


def visible(ends, vis):
    """bool [B, S, S]: key j visible to row i of entry b. vis: uint32 numpy [B, S]."""
    S = ends[-1]
    gid = np.searchsorted(np.asarray(ends), np.arange(S), side="right")              # group of key j
    return torch.from_numpy(((vis[:, :, None] >> gid[None, None, :].astype(np.uint32)) & 1).astype(bool))


def masked_reference(qkv, Hn, ends, vis):
    """fp64 softmax-attention with -inf on the hidden keys; (ref, sum p|v|, max|v|). Rows that see nothing: ref = 0, p = 0."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    q, k, v = (qkv[..., i * d : (i + 1) * d].double().reshape(Bn, S, Hn, DH) for i in range(3))
    see = visible(ends, vis)
    ref, pv = torch.zeros(Bn, S, Hn, DH, dtype=torch.float64), torch.zeros(Bn, S, Hn, DH, dtype=torch.float64)
    for b in range(Bn):
        sb = see[b if see.shape[0] > 1 else 0]
        some = sb.any(dim=1)
        for h in range(Hn):
            s = (q[b, :, h] @ k[b, :, h].t()) * DH ** -0.5
            s = s.masked_fill(~sb, float("-inf"))
            p = torch.zeros_like(s)
            p[some] = torch.softmax(s[some], dim=-1)
            ref[b, :, h], pv[b, :, h] = p @ v[b, :, h], p @ v[b, :, h].abs()
    return ref.reshape(Bn, S, d), pv.reshape(Bn, S, d), float(v.abs().max())


def check_attention(what, got, ref, pv, vmax):
    got, ref, pv = got.double().cpu(), ref.double(), pv.double()
    base = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * pv
    slack = attn_slack(vmax)
    excess = float(((got - ref).abs() - base).max())
    print(f"[grouped attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    return check_bound(what, got, ref, base + slack)


def run_grouped(ops, qkv, Hn, device, what, ends, vis, ref=None, split=True, check_entries=True):
    """run_guarded of the edges file with groups=: out of place on guarded buffers, twice; bound, guards, inputs untouched; rows that see
    nothing exactly zero; in place over q; every entry alone. vis: uint32 numpy [B or 1, S]. Returns the output."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()
    groups = ops.KeyGroups(ends, words(vis, device))

    def run():
        obuf, o = new_o(Bn, S, d, device)
        ops.attention(q, k, v, o, Hn, split=split, groups=groups)
        torch.cuda.synchronize()
        return obuf

    obuf = twice(run)
    got = obuf[:, :S, :d]
    r, pv, vmax = masked_reference(qkv, Hn, ends, vis) if ref is None else ref
    check_attention(what, got, r, pv, vmax)
    blind = torch.from_numpy(np.broadcast_to(vis, (Bn, S)) == 0)
    if bool(blind.any()):
        assert int((got.cpu()[blind] != 0).sum()) == 0, f"{what}: a row that sees no key is not exactly zero"
    assert guards_intact(obuf, S, d), f"{what}: wrote outside [:S, :H*128] of the output"
    assert same_bits(buf, before), f"{what}: the kernel wrote to its inputs"
    ops.attention(q, k, v, q, Hn, split=split, groups=groups)
    torch.cuda.synchronize()
    assert same_bits(q, got), f"{what}: in place over q differs"
    expect = before.clone()
    expect[:, :S, :d] = got
    assert same_bits(buf, expect), f"{what}: the in-place run touched more than q"
    if check_entries and Bn > 1:
        for b in range(Bn):
            _, q1, k1, v1 = fused_buffer(qkv[b : b + 1], device)
            o1buf, o1 = new_o(1, S, d, device)
            vb = vis[b : b + 1] if vis.shape[0] > 1 else vis
            ops.attention(q1, k1, v1, o1, Hn, split=split, groups=ops.KeyGroups(ends, words(vb, device)))
            torch.cuda.synchronize()
            assert same_bits(o1buf[0], obuf[b]), f"{what}: entry {b} differs from its batch-1 launch"
    return got


def sweep_table(S, n, shift):
    """Row words in which, by 32-row wave block: even blocks mix the five kinds row by row, odd blocks hold one kind throughout (a whole
    block that hides a group, or everything). Kinds: sees all / only the first group / not the first / only the last (ragged) / nothing."""
    full = (1 << n) - 1
    kinds = [full, 1, full & ~1, 1 << (n - 1), 0]
    i = np.arange(S)
    blk = i // 32
    kind = np.where(blk % 2 == 0, (i + shift) % 5, (blk // 2 + 2 + shift) % 5)
    return np.asarray(kinds, dtype=np.uint32)[kind]


SWEEP = [64, 65, 128, 129, 192, 257, 320]


@pytest.mark.parametrize("S,shared", [(S, False) for S in SWEEP] + [(129, True), (320, True)])
def test_grouped_length_and_boundary_sweep(ops, gpu, S, shared):
    Bn, Hn = 2, 2
    ends = tile_ends(S)
    qkv = make_qkv(Bn, S, Hn, 5000 + S)
    vis = np.stack([sweep_table(S, len(ends), 0)] if shared else [sweep_table(S, len(ends), 0), sweep_table(S, len(ends), 3)])
    assert (vis == 0).any() and (vis == (1 << len(ends)) - 1).any()
    run_grouped(ops, qkv, Hn, gpu, f"sweep S={S} {'shared' if shared else 'per-entry'}", ends, vis)


def test_grouped_one_visible_key(ops, gpu):
    """S = 129, ends (64, 128, 129): a row that sees only group 2 sees key 128 alone and returns v[128] bit for bit."""
    Bn, Hn, S = 2, 2, 129
    d = Hn * DH
    ends = (64, 128, 129)
    qkv = make_qkv(Bn, S, Hn, 5200)
    vis = np.full((1, S), 7, dtype=np.uint32)
    only = [0, 31, 33, 70, 127, 128]
    vis[0, only] = 4
    vis[0, 96:128] = 4                                               # a whole wave block
    got = run_grouped(ops, qkv, Hn, gpu, "one visible key", ends, vis)
    v128 = qkv[:, 128, 2 * d :].to(gpu)
    for row in only + list(range(96, 128)):
        assert same_bits(got[:, row], v128), row


@pytest.mark.parametrize("where", ["leading", "last"])
def test_grouped_dominant_hidden_key(ops, gpu, where):
    """A key whose score lies ~45 above the rest, HIDDEN from the row it dominates: in the leading group (key 5) and alone in the ragged
    last tile (key S - 1). The output meets the bound of the reference that excludes it."""
    Bn, Hn, S = 2, 2, 129
    d = Hn * DH
    ends = (64, 128, 129)
    rows = [(0, 0, 5), (0, 1, S - 2), (1, 0, 40), (1, 1, 64)]
    key, bit = (5, 0) if where == "leading" else (S - 1, 2)
    qkv = make_qkv(Bn, S, Hn, 5300 + bit)
    for b, h, row in rows:
        qkv[b, key, d + h * DH : d + (h + 1) * DH] = qkv[b, row, h * DH : (h + 1) * DH]
    vis = np.full((Bn, S), 7, dtype=np.uint32)
    for b, h, row in rows:
        vis[b, row] = 7 & ~(1 << bit)
    run_grouped(ops, qkv, Hn, gpu, f"dominant hidden key, {where}", ends, vis)


@pytest.mark.parametrize("S,Hn,split", [(257, 2, True), (2048, 8, True), (2048, 8, False)])
def test_grouped_all_bits_set_is_the_dense_kernel(ops, gpu, S, Hn, split):
    Bn = 2 if S == 257 else 1
    d = Hn * DH
    ends = tile_ends(S)
    qkv = make_qkv(Bn, S, Hn, 5400 + S)
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o_d = new_o(Bn, S, d, gpu)
    _, o_g = new_o(Bn, S, d, gpu)
    with variant(0):
        ops.attention(q, k, v, o_d, Hn, split=split)
    vis = np.full((1, S), (1 << len(ends)) - 1, dtype=np.uint32)
    ops.attention(q, k, v, o_g, Hn, split=split, groups=ops.KeyGroups(ends, words(vis, gpu)))
    torch.cuda.synchronize()
    assert same_bits(o_g, o_d)


def test_grouped_key_split(ops, gpu):
    """S = 2048, H = 8 (the smallest shape that splits on a 256-CU part), ends (512, 1024, 1536, 2048): whole split runs lie inside one
    group, so runs that see nothing occur for the rows that see only group 2, only {0, 3}, or nothing."""
    from reptext_amd import native

    S, Hn = 2048, 8
    d = Hn * DH
    assert native.load().rt_attention_ws_bytes(1, S, Hn) > 0
    ends = (512, 1024, 1536, 2048)
    qkv = make_qkv(1, S, Hn, 5500)
    for h, row, key in ((0, 10, 1500), (7, 2000, S - 3), (5, 1990, 70)):
        qkv[0, key, d + h * DH : d + (h + 1) * DH] = qkv[0, row, h * DH : (h + 1) * DH]
    i = np.arange(S)
    blk = i // 32
    kinds = np.asarray([4, 9, 0, 15], dtype=np.uint32)               # only group 2 / only {0, 3} / nothing / all
    vis = kinds[np.where(blk % 2 == 0, i % 4, (blk // 2) % 4)][None]
    ref = masked_reference(qkv, Hn, ends, vis)
    got = run_grouped(ops, qkv, Hn, gpu, "grouped key split", ends, vis, ref=ref)
    unsplit = run_grouped(ops, qkv, Hn, gpu, "grouped key split, split=False", ends, vis, ref=ref, split=False)
    assert unsplit.shape == got.shape
    groups = ops.KeyGroups(ends, words(vis, gpu))
    _, q, k, v = fused_buffer(qkv, gpu)
    for _ in range(4):
        _, o = new_o(1, S, d, gpu)
        ops.attention(q, k, v, o, Hn, groups=groups)
        assert same_bits(o, got)
    qkv3 = torch.cat([qkv, qkv.flip(1), qkv], dim=0)
    _, q3, k3, v3 = fused_buffer(qkv3, gpu)
    o3buf, o3 = new_o(3, S, d, gpu)
    ops.attention(q3, k3, v3, o3, Hn, groups=groups)                 # one table for the batch
    torch.cuda.synchronize()
    assert same_bits(o3[0], got[0]) and same_bits(o3[2], got[0])
    assert guards_intact(o3buf, S, d)
    for Bn in (1, 3):
        ws = ops._attention_workspace(Bn, S, Hn, gpu)
        n = Bn * Hn * ((S + 127) // 128)
        assert ws is not None and int(ws[: 4 * n].view(torch.int32).abs().max()) == 0


def test_grouped_argument_checks(ops, gpu):
    Bn, Hn, S = 1, 2, 129
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 5600)
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o = new_o(Bn, S, d, gpu)
    vis = words(np.full((1, S), 1, dtype=np.uint32), gpu)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.attention(q, k, v, o, Hn, groups=ops.KeyGroups((60, 129), vis))
    with pytest.raises(ValueError, match="last end"):
        ops.attention(q, k, v, o, Hn, groups=ops.KeyGroups((64, 128), vis))
    S33 = 64 * 33
    qkv = make_qkv(1, S33, 1, 5601)
    _, q2, k2, v2 = fused_buffer(qkv, gpu)
    _, o2 = new_o(1, S33, DH, gpu)
    with pytest.raises(ValueError, match="1..32"):
        ops.attention(q2, k2, v2, o2, 1, groups=ops.KeyGroups(tile_ends(S33), words(np.ones((1, S33), dtype=np.uint32), gpu)))
    with pytest.raises(ValueError, match="rows="):
        ops.attention(q, k, v, o, Hn, rows=(0, 64), groups=ops.KeyGroups((64, 128, 129), vis))
    # the C entry refuses them too (a caller that bypasses ops)
    from reptext_amd import native
    import ctypes as C

    def raw(ends, n=None, scale=DH ** -0.5):
        arr = (C.c_int32 * len(ends))(*ends)
        return native.load().rt_attention_fwd_grouped(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(1), q.stride(0), o.stride(1),
                                                      o.stride(0), Bn, S, Hn, scale, C.cast(arr, C.c_void_p), len(ends) if n is None else n,
                                                      vis.data_ptr(), 0, None, 0, torch.cuda.current_stream().cuda_stream)

    assert raw((60, 129)) == native.RT_E_BADARG
    assert raw((64, 128)) == native.RT_E_BADARG
    assert raw((64, 128, 129), n=33) == native.RT_E_BADARG
    assert raw((64, 128, 129), scale=0.0) == native.RT_E_BADARG
    assert raw((64, 128, 129)) == 0
    torch.cuda.synchronize()
