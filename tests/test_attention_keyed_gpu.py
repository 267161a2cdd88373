"""rt_attention_fwd_keyed (through ops.attention(groups=ops.KeyClasses)): joint attention in which every KEY carries a class id byte and
row i sees key j iff bit class[j] of the row's word is set. The harness of test_attention_groups_gpu.py / test_attention_edges_gpu.py —
guarded q|k|v buffer, sentinel around the output, two launches with the same bits, in place over q, every entry alone — against an fp64
softmax with -inf on the hidden keys, judged PER ELEMENT with those files' bound
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
A row that sees no key must be exactly zero.

What can go wrong that the grouped kernel cannot: a score register tested against another key's class (the (r, hh, h) -> key map), a
class read behind S, a tile of several classes taking the one-class path or the reverse.

The key index map: four class tables over S = 128 cannot make every key the single visible key of some row whose word has one bit —
the keys tested by one table need distinct classes and every other key a class that none of those rows sees, so a table tests at most 31
keys and four tables 124. Eight tables of 16 keys are used (classes 0..15 for the keys under test, 16..31 for the others), after one
launch with class j % 32 in which row i sees class i % 32 (four keys), which is kept
and judged against the reference."""
import numpy as np
import pytest
import torch

from support_kernels import BF16, check_bound, same_bits, twice
from test_attention_edges_gpu import DH, fused_buffer, guards_intact, make_qkv, new_o, variant
from test_attention_groups_gpu import SWEEP, sweep_table, tile_ends, words

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


def visible(vis, cls):
    """bool [B or 1, S, S]: key j visible to row i. vis: uint32 numpy [B or 1, S]; cls: uint8 numpy [B or 1, S]."""
    n = max(vis.shape[0], cls.shape[0])
    vis, cls = np.broadcast_to(vis, (n, vis.shape[1])), np.broadcast_to(cls, (n, cls.shape[1]))
    return torch.from_numpy(((vis[:, :, None] >> cls[:, None, :].astype(np.uint32)) & 1).astype(bool))


def masked_reference(qkv, Hn, vis, cls):
    """fp64 softmax-attention with -inf on the hidden keys; (ref, sum p|v|, max|v|). Rows that see nothing: ref = 0, p = 0."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    q, k, v = (qkv[..., i * d : (i + 1) * d].double().reshape(Bn, S, Hn, DH) for i in range(3))
    see = visible(vis, cls)
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
    print(f"[keyed attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    return check_bound(what, got, ref, base + slack)


def classes(ops, vis, cls, device, cls_dev=None):
    """The record of a launch: checked on the host tables, then moved. cls_dev: a device view to use for the class table instead."""
    kc = ops.KeyClasses(words(vis, "cpu"), torch.from_numpy(np.ascontiguousarray(cls))).to(device)
    return kc if cls_dev is None else ops.KeyClasses(kc.row_vis, cls_dev)


def run_keyed(ops, qkv, Hn, device, what, vis, cls, ref=None, split=True, check_entries=True, cls_dev=None):
    """run_grouped of the groups file with a KeyClasses: out of place on guarded buffers, twice; bound, guards, inputs untouched; rows that
    see nothing exactly zero; in place over q; every entry alone. vis uint32 / cls uint8 numpy [B or 1, S]. Returns the output."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()
    groups = classes(ops, vis, cls, device, cls_dev)

    def run():
        obuf, o = new_o(Bn, S, d, device)
        ops.attention(q, k, v, o, Hn, split=split, groups=groups)
        torch.cuda.synchronize()
        return obuf

    obuf = twice(run)
    got = obuf[:, :S, :d]
    r, pv, vmax = masked_reference(qkv, Hn, vis, cls) if ref is None else ref
    check_attention(what, got, r, pv, vmax)
    blind = ~visible(vis, cls).any(dim=2)
    blind = blind.expand(Bn, S)
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
            vb, cb = (vis[b : b + 1] if vis.shape[0] > 1 else vis), (cls[b : b + 1] if cls.shape[0] > 1 else cls)
            ops.attention(q1, k1, v1, o1, Hn, split=split, groups=classes(ops, vb, cb, device))
            torch.cuda.synchronize()
            assert same_bits(o1buf[0], obuf[b]), f"{what}: entry {b} differs from its batch-1 launch"
    return got


def test_keyed_key_index_map(ops, gpu):
    """Every one of the 128 keys is the single visible key of rows in every wave and both lane halves, which then return its value row
    bit for bit: only a right (register, lane half, half tile) -> key map passes."""
    Bn, Hn, S = 1, 2, 128
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 6000)
    j = np.arange(S)
    run_keyed(ops, qkv, Hn, gpu, "class j % 32, row i sees class i % 32", (np.uint32(1) << (j % 32).astype(np.uint32))[None], (j % 32).astype(np.uint8)[None])
    vis = (np.uint32(1) << (j % 16).astype(np.uint32))[None]
    for t in range(8):
        cls = np.where(j // 16 == t, j % 16, 16 + j % 16).astype(np.uint8)[None]
        got = run_keyed(ops, qkv, Hn, gpu, f"one visible key, table {t}", vis, cls)
        expect = qkv[:, 16 * t + j % 16, 2 * d :].to(gpu)                # row i sees key 16 t + i % 16 alone
        assert same_bits(got, expect), t


@pytest.mark.parametrize("S,shared", [(S, False) for S in SWEEP] + [(129, True), (320, True)])
def test_keyed_length_and_boundary_sweep(ops, gpu, S, shared):
    Bn, Hn = 2, 2
    qkv = make_qkv(Bn, S, Hn, 6100 + S)
    j = np.arange(S)
    cls = np.stack([(7 * j + b) % 5 for b in range(1 if shared else Bn)]).astype(np.uint8)
    vis = np.stack([sweep_table(S, 5, 0)] if shared else [sweep_table(S, 5, 0), sweep_table(S, 5, 3)])
    assert (vis == 0).any() and (vis == 31).any()
    run_keyed(ops, qkv, Hn, gpu, f"sweep S={S} {'shared' if shared else 'per-entry'}", vis, cls)


@pytest.mark.parametrize("S", [65, 129])
def test_keyed_class_bytes_behind_S_are_not_read_as_keys(ops, gpu, S):
    """The class table is a view (odd base offset, batch stride S + 67) of a buffer whose other bytes name class 0, which every row
    sees and no key has: the rows that see class 0 alone stay exactly zero, everything else meets the reference."""
    Bn, Hn = 2, 2
    qkv = make_qkv(Bn, S, Hn, 6200 + S)
    j = np.arange(S)
    cls = np.stack([1 + (3 * j + b) % 4 for b in range(Bn)]).astype(np.uint8)
    kinds = np.asarray([31, 1, 1 | 2, 1 | 16, 1 | 4 | 8], dtype=np.uint32)
    vis = np.stack([kinds[(j + 2 * b) % 5] for b in range(Bn)])
    big = torch.zeros(Bn, S + 67, dtype=torch.uint8)
    big[:, 3 : 3 + S] = torch.from_numpy(cls)
    view = big.to(gpu)[:, 3 : 3 + S]
    assert view.data_ptr() % 2 == 1 and view.stride() == (S + 67, 1)
    run_keyed(ops, qkv, Hn, gpu, f"class bytes behind S={S}", vis, cls, cls_dev=view, check_entries=False)


def group_classes(ends):
    S = ends[-1]
    return np.searchsorted(np.asarray(ends), np.arange(S), side="right").astype(np.uint8)[None]


@pytest.mark.parametrize("S", [129, 257, 320])
def test_keyed_with_a_class_per_group_is_the_grouped_kernel(ops, gpu, S):
    Bn, Hn = 2, 2
    d = Hn * DH
    ends = tile_ends(S)
    qkv = make_qkv(Bn, S, Hn, 5000 + S)
    vis = np.stack([sweep_table(S, len(ends), 0), sweep_table(S, len(ends), 3)])
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o_g = new_o(Bn, S, d, gpu)
    _, o_k = new_o(Bn, S, d, gpu)
    ops.attention(q, k, v, o_g, Hn, groups=ops.KeyGroups(ends, words(vis, gpu)))
    ops.attention(q, k, v, o_k, Hn, groups=classes(ops, vis, group_classes(ends), gpu))
    torch.cuda.synchronize()
    assert same_bits(o_k, o_g)


@pytest.mark.parametrize("split", [True, False])
def test_keyed_equals_grouped_and_dense_at_a_split_shape(ops, gpu, split):
    S, Hn = 2048, 8
    d = Hn * DH
    ends = (512, 1024, 1536, 2048)
    qkv = make_qkv(1, S, Hn, 5500)
    i = np.arange(S)
    blk = i // 32
    kinds = np.asarray([4, 9, 0, 15], dtype=np.uint32)
    vis = kinds[np.where(blk % 2 == 0, i % 4, (blk // 2) % 4)][None]
    _, q, k, v = fused_buffer(qkv, gpu)
    outs = [new_o(1, S, d, gpu)[1] for _ in range(4)]
    ops.attention(q, k, v, outs[0], Hn, split=split, groups=ops.KeyGroups(ends, words(vis, gpu)))
    ops.attention(q, k, v, outs[1], Hn, split=split, groups=classes(ops, vis, group_classes(ends), gpu))
    with variant(0):
        ops.attention(q, k, v, outs[2], Hn, split=split)
    full = np.full((1, S), 0xFFFFFFFF, dtype=np.uint32)
    ops.attention(q, k, v, outs[3], Hn, split=split, groups=classes(ops, full, (i % 32).astype(np.uint8)[None], gpu))
    torch.cuda.synchronize()
    assert same_bits(outs[1], outs[0]), "a class per group differs from the grouped launch"
    assert same_bits(outs[3], outs[2]), "all bits set differs from the dense launch"


@pytest.mark.parametrize("where", ["mid-tile", "ragged"])
def test_keyed_dominant_hidden_key(ops, gpu, where):
    """A key whose score lies ~45 above the rest, HIDDEN from the rows it dominates while its neighbours j - 1 and j + 1 are visible:
    mid-tile (j = 37) and alone in the ragged last tile (j = S - 1)."""
    Bn, Hn, S = 2, 2, 129
    d = Hn * DH
    rows = [(0, 0, 5), (0, 1, S - 2), (1, 0, 40), (1, 1, 64)]
    key = 37 if where == "mid-tile" else S - 1
    qkv = make_qkv(Bn, S, Hn, 6300 + key)
    for b, h, row in rows:
        qkv[b, key, d + h * DH : d + (h + 1) * DH] = qkv[b, row, h * DH : (h + 1) * DH]
    cls = np.zeros((1, S), dtype=np.uint8)
    cls[0, key] = 1
    vis = np.full((Bn, S), 3, dtype=np.uint32)
    for b, h, row in rows:
        vis[b, row] = 1
    run_keyed(ops, qkv, Hn, gpu, f"dominant hidden key, {where}", vis, cls)


def test_keyed_key_split(ops, gpu):
    """S = 2048, H = 8 (the smallest shape that splits on a 256-CU part). The classes alternate key by key: {0, 1} below key 1024, {2, 3}
    from it on, so every tile is mixed and whole split runs hold two classes only; rows that see class 2 alone, {0, 3} or nothing meet
    runs in which they see nothing."""
    from reptext_amd import native

    S, Hn = 2048, 8
    d = Hn * DH
    assert native.load().rt_attention_ws_bytes(1, S, Hn) > 0
    qkv = make_qkv(1, S, Hn, 6400)
    for h, row, key in ((0, 10, 1500), (7, 2000, S - 3), (5, 1990, 70)):
        qkv[0, key, d + h * DH : d + (h + 1) * DH] = qkv[0, row, h * DH : (h + 1) * DH]
    i = np.arange(S)
    cls = (2 * (i >= 1024) + i % 2).astype(np.uint8)[None]
    blk = i // 32
    kinds = np.asarray([4, 9, 0, 15], dtype=np.uint32)               # only class 2 / only {0, 3} / nothing / all
    vis = kinds[np.where(blk % 2 == 0, i % 4, (blk // 2) % 4)][None]
    ref = masked_reference(qkv, Hn, vis, cls)
    got = run_keyed(ops, qkv, Hn, gpu, "keyed key split", vis, cls, ref=ref)
    unsplit = run_keyed(ops, qkv, Hn, gpu, "keyed key split, split=False", vis, cls, ref=ref, split=False)
    assert unsplit.shape == got.shape
    groups = classes(ops, vis, cls, gpu)
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


def test_keyed_argument_checks(ops, gpu):
    from reptext_amd import native

    Bn, Hn, S = 1, 2, 129
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 6500)
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o = new_o(Bn, S, d, gpu)
    vis_h, cls_h = torch.ones(1, S, dtype=torch.int32), torch.zeros(1, S, dtype=torch.uint8)
    good = ops.KeyClasses(vis_h, cls_h).to(gpu)
    bad = cls_h.clone()
    bad[0, 100] = 32
    with pytest.raises(ValueError, match="below 32"):
        ops.KeyClasses(vis_h, bad)
    with pytest.raises(ValueError, match="rows="):
        ops.attention(q, k, v, o, Hn, rows=(0, 64), groups=good)
    with pytest.raises(ValueError, match="scale > 0"):
        ops.attention(q, k, v, o, Hn, scale=0.0, groups=good)
    with pytest.raises(ValueError, match=r"need \[1 or 1, 129\]"):
        ops.attention(q, k, v, o, Hn, groups=ops.KeyClasses(vis_h[:, :128].contiguous(), cls_h[:, :128].contiguous()).to(gpu))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention(q, k, v, o, Hn, groups=ops.KeyClasses(vis_h, cls_h))
    # the C entry refuses them too (a caller that bypasses ops)
    pad = torch.zeros(S + 2, dtype=torch.int32, device=gpu)

    def raw(vis=good.row_vis.data_ptr(), cls=good.key_class.data_ptr(), scale=DH ** -0.5, svb=0, scb=0):
        return native.load().rt_attention_fwd_keyed(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(1), q.stride(0), o.stride(1),
                                                    o.stride(0), Bn, S, Hn, scale, vis, svb, cls, scb, None, 0,
                                                    torch.cuda.current_stream().cuda_stream)

    assert raw(vis=None) == native.RT_E_BADARG and raw(cls=None) == native.RT_E_BADARG
    assert raw(scale=0.0) == native.RT_E_BADARG and raw(svb=-1) == native.RT_E_BADARG and raw(scb=-1) == native.RT_E_BADARG
    assert raw(vis=pad.data_ptr() + 2) == native.RT_E_ALIGN                # row_vis is read a word at a time; the byte table asks nothing
    assert raw() == 0
    torch.cuda.synchronize()
