"""rt_attention_fwd_grouped_biased / rt_attention_fwd_keyed_biased (through ops.attention(groups=, key_bias=)): the grouped and the keyed
joint attention with an additive fp32 bias per key CLASS on the logits — the group index of a key under the grouped rule, its class byte
under the keyed one. The harness of test_attention_groups_gpu.py / test_attention_keyed_gpu.py, whose pieces are imported — guarded q|k|v
buffer, sentinels around the output, two launches with the same bits, in place over q, every batch entry alone — against an fp64 softmax
with -inf on the hidden keys and the bias added to the logits, judged PER ELEMENT with those files' bound
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
p the fp64 masked, biased softmax row. A row that sees no key must be exactly zero, whatever the biases.

What can go wrong that the unbiased launches cannot: a bias added after the half's maximum was taken (the rescale decision then misses
it: +8 nats is more than RESCALE_THR), a bias in the wrong units (the kernel holds raw scores and log2 units), the bias of another
group (read when the group advances, or not), of another key's class (the score register -> key map of a tile of several classes), a
hidden key brought back by its bias, a table row of another batch entry, a split record whose maximum lacks the bias."""
import ctypes as C

import numpy as np
import pytest
import torch

from support_kernels import check_bound, same_bits, twice
from test_attention_edges_gpu import DH, fused_buffer, guards_intact, make_qkv, new_o
from test_attention_groups_gpu import SWEEP, sweep_table, tile_ends, words
from test_attention_keyed_gpu import classes, group_classes, visible

pytestmark = pytest.mark.gpu

# Worst excess of |got - ref| over the first two terms of the bound across every case of this file (run with -s: each case prints its
# own). NOT YET MEASURED on an MI355X: the siblings' files measured 0.0 everywhere, and until this file's cases have printed theirs the
# value stays 0.0, under which the slack is the siblings' 2^-20 max|v| of the case's data — the narrowest the rule allows.
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


class Grouped:
    """Keys in tile-aligned groups: the class of key j is its group index."""
    def __init__(self, ends):
        self.ends, self.cls = tuple(ends), group_classes(ends)

    def record(self, ops, vis, device, entry=None):
        return ops.KeyGroups(self.ends, words(vis, device))

    def entry(self, b):
        return self


class Keyed:
    """A class byte per key: uint8 numpy [B or 1, S]."""
    def __init__(self, cls):
        self.cls = np.ascontiguousarray(cls, dtype=np.uint8)

    def record(self, ops, vis, device):
        return classes(ops, vis, self.cls, device)

    def entry(self, b):
        return Keyed(self.cls[b : b + 1]) if self.cls.shape[0] > 1 else self


def table(entries, rows=1):
    """{class: bias} (one dict, or one per batch entry) -> float32 numpy [rows, 32]."""
    dicts = entries if isinstance(entries, (list, tuple)) else [entries] * rows
    t = np.zeros((len(dicts), 32), dtype=np.float32)
    for b, d in enumerate(dicts):
        for c, x in d.items():
            t[b, c] = x
    return t


def biased_reference(qkv, Hn, vis, cls, bias):
    """fp64 softmax-attention with -inf on the hidden keys and bias[b, class of key j] added to the logits; (ref, sum p|v|, max|v|).
    Rows that see nothing: ref = 0, p = 0. vis uint32 / cls uint8 numpy [B or 1, S]; bias float32 numpy [B or 1, 32]."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    q, k, v = (qkv[..., i * d : (i + 1) * d].double().reshape(Bn, S, Hn, DH) for i in range(3))
    see = visible(vis, cls)
    ref, pv = torch.zeros(Bn, S, Hn, DH, dtype=torch.float64), torch.zeros(Bn, S, Hn, DH, dtype=torch.float64)
    for b in range(Bn):
        sb = see[b if see.shape[0] > 1 else 0]
        kb = torch.from_numpy(bias[b if bias.shape[0] > 1 else 0].astype(np.float64)[cls[b if cls.shape[0] > 1 else 0].astype(np.int64)])
        some = sb.any(dim=1)
        for h in range(Hn):
            s = (q[b, :, h] @ k[b, :, h].t()) * DH ** -0.5 + kb[None, :]
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
    print(f"[biased attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    return check_bound(what, got, ref, base + slack)


def run_biased(ops, qkv, Hn, device, what, vis, mode, bias, ref=None, split=True, check_entries=True):
    """run_grouped / run_keyed of the sibling files with key_bias=: out of place on guarded buffers, twice; bound, guards, inputs
    untouched; rows that see nothing exactly zero; in place over q; every entry alone, with its own row of a [B, 32] table. vis: uint32
    numpy [B or 1, S]; mode: a Grouped or a Keyed; bias: float32 numpy [B or 1, 32]. Returns the output."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()
    groups = mode.record(ops, vis, device)
    kb = torch.from_numpy(bias).to(device)

    def run():
        obuf, o = new_o(Bn, S, d, device)
        ops.attention(q, k, v, o, Hn, split=split, groups=groups, key_bias=kb)
        torch.cuda.synchronize()
        return obuf

    obuf = twice(run)
    got = obuf[:, :S, :d]
    r, pv, vmax = biased_reference(qkv, Hn, vis, mode.cls, bias) if ref is None else ref
    check_attention(what, got, r, pv, vmax)
    blind = (~visible(vis, mode.cls).any(dim=2)).expand(Bn, S)
    if bool(blind.any()):
        assert int((got.cpu()[blind] != 0).sum()) == 0, f"{what}: a row that sees no key is not exactly zero"
    assert guards_intact(obuf, S, d), f"{what}: wrote outside [:S, :H*128] of the output"
    assert same_bits(buf, before), f"{what}: the kernel wrote to its inputs"
    ops.attention(q, k, v, q, Hn, split=split, groups=groups, key_bias=kb)
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
            kb1 = kb[b : b + 1] if kb.shape[0] > 1 else kb
            ops.attention(q1, k1, v1, o1, Hn, split=split, groups=mode.entry(b).record(ops, vb, device), key_bias=kb1)
            torch.cuda.synchronize()
            assert same_bits(o1buf[0], obuf[b]), f"{what}: entry {b} differs from its batch-1 launch"
    return got


def unbiased(ops, qkv, Hn, device, vis, mode, split=True):
    Bn, S, _ = qkv.shape
    _, q, k, v = fused_buffer(qkv, device)
    _, o = new_o(Bn, S, Hn * DH, device)
    ops.attention(q, k, v, o, Hn, split=split, groups=mode.record(ops, vis, device))
    torch.cuda.synchronize()
    return o


def spread(n, shift=0):
    """{class: bias} for classes 0..n-1: distinct values over +-4, none of them 0, in an order that is not monotonic in the class."""
    m = n + n % 2                                                    # an even count of points, symmetric about 0: no 0 among them
    x = np.linspace(-4.0, 4.0, m)[np.random.default_rng(m).permutation(m)]
    return {c: float(x[(c + shift) % m]) for c in range(n)}


def mixed_and_whole_tiles(S, Bn):
    """Class bytes in which the even 64-key tiles hold one class (the tile index mod 5) and the odd ones five, key by key."""
    j = np.arange(S)
    return np.stack([np.where((j // 64) % 2 == 0, (j // 64) % 5, (7 * j + b) % 5) for b in range(Bn)]).astype(np.uint8)


# ---- grouped

@pytest.mark.parametrize("S,per_entry", [(S, S % 2 == 0) for S in SWEEP])
def test_grouped_biased_length_sweep(ops, gpu, S, per_entry):
    """The siblings' length sweep (ragged last tiles, a group that ends at S, rows of every kind) with a bias of its own on every
    group; the even lengths with a [B, 32] table whose rows differ, the odd ones with [1, 32]."""
    Bn, Hn = 2, 2
    ends = tile_ends(S)
    n = len(ends)
    qkv = make_qkv(Bn, S, Hn, 7000 + S)
    vis = np.stack([sweep_table(S, n, 0), sweep_table(S, n, 3)])
    bias = table([spread(n), spread(n, 1)] if per_entry else spread(n))
    assert len(set(bias[0, :n])) == n and (bias[:, :n] != 0).all() and (vis == 0).any()
    run_biased(ops, qkv, Hn, gpu, f"grouped sweep S={S} table {bias.shape[0]}x32", vis, Grouped(ends), bias)


@pytest.mark.parametrize("x", [8.0, -8.0])
def test_grouped_one_group_far_above_or_below(ops, gpu, x):
    """+8 nats (11.5 in log2 units, above RESCALE_THR = 6) on group 3 of 5, late in the key order: its keys dominate every row that sees
    them and the running maximum has to jump when their tile arrives — a bias added after the half's maximum would leave numerators of
    2^11 against a stale maximum, outside the bound at once. -8: the group all but vanishes."""
    Bn, Hn, S = 2, 2, 320
    ends = tile_ends(S)
    qkv = make_qkv(Bn, S, Hn, 7100 + int(x))
    vis = np.stack([sweep_table(S, 5, 0), sweep_table(S, 5, 3)])
    run_biased(ops, qkv, Hn, gpu, f"grouped, {x:+} on group 3", vis, Grouped(ends), table({3: x}))


# ---- keyed

@pytest.mark.parametrize("S,per_entry", [(S, S % 2 == 0) for S in SWEEP])
def test_keyed_biased_tiles_of_one_and_of_several_classes(ops, gpu, S, per_entry):
    """Even tiles hold one class (the scalar path), odd tiles five (every score takes its own key's bias); S = 65, 129, 257: the class
    table is read in a ragged tile, clamped to S - 1."""
    Bn, Hn = 2, 2
    qkv = make_qkv(Bn, S, Hn, 7200 + S)
    cls = mixed_and_whole_tiles(S, Bn if per_entry else 1)
    vis = np.stack([sweep_table(S, 5, 0), sweep_table(S, 5, 3)])
    bias = table([spread(5), spread(5, 2)] if per_entry else spread(5))
    run_biased(ops, qkv, Hn, gpu, f"keyed sweep S={S} table {bias.shape[0]}x32", vis, Keyed(cls), bias)


@pytest.mark.parametrize("t", range(8))
def test_keyed_biased_key_index_map(ops, gpu, t):
    """Every key index receives its own class's bias and no other key's. The design of the keyed file's key-index test: S = 128, eight
    tables (t) of 16 keys under test — keys 16t .. 16t + 15 carry the classes 0..15, one key each, every other key a class of 16..31.
    A launch has two batch entries, each with its own row of a [2, 32] table: +8 on ONE class c < 16, 0 everywhere else, every row sees
    everything. Key 16t + c is then the only biased key of that entry and (scores are N(0, 2^2), so e^8 against 127 weights of order 1)
    carries most of every row's softmax. Eight launches of two entries give c = 0..15; the eight tables give every key of 0..127 its
    turn, which covers both tiles, both halves of a tile, every score register r = 0..15 and both lane halves hh of the map
    key = 64 tile + 32 h + (r & 3) + 8 (r >> 2) + 4 hh. A bias handed to another score register lands on a key whose class has bias 0 in
    the reference: that row's output is then the wrong value row, off by the order of |v| against a bound of 2^-8 of it."""
    Bn, Hn, S = 2, 2, 128
    qkv = make_qkv(Bn, S, Hn, 7300)
    j = np.arange(S)
    cls = np.where(j // 16 == t, j % 16, 16 + j % 16).astype(np.uint8)[None]
    vis = np.full((1, S), 0xFFFFFFFF, dtype=np.uint32)
    for pair in range(8):
        bias = table([{2 * pair: 8.0}, {2 * pair + 1: 8.0}])
        ref = biased_reference(qkv, Hn, vis, cls, bias)
        run_biased(ops, qkv, Hn, gpu, f"key map, table {t}, keys {16 * t + 2 * pair} and {16 * t + 2 * pair + 1}", vis, Keyed(cls), bias, ref=ref)


def test_keyed_biased_class_table_behind_S(ops, gpu):
    """S = 129: the ragged tile's class loads are clamped; the class table is a view with an odd base and a padded batch stride whose
    other bytes name class 0, which no key has and whose bias is +8: it must reach no score."""
    Bn, Hn, S = 2, 2, 129
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 7400)
    j = np.arange(S)
    cls = np.stack([1 + (3 * j + b) % 4 for b in range(Bn)]).astype(np.uint8)
    kinds = np.asarray([31, 1, 1 | 2, 1 | 16, 1 | 4 | 8], dtype=np.uint32)
    vis = np.stack([kinds[(j + 2 * b) % 5] for b in range(Bn)])
    bias = table({0: 8.0, 1: -2.0, 2: 1.5, 3: 3.0, 4: -3.5})
    big = torch.zeros(Bn, S + 67, dtype=torch.uint8)
    big[:, 3 : 3 + S] = torch.from_numpy(cls)
    view = big.to(gpu)[:, 3 : 3 + S]
    assert view.data_ptr() % 2 == 1 and view.stride() == (S + 67, 1)
    _, q, k, v = fused_buffer(qkv, gpu)
    kc = classes(ops, vis, cls, gpu)
    obuf, o = new_o(Bn, S, d, gpu)
    ops.attention(q, k, v, o, Hn, groups=ops.KeyClasses(kc.row_vis, view), key_bias=torch.from_numpy(bias).to(gpu))
    torch.cuda.synchronize()
    ref, pv, vmax = biased_reference(qkv, Hn, vis, cls, bias)
    check_attention("class bytes behind S=129", o, ref, pv, vmax)
    assert guards_intact(obuf, S, d)
    blind = ~visible(vis, cls).any(dim=2)
    assert bool(blind.any()) and int((o.cpu()[blind] != 0).sum()) == 0


# ---- both launches

def modes_at(S, Bn):
    return [("grouped", Grouped(tile_ends(S))), ("keyed", Keyed(mixed_and_whole_tiles(S, Bn)))]


@pytest.mark.parametrize("kind", ["grouped", "keyed"])
def test_a_table_of_zeros_gives_the_bits_of_the_unbiased_launch(ops, gpu, kind):
    Bn, Hn, S = 2, 2, 257
    mode = dict(modes_at(S, Bn))[kind]
    qkv = make_qkv(Bn, S, Hn, 7500)
    vis = np.stack([sweep_table(S, 5, 0), sweep_table(S, 5, 3)])
    _, q, k, v = fused_buffer(qkv, gpu)
    for rows in (1, Bn):
        _, o = new_o(Bn, S, Hn * DH, gpu)
        ops.attention(q, k, v, o, Hn, groups=mode.record(ops, vis, gpu), key_bias=torch.zeros(rows, 32, device=gpu))
        torch.cuda.synchronize()
        assert same_bits(o, unbiased(ops, qkv, Hn, gpu, vis, mode)), rows


@pytest.mark.parametrize("kind", ["grouped", "keyed"])
def test_the_same_constant_on_every_class_leaves_the_softmax_alone(ops, gpu, kind):
    """Softmax invariance: the UNBIASED fp64 reference, within the bound."""
    Bn, Hn, S = 2, 2, 257
    mode = dict(modes_at(S, Bn))[kind]
    qkv = make_qkv(Bn, S, Hn, 7600)
    vis = np.stack([sweep_table(S, 5, 0), sweep_table(S, 5, 3)])
    ref = biased_reference(qkv, Hn, vis, mode.cls, table({}))
    for x in (3.0, -5.0):
        run_biased(ops, qkv, Hn, gpu, f"{kind}, {x:+} on every class", vis, mode, table({c: x for c in range(5)}), ref=ref)


@pytest.mark.parametrize("kind", ["grouped", "keyed"])
def test_a_hidden_key_with_a_bias_stays_hidden(ops, gpu, kind):
    """+8 on class 1, which only the rows of two kinds in five see. Were a hidden key of class 1 let in by its bias, it would carry most
    of the row against a reference that excludes it. Rows whose word is 0 are exactly zero (run_biased asserts it)."""
    Bn, Hn, S = 2, 2, 257
    mode = dict(modes_at(S, Bn))[kind]
    qkv = make_qkv(Bn, S, Hn, 7700)
    i = np.arange(S)
    kinds = np.asarray([31, 31 & ~2, 1, 0, 2], dtype=np.uint32)               # all / not class 1 / only class 0 / nothing / only class 1
    vis = np.stack([kinds[(i + b) % 5] for b in range(Bn)])
    run_biased(ops, qkv, Hn, gpu, f"{kind}, +8 on a class hidden from most rows", vis, mode, table({1: 8.0}))


@pytest.mark.parametrize("kind", ["grouped", "keyed"])
@pytest.mark.parametrize("split", [True, False])
def test_biased_key_split(ops, gpu, kind, split):
    """S = 2048, H = 8, the shape of the siblings' key-split tests (the smallest that splits on a 256-CU part). Grouped: ends (512, 1024,
    1536, 2048) with +5 on group 2 and -3 on group 0; keyed: classes {0, 1} key by key below key 1024 and {2, 3} from it on (every
    tile has two classes) with +5 on class 2 and -3 on class 1. The biased keys 1024.. lie in the middle of every item's 32 key tiles,
    so in partial runs of the split items: their records' maxima include the bias and the combine weighs them by it."""
    from reptext_amd import native

    S, Hn = 2048, 8
    d = Hn * DH
    assert native.load().rt_attention_ws_bytes(1, S, Hn) > 0
    qkv = make_qkv(1, S, Hn, 7800)
    i = np.arange(S)
    blk = i // 32
    kinds = np.asarray([4, 9, 0, 15], dtype=np.uint32)               # only class 2 / only {0, 3} / nothing / all
    vis = kinds[np.where(blk % 2 == 0, i % 4, (blk // 2) % 4)][None]
    if kind == "grouped":
        mode, bias = Grouped((512, 1024, 1536, 2048)), table({2: 5.0, 0: -3.0})
    else:
        mode, bias = Keyed((2 * (i >= 1024) + i % 2)[None]), table({2: 5.0, 1: -3.0})
    got = run_biased(ops, qkv, Hn, gpu, f"{kind} key split, split={split}", vis, mode, bias, split=split)
    if split:
        ws = ops._attention_workspace(1, S, Hn, gpu)
        n = Hn * ((S + 127) // 128)
        assert ws is not None and int(ws[: 4 * n].view(torch.int32).abs().max()) == 0
    assert got.shape == (1, S, d)


def test_biased_argument_checks(ops, gpu):
    from reptext_amd import native

    Bn, Hn, S = 2, 2, 129
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 7900)
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o = new_o(Bn, S, d, gpu)
    vis = np.full((1, S), 7, dtype=np.uint32)
    ends = (64, 128, 129)
    grouped = ops.KeyGroups(ends, words(vis, gpu))
    keyed = classes(ops, vis, group_classes(ends), gpu)
    kb = torch.zeros(1, 32, device=gpu)
    for groups in (grouped, keyed):
        with pytest.raises(TypeError, match="float32"):
            ops.attention(q, k, v, o, Hn, groups=groups, key_bias=kb.double())
        with pytest.raises(ValueError, match=r"need \[2 or 1, 32\]"):
            ops.attention(q, k, v, o, Hn, groups=groups, key_bias=torch.zeros(3, 32, device=gpu))
        with pytest.raises(ValueError, match=r"need \[2 or 1, 32\]"):
            ops.attention(q, k, v, o, Hn, groups=groups, key_bias=torch.zeros(1, 64, device=gpu)[:, ::2])
        with pytest.raises(RuntimeError, match="key_bias is on cpu"):
            ops.attention(q, k, v, o, Hn, groups=groups, key_bias=kb.cpu())
    with pytest.raises(ValueError, match="needs groups="):
        ops.attention(q, k, v, o, Hn, key_bias=kb)
    # the C entries refuse what a caller that bypasses ops may pass
    lib = native.load()
    pad = torch.zeros(40, dtype=torch.float32, device=gpu)
    arr = (C.c_int32 * 3)(*ends)
    head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(1), q.stride(0), o.stride(1), o.stride(0), Bn, S, Hn, DH ** -0.5)
    tail = (None, 0, torch.cuda.current_stream().cuda_stream)

    def raw_grouped(bias=kb.data_ptr(), sbb=0):
        return lib.rt_attention_fwd_grouped_biased(*head, C.cast(arr, C.c_void_p), 3, grouped.row_vis.data_ptr(), 0, *tail, bias, sbb)

    def raw_keyed(bias=kb.data_ptr(), sbb=0):
        return lib.rt_attention_fwd_keyed_biased(*head, keyed.row_vis.data_ptr(), 0, keyed.key_class.data_ptr(), 0, *tail, bias, sbb)

    for raw in (raw_grouped, raw_keyed):
        assert raw(bias=None) == native.RT_E_BADARG and raw(sbb=-1) == native.RT_E_BADARG
        assert raw(bias=pad.data_ptr() + 2) == native.RT_E_ALIGN
        assert raw() == 0
    torch.cuda.synchronize()
