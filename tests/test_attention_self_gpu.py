"""rt_attention_fwd_keyed_self (through ops.attention(groups=ops.KeyClasses, self_key=True)): the keyed rule, and row i also sees key i
(perturbed-attention guidance). The harness of test_attention_keyed_gpu.py — guarded q|k|v buffer, sentinel around the output, two
launches with the same bits, in place over q, inputs untouched, every entry alone — against that file's fp64 softmax with
`visible |= eye(S)`, judged PER ELEMENT with its bound
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack

What can go wrong that the keyed kernel cannot: the self bit on another score register, lane half or tile than the row's own key; a
one-class tile hidden from a row still taking the whole-tile hide; a key-split run that holds nothing but hidden tiles weighing in.
With every word 0 each row sees its own key alone: p = exp2(0) = 1 in bf16, l = 1 up to an fp32 rounding of the exponent's argument
(far below half a bf16 ulp), fp32 accumulation of 1·v_i and exact zeros — the output is v bit for bit, which follows from the
arithmetic and is asserted as such."""
import numpy as np
import pytest
import torch

from support_kernels import check_bound, same_bits, twice
from test_attention_edges_gpu import DH, fused_buffer, guards_intact, make_qkv, new_o
from test_attention_groups_gpu import SWEEP, sweep_table
from test_attention_keyed_gpu import classes, visible

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


def self_visible(vis, cls):
    see = visible(vis, cls)
    return see | torch.eye(see.shape[1], dtype=torch.bool)[None]


def self_reference(qkv, Hn, vis, cls):
    """fp64 softmax-attention with -inf on the hidden keys, row i's own key never hidden; (ref, sum p|v|, max|v|)."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    q, k, v = (qkv[..., i * d : (i + 1) * d].double().reshape(Bn, S, Hn, DH) for i in range(3))
    see = self_visible(vis, cls)
    ref, pv = torch.zeros(Bn, S, Hn, DH, dtype=torch.float64), torch.zeros(Bn, S, Hn, DH, dtype=torch.float64)
    for b in range(Bn):
        sb = see[b if see.shape[0] > 1 else 0]
        for h in range(Hn):
            s = ((q[b, :, h] @ k[b, :, h].t()) * DH ** -0.5).masked_fill(~sb, float("-inf"))
            p = torch.softmax(s, dim=-1)
            ref[b, :, h], pv[b, :, h] = p @ v[b, :, h], p @ v[b, :, h].abs()
    return ref.reshape(Bn, S, d), pv.reshape(Bn, S, d), float(v.abs().max())


def check_attention(what, got, ref, pv, vmax):
    got, ref, pv = got.double().cpu(), ref.double(), pv.double()
    base = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * pv
    slack = attn_slack(vmax)
    excess = float(((got - ref).abs() - base).max())
    print(f"[self attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    return check_bound(what, got, ref, base + slack)


def run_self(ops, qkv, Hn, device, what, vis, cls, split=True, reference=True):
    """run_keyed of the keyed file with self_key=True: out of place on guarded buffers, twice; bound, guards, inputs untouched; in place
    over q; every entry alone. vis uint32 / cls uint8 numpy [B or 1, S]. Returns the output."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()
    groups = classes(ops, vis, cls, device)

    def run():
        obuf, o = new_o(Bn, S, d, device)
        ops.attention(q, k, v, o, Hn, split=split, groups=groups, self_key=True)
        torch.cuda.synchronize()
        return obuf

    obuf = twice(run)
    got = obuf[:, :S, :d]
    if reference:
        check_attention(what, got, *self_reference(qkv, Hn, vis, cls))
    assert guards_intact(obuf, S, d), f"{what}: wrote outside [:S, :H*128] of the output"
    assert same_bits(buf, before), f"{what}: the kernel wrote to its inputs"
    ops.attention(q, k, v, q, Hn, split=split, groups=groups, self_key=True)
    torch.cuda.synchronize()
    assert same_bits(q, got), f"{what}: in place over q differs"
    expect = before.clone()
    expect[:, :S, :d] = got
    assert same_bits(buf, expect), f"{what}: the in-place run touched more than q"
    if Bn > 1:
        for b in range(Bn):
            _, q1, k1, v1 = fused_buffer(qkv[b : b + 1], device)
            o1buf, o1 = new_o(1, S, d, device)
            vb, cb = (vis[b : b + 1] if vis.shape[0] > 1 else vis), (cls[b : b + 1] if cls.shape[0] > 1 else cls)
            ops.attention(q1, k1, v1, o1, Hn, split=split, groups=classes(ops, vb, cb, device), self_key=True)
            torch.cuda.synchronize()
            assert same_bits(o1buf[0], obuf[b]), f"{what}: entry {b} differs from its batch-1 launch"
    return got


SPLITS = [True, False]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("S", SWEEP)
def test_self_all_words_zero_returns_v(ops, gpu, S, split):
    """(a) Every row sees its own key alone, in one-class tiles and in mixed ones: the output is v bit for bit."""
    Bn, Hn = 2, 2
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 7000 + S)
    vis = np.zeros((Bn, S), dtype=np.uint32)
    j = np.arange(S)
    for name, cls in (("one class", np.zeros((1, S), dtype=np.uint8)), ("class j % 32", (j % 32).astype(np.uint8)[None])):
        got = run_self(ops, qkv, Hn, gpu, f"all words 0, {name}, S={S} split={split}", vis, cls, split=split)
        assert same_bits(got, qkv[..., 2 * d :].to(gpu)), f"{name}: a row that sees its own key alone does not return its value row"


@pytest.mark.parametrize("split", SPLITS)
def test_self_all_words_zero_at_a_split_shape(ops, gpu, split):
    """(a) at S = 2048, H = 8 (the smallest shape that splits on a 256-CU part): all but one run of a split item see nothing and must
    weigh 0 in the combine."""
    from reptext_amd import native

    S, Hn = 2048, 8
    d = Hn * DH
    assert native.load().rt_attention_ws_bytes(1, S, Hn) > 0
    qkv = make_qkv(1, S, Hn, 7100)
    got = run_self(ops, qkv, Hn, gpu, f"all words 0, split shape, split={split}", np.zeros((1, S), dtype=np.uint32),
                   (np.arange(S) % 3).astype(np.uint8)[None], split=split, reference=False)
    assert same_bits(got, qkv[..., 2 * d :].to(gpu))
    ws = ops._attention_workspace(1, S, Hn, gpu)
    n = Hn * ((S + 127) // 128)
    assert ws is not None and int(ws[: 4 * n].view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("S", SWEEP)
def test_self_perturbed_tables(ops, gpu, S, split):
    """(b) The tables of the pipeline's rule with T = 64 text rows, per-batch [2, S]: entry 0 perturbed (an image row sees the text keys
    and its own), entry 1 sees everything. S = 64: text rows alone."""
    from reptext_amd.pipeline import perturbed_attention_tables

    Hn, T = 2, 64
    qkv = make_qkv(2, S, Hn, 7200 + S)
    row_vis, key_class = perturbed_attention_tables(T, S - T, 1)
    assert row_vis.shape == (2, S) and key_class.shape == (1, S)
    run_self(ops, qkv, Hn, gpu, f"perturbed tables S={S} split={split}", row_vis.numpy().view(np.uint32), key_class.numpy(), split=split)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("S", SWEEP)
def test_self_sweep_words(ops, gpu, S, split):
    """(c) sweep_table's words (all / one class / all but one / the last / nothing, row by row and by whole wave blocks) over class j % 32."""
    Bn, Hn = 2, 2
    qkv = make_qkv(Bn, S, Hn, 7300 + S)
    cls = (np.arange(S) % 32).astype(np.uint8)[None]
    vis = np.stack([sweep_table(S, 32, 0), sweep_table(S, 32, 3)])
    assert (vis == 0).any() and (vis == 0xFFFFFFFF).any()
    run_self(ops, qkv, Hn, gpu, f"sweep words S={S} split={split}", vis, cls, split=split)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("S", SWEEP)
def test_self_rows_that_see_their_own_class_are_the_keyed_launch(ops, gpu, S, split):
    """(d) Every row's word holds its own class's bit (and other bits as sweep_table gives them): the self rule adds nothing, and the
    launch gives the bits of rt_attention_fwd_keyed."""
    Bn, Hn = 2, 2
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 7400 + S)
    j = np.arange(S)
    cls = np.stack([(7 * j + b) % 5 for b in range(Bn)]).astype(np.uint8)
    vis = np.stack([sweep_table(S, 5, 0), sweep_table(S, 5, 3)]) | (np.uint32(1) << cls.astype(np.uint32))
    _, q, k, v = fused_buffer(qkv, gpu)
    _, o_k = new_o(Bn, S, d, gpu)
    groups = classes(ops, vis, cls, gpu)
    ops.attention(q, k, v, o_k, Hn, split=split, groups=groups)
    got = run_self(ops, qkv, Hn, gpu, f"own class visible S={S} split={split}", vis, cls, split=split)
    assert same_bits(got, o_k[:, :S, :d]), "a row that sees its own class differs from the keyed launch"


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("S", [65, 129, 257])
def test_self_last_row_of_a_ragged_length(ops, gpu, S, split):
    """(e) The last row's own key is the last key, alone in the ragged last tile: with word 0 it returns v[S-1] bit for bit, while the
    other rows see class 0 = every key but the last."""
    Bn, Hn = 2, 2
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 7500 + S)
    cls = np.zeros((1, S), dtype=np.uint8)
    cls[0, S - 1] = 1
    vis = np.ones((Bn, S), dtype=np.uint32)
    vis[:, S - 1] = 0
    got = run_self(ops, qkv, Hn, gpu, f"ragged last row S={S} split={split}", vis, cls, split=split)
    assert same_bits(got[:, S - 1], qkv[:, S - 1, 2 * d :].to(gpu))
