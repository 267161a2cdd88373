"""Head-128 rt_attention_fwd (through ops.attention) at the lengths where a flash kernel goes wrong — one ragged tile and nothing else, 64k - 1,
64k, 64k + 1, S = 1 — and the key-split tail at the smallest shape that splits, against an fp64 reference, judged PER ELEMENT, on
guarded buffers: NaN in the rows behind S and in the pad columns of the fused q|k|v buffer (a V row past S that reaches the MFMA gives
0 x NaN: masking the score alone is not enough), a sentinel around the output.

Reference (support_kernels.attention_ref): fp64 softmax-attention from the bf16 inputs. Bound, per element:
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
p the fp64 softmax row. First term: the bf16 rounding of the output. Second: the bf16 rounding of P as the second product's operand and
of the normaliser, each at most 2^-9 relative. slack: the fp32 exp2, score arithmetic and accumulation; see attn_slack.

Runs with rt_attention_variant(0) — csrc/attention.hip, the kernel that serves every length — and with variant 2 for the one length of
the sweep that csrc/attention_v3.hip takes (S % 256 == 0: 256)."""
import pytest
import torch

from support_kernels import BF16, NAN, SENT, attention_ref, check_bound, same_bits, twice

pytestmark = pytest.mark.gpu

# Worst excess of |got - ref| over the first two terms of the bound, across the length sweep, the late-key cases, the narrow-store case
# and the key-split shapes (split and unsplit), both kernels, measured on an MI355X (run this file with -s: every case prints its own
# excess): 0.0 everywhere (worst err/bound 0.80). With nothing measured to multiply by 4, the slack is
# 2^-20 max|v| of the case's data (about 4.5e-6 here), which the fp32 exp2, score arithmetic and accumulation stay far inside.
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


LENGTHS = [1, 7, 63, 64, 65, 127, 128, 129, 191, 256, 257]
B, H, DH = 2, 2, 128


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


class variant:
    """rt_attention_variant(mode) for the duration of a with-block; the previous mode is restored whatever happens."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from reptext_amd import native

        self.lib = native.load()
        self.prev = self.lib.rt_attention_variant(-1)
        self.lib.rt_attention_variant(self.mode)

    def __exit__(self, *exc):
        self.lib.rt_attention_variant(self.prev)


def make_qkv(Bn, S, Hn, seed, late_key_rows=()):
    """bf16 [Bn, S, 3 * Hn * 128] on the CPU, q scaled by 2 (a sharper softmax than N(0,1) scores). late_key_rows = (b, h, row): the LAST key
    of (b, h) becomes that query row's direction, so its score is ~45 above the rest and the running-max rescale fires on the last tile."""
    d = Hn * DH
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(Bn, S, 3 * d, generator=g)
    qkv[..., :d] *= 2.0
    qkv = qkv.to(BF16)
    for b, h, row in late_key_rows:
        qkv[b, S - 1, d + h * DH : d + (h + 1) * DH] = qkv[b, row, h * DH : (h + 1) * DH]
    return qkv


def reference(qkv, Hn, scale=None):
    Bn, S, _ = qkv.shape
    d = Hn * DH
    q, k, v = (qkv[..., i * d : (i + 1) * d].float().reshape(Bn, S, Hn, DH) for i in range(3))
    ref, pv = attention_ref(q, k, v, scale)
    return ref, pv, float(v.abs().max())


def fused_buffer(qkv, device):
    """[Bn, S + 70, 3d + 64] with NaN in rows S.. of every batch entry and in the pad columns (more than one 64-key tile behind S: a ragged
    tile's over-read would land in NaN, inside the allocation); ld > 3d, padded batch stride. Returns (buffer, q, k, v views)."""
    Bn, S, d3 = qkv.shape
    buf = torch.full((Bn, S + 70, d3 + 64), NAN, dtype=BF16)
    buf[:, :S, :d3] = qkv
    buf = buf.to(device)
    d = d3 // 3
    return (buf,) + tuple(buf[:, :S, i * d : (i + 1) * d] for i in range(3))


def new_o(Bn, S, d, device, ldo=None):
    """[Bn, S + 3, ldo] holding the sentinel (ldo = d + 8 differs from ld), and its [Bn, S, d] view."""
    buf = torch.full((Bn, S + 3, d + 8 if ldo is None else ldo), SENT, dtype=BF16, device=device)
    return buf, buf[:, :S, :d]


def guards_intact(obuf, S, d):
    m = torch.ones(obuf.shape, dtype=torch.bool, device=obuf.device)
    m[:, :S, :d] = False
    return same_bits(obuf[m], torch.full_like(obuf[m], SENT))


def check_attention(what, got, ref, pv, vmax, slack_of=attn_slack):
    """The per-element bound; prints the part of the error the slack has to carry before it asserts. slack_of: the attn_slack of the
    file that asks (test_attention_v3_edges_gpu.py keeps a MEASURED_EXCESS of its own)."""
    got, ref, pv = got.double().cpu(), ref.double(), pv.double()
    base = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * pv
    slack = slack_of(vmax)
    excess = float(((got - ref).abs() - base).max())
    print(f"[attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    return check_bound(what, got, ref, base + slack)


def run_guarded(ops, qkv, Hn, device, what, ref=None, ldo=None, split=True, check_entries=True, scale=None, slack_of=attn_slack):
    """Out of place on guarded buffers, twice; bound, guards, inputs untouched; in place over q; every entry alone. Returns the output.
    scale: the softmax scale of every launch and of the reference (None: the kernels' default, 128^-0.5)."""
    Bn, S, _ = qkv.shape
    d = Hn * DH
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()

    def run():
        obuf, o = new_o(Bn, S, d, device, ldo)
        ops.attention(q, k, v, o, Hn, scale=scale, split=split)
        torch.cuda.synchronize()
        return obuf

    obuf = twice(run)
    got = obuf[:, :S, :d]
    r, pv, vmax = reference(qkv, Hn, scale) if ref is None else ref
    check_attention(what, got, r, pv, vmax, slack_of)
    assert guards_intact(obuf, S, d), f"{what}: wrote outside [:S, :H*128] of the output"
    assert same_bits(buf, before), f"{what}: the kernel wrote to its inputs"
    # in place over q: the same bits, and nothing else of the fused buffer changes
    ops.attention(q, k, v, q, Hn, scale=scale, split=split)
    torch.cuda.synchronize()
    assert same_bits(q, got), f"{what}: in place over q differs"
    expect = before.clone()
    expect[:, :S, :d] = got
    assert same_bits(buf, expect), f"{what}: the in-place run touched more than q"
    if check_entries and Bn > 1:
        for b in range(Bn):                                        # entry b of the batched launch = the batch-1 launch of that entry
            _, q1, k1, v1 = fused_buffer(qkv[b : b + 1], device)
            o1buf, o1 = new_o(1, S, d, device, ldo)
            ops.attention(q1, k1, v1, o1, Hn, scale=scale, split=split)
            torch.cuda.synchronize()
            assert same_bits(o1buf[0], obuf[b]), f"{what}: entry {b} differs from its batch-1 launch"
    return got


@pytest.mark.parametrize("S,mode", [(S, 0) for S in LENGTHS] + [(256, 2)])
def test_attention_length_edges(ops, gpu, S, mode):
    qkv = make_qkv(B, S, H, 1000 + S)
    with variant(mode):
        run_guarded(ops, qkv, H, gpu, f"S={S} variant {mode}")


@pytest.mark.parametrize("S,mode", [(65, 0), (257, 0)])
def test_attention_late_dominant_key(ops, gpu, S, mode):
    """The dominant key is the LAST key, alone in the ragged tile: the rescale fires on a tile that is 63/64 masked."""
    rows = [(0, 0, 5), (0, 1, S - 1), (1, 0, 40), (1, 1, 64)]
    qkv = make_qkv(B, S, H, 2000 + S, late_key_rows=rows)
    d = H * DH
    with variant(mode):
        got = run_guarded(ops, qkv, H, gpu, f"late key S={S} variant {mode}").float().cpu()
    for b, h, row in rows:                                         # the row is (almost exactly) the value row of the last key
        vlast = qkv[b, S - 1, 2 * d + h * DH : 2 * d + (h + 1) * DH].float()
        assert float((got[b, row, h * DH : (h + 1) * DH] - vlast).abs().max()) < 0.05, (b, h, row)


def test_attention_narrow_output_rows(ops, gpu):
    """ldo % 8 == 4 takes the 8-byte store path: the same bits as the 16-byte one, inside its own guards."""
    S, d = 65, H * DH
    qkv = make_qkv(B, S, H, 3000)
    ref = reference(qkv, H)
    with variant(0):
        wide = run_guarded(ops, qkv, H, gpu, "S=65 ldo=d+8", ref=ref, check_entries=False)
        narrow = run_guarded(ops, qkv, H, gpu, "S=65 ldo=d+4", ref=ref, ldo=d + 4, check_entries=False)
    assert same_bits(narrow, wide)


@pytest.mark.parametrize("S", [2048, 2040])
def test_attention_key_split_tail_small(ops, gpu, S):
    """The smallest shape that splits on a 256-CU part (H = 8: 16 items per XCD group on 64 slots) and its ragged neighbour (the same tile
    counts), attention.hip: split and unsplit meet the fp64 bound, four more launches repeat the bits, entries of a batch of 3 equal the
    batch-1 launch, and the ticket counters are zero afterwards."""
    from reptext_amd import native

    Hn, d = 8, 8 * DH
    assert native.load().rt_attention_ws_bytes(1, S, Hn) > 0           # a part on which this shape does not split tests nothing: fail
    qkv = make_qkv(1, S, Hn, 4000 + S)
    for h, row, key in ((0, 10, 1500), (7, 2000, S - 3), (5, 1990, 70)):    # dominant keys on either side of a cut
        qkv[0, key, d + h * DH : d + (h + 1) * DH] = qkv[0, row, h * DH : (h + 1) * DH]
    ref = reference(qkv, Hn)
    with variant(0):
        got = run_guarded(ops, qkv, Hn, gpu, f"key split S={S}", ref=ref)
        run_guarded(ops, qkv, Hn, gpu, f"key split S={S} split=False", ref=ref, split=False)
        _, q, k, v = fused_buffer(qkv, gpu)
        for _ in range(4):
            obuf, o = new_o(1, S, d, gpu)
            ops.attention(q, k, v, o, Hn)
            assert same_bits(o, got)
        qkv3 = torch.cat([qkv, qkv.flip(1), qkv], dim=0)
        _, q3, k3, v3 = fused_buffer(qkv3, gpu)
        o3buf, o3 = new_o(3, S, d, gpu)
        ops.attention(q3, k3, v3, o3, Hn)
        torch.cuda.synchronize()
        assert same_bits(o3[0], got[0]) and same_bits(o3[2], got[0])
        assert guards_intact(o3buf, S, d)
        for Bn in (1, 3):                                              # the cached workspaces' ticket counters: B * H * ceil(S / 128) int32
            ws = ops._attention_workspace(Bn, S, Hn, gpu)
            n = Bn * Hn * ((S + 127) // 128)
            assert ws is not None and int(ws[: 4 * n].view(torch.int32).abs().max()) == 0
