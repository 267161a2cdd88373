"""csrc/attention_v3.hip (through ops.attention) where ITS scheme can go wrong, against the fp64 reference, judged PER ELEMENT on the guarded
buffers of test_attention_edges_gpu.py (run_guarded: NaN rows behind S and NaN pad columns, a sentinel around the output, two launches
with the same bits, inputs untouched, in place over q, every batch entry equal to its batch-1 launch):

  A. a dominant key at every one of a tile's 64 positions (both 32-key halves, the 16 speculative numerators and the 16 late ones of
     each), in tile 0, in the last tile (the drain) and in between, for query rows of every wave and both 32-row blocks; once with a
     jump of ~196 log2 units (the speculative exp2 is +inf: the redo must overwrite it before an MFMA sees it), once with ~16;
  B. staircases of 16 key halves rising 3, 5.5, 6.5 and 9 log2 units per half: below the 2^6 threshold of the rescale decision (it
     fires only cumulatively, numerators up to 64 reach the MFMA), just below, just above, and well above it;
  C. 8 and 12 tiles unsplit: the 3-deep ring wraps more than once;
  D. the key-split tail at the smallest shapes that reach each path: segments of every length 1 .. 9 starting at any tile, runs that
     cross an item boundary, groups that split beside groups that do not, and a workgroup that runs a whole item and then two pieces.

Reference (support_kernels.attention_ref): fp64 softmax-attention from the bf16 inputs. Bound, per element, as in
test_attention_edges_gpu.py:
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
The first two terms hold for this kernel's scheme as they do for attention.hip's: a numerator formed against a stale maximum is up to
2^6 but still ONE bf16 rounding (2^-9 relative), the row sum is built on the matrix pipe from the same bf16 numerators, the output is
rounded once. slack: see attn_slack.

The split cases read the cut from a Python mirror of csrc/attention_split.h (group_cut, split_run) and assert through it the property
each shape is here for; a part on which a shape does not give that property fails the case (it must not pass untested)."""
import math

import pytest
import torch

from support_kernels import BF16, rel_l2, same_bits
from test_attention_edges_gpu import DH, fused_buffer, guards_intact, make_qkv, new_o, ops, reference, run_guarded, variant  # noqa: F401 (ops: fixture)

pytestmark = pytest.mark.gpu

# Worst excess of |got - ref| over the first two terms of the bound across every case of this file (A: S = 512 / 768 / 512 with scale 0.05,
# B, C: S = 512 / 768, D: the three shapes split and unsplit; attention_v3.hip and, where a case also runs it, attention.hip), measured on
# an MI355X against the fp64 reference (run this file with -s: every case prints its own excess): 0.0 in every case. Worst err/bound:
# attention_v3 0.844, attention.hip 0.895, both in A at S = 768 (B 0.59 / 0.76, C 0.56, D 0.58). With nothing measured to multiply by 4,
# the slack is 2^-20 max|v| of the case's data (4.3e-6 ... 5.2e-6).
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


# ------------------------------------------------------------------------------- the cut of csrc/attention_split.h, for attention_v3.hip
BQ3, BKV = 256, 64                   # query rows per item, keys per tile (attention_v3.hip)
SPLIT_MIN_TILES = 8
REC3_B = 135168                      # one (workgroup, segment) record of attention_v3.hip


def spx_of(device):
    """Workgroups per XCD group: one per CU."""
    return torch.cuda.get_device_properties(device).multi_processor_count // 8


def group_cut(S, H, spx, xcd):
    """(start, cnt, nfull, rem) of XCD group xcd: its first item and item count, how many it runs whole, how many it deals out in tiles."""
    ntiles, NI = S // BKV, H * (S // BQ3)
    base, extra = NI >> 3, NI & 7
    cnt = base + (1 if xcd < extra else 0)
    start = xcd * base + min(xcd, extra)
    nf = cnt // spx * spx
    rem = cnt - nf
    if rem > 0 and rem * 16 < spx * 15 and rem * ntiles >= spx * SPLIT_MIN_TILES:
        return start, cnt, nf, rem
    return start, cnt, cnt, 0


def split_run(S, H, spx, xcd, j):
    """The two segments (item, tb, te) of splitting workgroup j of a group with rem > 0; None where a segment is empty."""
    ntiles = S // BKV
    start, _, nfull, rem = group_cut(S, H, spx, xcd)
    U = rem * ntiles
    lo, hi = j * U // spx, (j + 1) * U // spx
    i0 = lo // ntiles
    first = start + nfull + i0
    segs = ((first, lo - i0 * ntiles, min(hi - i0 * ntiles, ntiles)), (first + 1, 0, hi - (i0 + 1) * ntiles))
    return [s if s[2] > s[1] else None for s in segs]


class Cut:
    """The cut of one (S, H) on `spx` workgroups per group: groups[x] = (start, cnt, nfull, rem); runs[x][j] = the two segments."""

    def __init__(self, S, H, spx):
        self.S, self.H, self.spx, self.ntiles, self.nqb = S, H, spx, S // BKV, S // BQ3
        self.groups = [group_cut(S, H, spx, x) for x in range(8)]
        self.runs = {x: [split_run(S, H, spx, x, j) for j in range(spx)] for x, g in enumerate(self.groups) if g[3] > 0}
        self.segments = [s for x in self.runs for run in self.runs[x] for s in run if s is not None]
        # what the kernel relies on: the segments of a split item are its tiles, each once, and no run touches a third item
        tiles = {}
        for item, tb, te in self.segments:
            tiles.setdefault(item, []).extend(range(tb, te))
        for x, (start, _, nfull, rem) in enumerate(self.groups):
            for item in range(start + nfull, start + nfull + rem):
                assert sorted(tiles.get(item, [])) == list(range(self.ntiles)), f"mirror: split item {item} of group {x} is not covered once"
        assert sum(len(t) for t in tiles.values()) == sum(g[3] for g in self.groups) * self.ntiles

    def where(self, item):
        """(head, first query row) of an item."""
        return item // self.nqb, (item % self.nqb) * BQ3

    def interior_cuts(self, x):
        """(item, t): a run of group x ends in front of tile t of a split item, 0 < t < ntiles."""
        start, _, nfull, rem = self.groups[x]
        U = rem * self.ntiles
        los = [j * U // self.spx for j in range(1, self.spx)]
        return [(start + nfull + lo // self.ntiles, lo % self.ntiles) for lo in los if lo % self.ntiles]


def cnt_bytes(B, S, H):
    return (B * H * ((S + 127) // 128) * 4 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------------------- helpers
def spike(qkv, b, h, row, key, mult=1.0):
    """Key `key` of (b, h) becomes mult x the query row `row`: that row's dominant key."""
    d = qkv.shape[-1] // 3
    qkv[b, key, d + h * DH : d + (h + 1) * DH] = (qkv[b, row, h * DH : (h + 1) * DH].float() * mult).to(BF16)


def value_row(qkv, b, h, key):
    d = qkv.shape[-1] // 3
    return qkv[b, key, 2 * d + h * DH : 2 * d + (h + 1) * DH].float()


def assert_rows_are_value_rows(what, got, qkv, placed, tol):
    got = got.float().cpu()
    for b, h, row, key in placed:
        err = float((got[b, row, h * DH : (h + 1) * DH] - value_row(qkv, b, h, key)).abs().max())
        assert err < tol, f"{what}: row {row} of (b {b}, head {h}) is {err:.3g} from the value row of its dominant key {key} (tile {key // BKV}, position {key % BKV})"


def assert_not_attention_hip(what, got, other):
    """`other`: attention.hip (variant 0) on the same data. Equal bits mean the launch was silently left to attention.hip."""
    print(f"[attention_v3] {what}: rel-L2 attention_v3 vs attention.hip {rel_l2(got.float().cpu(), other.float().cpu()):.3e}")
    assert not same_bits(got, other), f"{what}: the bits of attention.hip: attention_v3 did not take this launch"


def launch_variant0(ops, qkv, Hn, device, scale=None, split=True):
    Bn, S, _ = qkv.shape
    _, q, k, v = fused_buffer(qkv, device)
    obuf, o = new_o(Bn, S, Hn * DH, device)
    with variant(0):
        ops.attention(q, k, v, o, Hn, scale=scale, split=split)
        torch.cuda.synchronize()
    return o


# --------------------------------------------------------------------------------------- A. a dominant key at every position of a tile
@pytest.mark.parametrize("S,scale", [(512, None), (768, None), (512, 0.05)])
def test_v3_dominant_key_at_every_tile_position(ops, gpu, S, scale):
    """Query row 8p + 3 (p = 0 .. 63: every wave, both 32-row blocks of it, items 0 and 1) has key 64 (p mod ntiles) + p as its dominant
    key: position p of its tile, so all 64 positions occur (k0 and k1, speculative and late numerators), in tile 0, in the last tile
    and in between. Head 0: the key is 3 q (a jump of ~196 log2 units: exp2 of the speculative exponent is +inf, and 0 x inf would
    be NaN in O); head 1: 0.25 q (~16: over the threshold, nothing overflows). scale = 0.05 is the first non-default scale the bf16
    kernels are launched with. attention.hip runs the same data."""
    Hn, ntiles = 2, S // BKV
    qkv = make_qkv(1, S, Hn, 5000 + S)
    placed = [(0, 0, 8 * p + 3, BKV * (p % ntiles) + p) for p in range(64)]
    assert {key % BKV for _, _, _, key in placed} == set(range(64)) and {key // BKV for _, _, _, key in placed} >= {0, ntiles - 1}
    for h, mult in ((0, 3.0), (1, 0.25)):
        for _, _, row, key in placed:
            spike(qkv, 0, h, row, key, mult)
    ref = reference(qkv, Hn, scale)
    what = f"dominant keys S={S} scale={scale}"
    with variant(2):
        got = run_guarded(ops, qkv, Hn, gpu, f"{what} attention_v3", ref=ref, scale=scale, slack_of=attn_slack)
    with variant(0):
        other = run_guarded(ops, qkv, Hn, gpu, f"{what} attention.hip", ref=ref, scale=scale, slack_of=attn_slack)
    assert_not_attention_hip(what, got, other)
    assert_rows_are_value_rows(f"{what} attention_v3", got, qkv, placed, 0.08)
    assert_rows_are_value_rows(f"{what} attention.hip", other, qkv, placed, 0.08)


# ------------------------------------------------------------------------------------------- B. staircases around the 2^6 threshold
def test_v3_staircases_around_the_rescale_threshold(ops, gpu):
    """One query row r per (b, h); the 512 keys from `start` (inside a k1 half) are q_r s_j / (log2e scale |q_r|^2), so that row's score
    of key j is s_j = 12 + step (1 + (j - start) // 32) log2 units: a staircase of 16 key halves. step 3: no half outgrows the
    running maximum by 2^6 on its own (numerators up to 64 reach the MFMA and the row sum; the decision fires cumulatively); 5.5: it
    fires every other half; 6.5 and 9: every half. The top stays <= 160 log2 units (above that the fp32 score arithmetic eats into
    the bound's headroom). Rows in block a and block b of different waves and items."""
    Bn, Hn, S = 2, 2, 768
    d = Hn * DH
    qkv = make_qkv(Bn, S, Hn, 6000)
    unit = math.log2(math.e) * DH ** -0.5                                # log2 units per unit of q . k
    for (b, h), row, step, start in (((0, 0), 40, 3.0, 32), ((0, 1), 200, 5.5, 96), ((1, 0), 300, 6.5, 160), ((1, 1), 505, 9.0, 224)):
        assert start % BKV == 32 and start + 512 <= S and 12 + 16 * step <= 160
        q = qkv[b, row, h * DH : (h + 1) * DH].double()
        s = 12 + step * (1 + torch.arange(512, dtype=torch.float64) // 32)
        qkv[b, start : start + 512, d + h * DH : d + (h + 1) * DH] = (s[:, None] * q[None, :] / (unit * float(q.dot(q)))).to(BF16)
    ref = reference(qkv, Hn)
    with variant(2):
        got = run_guarded(ops, qkv, Hn, gpu, "staircases attention_v3", ref=ref, slack_of=attn_slack)
    with variant(0):
        other = run_guarded(ops, qkv, Hn, gpu, "staircases attention.hip", ref=ref, slack_of=attn_slack)
    assert_not_attention_hip("staircases", got, other)


# ---------------------------------------------------------------------------------------------------------- C. unsplit tile counts
@pytest.mark.parametrize("S", [512, 768])
def test_v3_unsplit_tile_counts(ops, gpu, S):
    """8 and 12 tiles, split=False: the 3-deep ring wraps more than once and no record is written."""
    Bn, Hn = 2, 2
    qkv = make_qkv(Bn, S, Hn, 7000 + S)
    with variant(2):
        got = run_guarded(ops, qkv, Hn, gpu, f"unsplit S={S} attention_v3", split=False, slack_of=attn_slack)
    assert_not_attention_hip(f"unsplit S={S}", got, launch_variant0(ops, qkv, Hn, gpu, split=False))


# --------------------------------------------------------------------------------------------------------- D. the key-split tail
def small_split_shape(cut):
    """(2, 2048, 9): every group deals 9 items out in runs of 9 tiles, so segments of every length 1 .. 9 occur and runs cross items."""
    lengths = {te - tb for _, tb, te in cut.segments}
    crossing = [run for x in cut.runs for run in cut.runs[x] if run[0] is not None and run[1] is not None]
    assert 1 in lengths and 2 in lengths and crossing, f"segment lengths {sorted(lengths)}, {len(crossing)} runs that cross an item boundary"


def mixed_groups_shape(cut):
    """(1, 1792, 11): groups of 10 items split (280 tiles on 32 workgroups), groups of 9 run whole (252 tiles < 8 per workgroup)."""
    assert any(g[3] > 0 for g in cut.groups) and any(g[3] == 0 and g[1] > 0 for g in cut.groups), "no group that splits beside one that does not"


def whole_then_pieces_shape(cut):
    """(1, 1536, 58): 44 or 43 items per group on 32 workgroups: a workgroup runs a whole item, then its two pieces of the other 12 or 11."""
    both = [g for g in cut.groups if g[2] > 0 and g[3] > 0]
    assert both and len({g[3] for g in both}) >= 2, "no group with whole items AND split items, or one rem only"


def place_split_keys(qkv, cut):
    """Dominant keys where the split can lose them; returns [(b, h, row, key)]. In three groups that split: the tile in front of a cut
    inside an item and the tile behind it. Where the shape has them: a single-tile segment, and the last tile of an item run whole."""
    Bn, nt, spots = qkv.shape[0], cut.ntiles, []
    for i, x in enumerate(list(cut.runs)[:: max(1, len(cut.runs) // 3)][:3]):
        cuts = cut.interior_cuts(x)
        item, t = cuts[(5 * i + 2) % len(cuts)]
        spots += [(item, t - 1), (item, t)]
    single = [s for s in cut.segments if s[2] - s[1] == 1]
    if single:
        spots.append((single[len(single) // 2][0], single[len(single) // 2][1]))
    whole = [g for g in cut.groups if g[2] > 0]
    if whole:
        start = max(whole, key=lambda g: g[3])[0]                    # a group that also splits, if there is one: its slot-0 item
        spots.append((start, nt - 1))
    placed = []
    for n, (item, tile) in enumerate(spots):
        h, q0 = cut.where(item)
        b, row, key = n % Bn, q0 + (41 * n + 9) % BQ3, BKV * tile + (23 * n + 5) % BKV
        spike(qkv, b, h, row, key)
        placed.append((b, h, row, key))
    assert len({p[:3] for p in placed}) == len(placed) and len({(p[0], p[1], p[3]) for p in placed}) == len(placed)
    return placed


@pytest.mark.parametrize("Bn,S,Hn,shape_is", [(2, 2048, 9, small_split_shape), (1, 1792, 11, mixed_groups_shape), (1, 1536, 58, whole_then_pieces_shape)])
def test_v3_key_split_tail(ops, gpu, Bn, S, Hn, shape_is):
    """The default variant (what the pipelines run; S >= 1536 is attention_v3's). Split and unsplit meet the fp64 bound; the rows whose
    dominant key sits beside a cut, alone in a one-tile segment or at the end of a whole item are that key's value row; the ticket
    counters are zero afterwards and four more launches repeat the bits."""
    from reptext_amd import native

    lib, spx, d = native.load(), spx_of(gpu), Hn * DH
    cut = Cut(S, Hn, spx)
    what = f"key split ({Bn}, {S}, {Hn})"
    try:
        assert cut.runs, "no group splits"
        shape_is(cut)
    except AssertionError as e:
        pytest.fail(f"{what} on {8 * spx} CUs does not reach the path it is here for ({shape_is.__name__}: {e}): it would test nothing")
    # the mirror and the library agree that this shape splits, on records of attention_v3's size
    for B1 in {1, Bn}:
        need = cnt_bytes(B1, S, Hn) + B1 * 8 * spx * 2 * REC3_B
        assert lib.rt_attention_ws_bytes(B1, S, Hn) >= need, f"{what}: workspace {lib.rt_attention_ws_bytes(B1, S, Hn)} < {need}"
    qkv = make_qkv(Bn, S, Hn, 8000 + S)
    placed = place_split_keys(qkv, cut)
    ref = reference(qkv, Hn)
    with variant(1):
        got = run_guarded(ops, qkv, Hn, gpu, f"{what} split", ref=ref, slack_of=attn_slack)
        whole = run_guarded(ops, qkv, Hn, gpu, f"{what} split=False", ref=ref, split=False, slack_of=attn_slack)
        assert_rows_are_value_rows(f"{what} split", got, qkv, placed, 0.05)
        assert_rows_are_value_rows(f"{what} split=False", whole, qkv, placed, 0.05)
        _, q, k, v = fused_buffer(qkv, gpu)
        for _ in range(4):
            obuf, o = new_o(Bn, S, d, gpu)
            ops.attention(q, k, v, o, Hn)
            assert same_bits(o, got) and guards_intact(obuf, S, d)
        for B1 in {1, Bn}:                                           # Bn > 1: run_guarded also launched every entry alone
            ws = ops._attention_workspace(B1, S, Hn, gpu)
            assert ws is not None and int(ws[: cnt_bytes(B1, S, Hn)].view(torch.int32).abs().max()) == 0, f"{what}: ticket counters left non-zero"
    assert_not_attention_hip(what, got, launch_variant0(ops, qkv, Hn, gpu))
