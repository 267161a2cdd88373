"""rt_attention_hd64 and rt_attention_hd72 (csrc/attention_small_head.hip, through ops.attention_hd64 / ops.attention_hd72) where a flash
kernel goes wrong, against the fp64 reference, judged PER ELEMENT, on the guarded buffers of small_head_attention.guarded: NaN rows
behind the keys and behind the queries, NaN pad columns, a sentinel around the output, five launches (the host's choice twice, then 1,
2 and 4 waves per workgroup) with the same bits, inputs untouched, every batch entry equal to its batch-1 launch.

  a. a length sweep: one ragged tile and nothing else, 64k - 1, 64k, 64k + 1, a last 16-row query tile with 1, 15 and 16 live rows,
     the encoders' own token counts; three heads, so that heads start at columns that are no multiple of 64;
  b. rectangular shapes (head 72), Sq > Sk among them, with q in a buffer of its own (ldq != ldkv, another batch stride), with one q
     shared by the batch (stride_qb = 0), and at B = 1;
  c. key selection: inputs whose softmax weight is 1.0 on one key per row, so the output must have that key's v row, bit for bit;
  d. q = 0: P is exactly 1 and the output the mean of v;
  e. a dominant key alone in the ragged last tile (the rescale fires on a tile that is 63/64 masked) and in the first (alpha = 1 after it);
  f. scales other than hd^-0.5;
  g. the admitted maxima, S = RT_ATTENTION_HD64_MAX_S and Sq = Sk = RT_ATTENTION_HD72_MAX_S.

Reference (support_kernels.attention_ref): fp64 softmax-attention from the bf16 inputs. Bound, per element, as in
test_attention_edges_gpu.py (check_attention is imported from there):
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
p the fp64 softmax row. First term: the bf16 rounding of the output. Second: the bf16 rounding of P as the second product's operand
(this kernel takes the row sum from the unrounded P, so nothing else is rounded to bf16). slack: the fp32 exp2, score arithmetic and
accumulation; see attn_slack. (c) has no tolerance at all, and the bound of (d) is derived."""
import functools

import pytest
import torch

import small_head_attention as sha
from support_kernels import BF16, U23, attention_ref, check_bound, same_bits
from test_attention_edges_gpu import check_attention

pytestmark = pytest.mark.gpu

# Worst excess of |got - ref| over the first two terms of the bound across every case of this file (a, b, e, f, g; both head dims),
# measured on an MI355X against the fp64 reference (run this file with -s: every case prints its own excess): 0.0 in every one of the
# 55 cases. Worst err/bound: 0.769, (f) hd72 at S = 129 with scale 0.5 (a 0.661, b 0.753, e 0.599, g 0.416). With nothing measured to
# multiply by 4, the slack is 2^-20 max|v| of the case's data (4.0e-6 ... 4.6e-6).
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


HDS = (64, 72)
SWEEP = [1, 7, 15, 16, 17, 63, 64, 65, 127, 128, 129]
TOKENS = {64: 257, 72: 729}                      # CLIP ViT-L/14 and SigLIP-so400m
SWEEP_CASES = [(hd, S) for hd in HDS for S in SWEEP + [TOKENS[hd]]]
LONG_CASES = [(hd, S) for hd in HDS for S in (65, TOKENS[hd])]


@functools.lru_cache(maxsize=None)
def random_case(hd, B, Sq, Sk, H, Bq, seed, scale=None, late=(), early=()):
    """CPU bf16 q [Bq, Sq, H·hd] (randn scaled by 2: a sharper softmax than N(0, 1) scores), k and v [B, Sk, H·hd] (randn), with
    their fp64 result: (q, k, v, ref, pv, max|v|). late / early = (b, h, row)s: the LAST key / key 3 of (b, h) becomes that row's q."""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    q = (2.0 * torch.randn(Bq, Sq, d, generator=g)).to(BF16)
    k, v = torch.randn(B, Sk, d, generator=g).to(BF16), torch.randn(B, Sk, d, generator=g).to(BF16)
    for rows, key in ((late, Sk - 1), (early, 3)):
        for b, h, row in rows:
            k[b, key, h * hd:(h + 1) * hd] = q[b, row, h * hd:(h + 1) * hd]
    ref, pv = attention_ref(q.reshape(Bq, Sq, H, hd), k.reshape(B, Sk, H, hd), v.reshape(B, Sk, H, hd), scale)
    return q, k, v, ref, pv, float(v.float().abs().max())


def run_random(gpu, what, hd, B, Sq, Sk, H, Bq, seed, own_q, scale=None, late=(), early=()):
    q, k, v, ref, pv, vmax = random_case(hd, B, Sq, Sk, H, Bq, seed, scale, late, early)
    got = sha.guarded(gpu, hd, q, k, v, H, own_q, scale)
    check_attention(what, got, ref, pv, vmax, attn_slack)
    return got, v


def run_selection(gpu, hd, B, Sq, Sk, H, own_q, seed):
    """The precondition on the inputs (from the fp64 scores alone), then the kernel's output against v[pi], bit for bit."""
    q, k, v, pi = sha.selection_case(hd, B, Sq, Sk, H, seed)
    gap, distinct = sha.selection_gap(q, k, pi, hd)
    print(f"[selection] hd{hd} B={B} Sq={Sq} Sk={Sk} H={H}: smallest gap of scale*score {gap:.1f}, k rows distinct: {distinct}")
    assert gap >= sha.MIN_GAP and distinct
    got = sha.guarded(gpu, hd, q, k, v, H, own_q)
    want = sha.selection_expected(v, pi, hd)
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert same_bits(got, want), f"{len(bad)} elements differ from v[pi], the first at (b, row, column) {tuple(bad[0].tolist())}"


# ------------------------------------------------------------------------------------------------------------------- a. lengths
@pytest.mark.parametrize("hd, S", SWEEP_CASES)
def test_small_head_length_sweep(gpu, hd, S):
    """Self-attention on the fused q|k|v layout, B = 2, H = 3. Excess over the first two terms of the bound, measured on an MI355X:
    0.0 at every length, both head dims; worst err/bound 0.661 (hd64, S = 15)."""
    run_random(gpu, f"hd{hd} S={S}", hd, 2, S, S, 3, 2, 100 * S + hd, False)


# ---------------------------------------------------------------------------------------------------------------- b. rectangular
RECT = [(1, 64), (1, 65), (5, 17), (17, 5), (33, 1), (65, 64), (130, 63)]
LAYOUTS = {"own q": (2, 2), "shared q": (3, 1), "batch 1": (1, 1)}              # (B, Bq)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("Sq, Sk", RECT)
def test_small_head_rectangular_hd72(gpu, Sq, Sk, layout):
    """q in a buffer of its own, H = 2: B = 2 with its own leading dimension and batch stride; B = 3 with one q for the whole batch
    (stride_qb = 0); B = 1 (ops passes stride_qb = 0 there too). With one key the output is v, bit for bit. Excess over the first two
    terms of the bound, measured on an MI355X: 0.0 in all 21 cases; worst err/bound 0.753 ((17, 5), shared q)."""
    B, Bq = LAYOUTS[layout]
    got, v = run_random(gpu, f"hd72 Sq={Sq} Sk={Sk} {layout}", 72, B, Sq, Sk, 2, Bq, 1000 * Sq + 10 * Sk + B, True)
    if Sk == 1:
        assert same_bits(got, v.expand(B, Sq, -1).contiguous())


# -------------------------------------------------------------------------------------------------------------- c. key selection
@pytest.mark.parametrize("hd, B, Sq, Sk, H, own_q, seed", sha.SELECTION_CASES)
def test_small_head_key_selection_is_bit_exact(gpu, hd, B, Sq, Sk, H, own_q, seed):
    """small_head_attention.selection_case: every other key's weight underflows below an fp32 ulp of the row sum and of every
    |v| >= 0.5, so row i must have the bits of v[pi(i)]: every row, every output column (the 72 tail too) and the key order of the
    P and Vᵀ fragments, with no tolerance. Smallest gaps (a condition on the inputs, checked here and in
    tests/test_small_head_refs_host.py): 56.6 (hd72, S = 729) ... 79.2 (hd72, S = 65)."""
    run_selection(gpu, hd, B, Sq, Sk, H, own_q, seed)


# ----------------------------------------------------------------------------------------------------------------------- d. q = 0
@pytest.mark.parametrize("hd, S", SWEEP_CASES)
def test_small_head_zero_queries_give_the_mean_of_v(gpu, hd, S):
    """q = 0: every score is 0, every P exactly 1 (exact in bf16), the row sum exactly S. Bound, derived and with no measured slack:
        |got - mean_j v_j| <= 2^-8 |ref| + (S + 8) 2^-23 mean_j |v_j|
    the bf16 rounding of the output, and S fp32 additions plus the few operations around them (the products with alpha = 1 and with
    1 / S), relative to the mean of |v|. A key >= S that is not masked, or a key left out, is an error of 1 / S of a v at its element.
    Worst err/bound measured on an MI355X: 0.994 (hd64, S = 7, where the first term alone is half a bf16 ulp of ref)."""
    B, H = 2, 3
    _, k, v, _, _, _ = random_case(hd, B, S, S, H, B, 100 * S + hd, None, (), ())
    got = sha.guarded(gpu, hd, torch.zeros_like(k), k, v, H, False)
    vd = v.double()
    ref, mab = vd.mean(dim=1, keepdim=True).expand(B, S, -1), vd.abs().mean(dim=1, keepdim=True).expand(B, S, -1)
    check_bound(f"hd{hd} S={S} q=0", got, ref, 2.0 ** -8 * ref.abs() + (S + 8) * U23 * mab)


# -------------------------------------------------------------------------------------------------------------- e. dominant keys
@pytest.mark.parametrize("hd, S", LONG_CASES)
def test_small_head_dominant_keys(gpu, hd, S):
    """For four (b, h, row) — rows of the first, a middle and the last query tile, row S - 1 among them — the LAST key is the row's
    own q: alone in the ragged tile, so the rescale fires on a tile that is 63/64 masked. For three others key 3 is the row's q: the
    first tile dominates and alpha = 1 afterwards. Per-element bound; and each planted row is its key's v row to 0.05 (the fp64
    reference to 0.02: a condition on the inputs). Excess over the first two terms of the bound, measured on an MI355X:
    0.0 in all four cases; worst err/bound 0.599 (hd72, S = 65)."""
    B, H = 2, 2
    late = ((0, 0, 5), (0, 1, S - 1), (1, 0, S // 2), (1, 1, 16 * ((S - 1) // 16)))
    early = ((0, 0, S - 1), (1, 0, 9), (1, 1, S // 2 + 1))
    got, v = run_random(gpu, f"hd{hd} S={S} dominant keys", hd, B, S, S, H, B, 7000 + S + hd, False, late=late, early=early)
    ref = random_case(hd, B, S, S, H, B, 7000 + S + hd, None, late, early)[3]
    for rows, key in ((late, S - 1), (early, 3)):
        for b, h, row in rows:
            cols = slice(h * hd, (h + 1) * hd)
            assert float((ref[b, row, cols] - v[b, key, cols].double()).abs().max()) < 0.02, ("the inputs", b, h, row)
            assert float((got[b, row, cols].float() - v[b, key, cols].float()).abs().max()) < 0.05, (b, h, row, key)


# ----------------------------------------------------------------------------------------------------------------------- f. scale
@pytest.mark.parametrize("scale", [0.05, 0.5])
@pytest.mark.parametrize("hd", HDS)
def test_small_head_scale(gpu, hd, scale):
    """S = 129, B = 2, H = 2, against the reference at that scale: the maximum is taken on the raw scores and the scale is folded
    into one factor with log2 e. Excess over the first two terms of the bound, measured on an MI355X: 0.0 in all four cases;
    worst err/bound 0.769 (hd72, scale 0.5)."""
    run_random(gpu, f"hd{hd} S=129 scale={scale}", hd, 2, 129, 129, 2, 2, 9000 + hd, False, scale=scale)


# ---------------------------------------------------------------------------------------------------------- g. the admitted maxima
def _maximum(hd):
    from reptext_amd import native

    return native.RT_ATTENTION_HD64_MAX_S if hd == 64 else native.RT_ATTENTION_HD72_MAX_S


@pytest.mark.parametrize("hd", HDS)
def test_small_head_admitted_maximum(gpu, hd):
    """B = 1, H = 1 at S = RT_ATTENTION_HD64_MAX_S / Sq = Sk = RT_ATTENTION_HD72_MAX_S: the bounds the header admits are run.
    Excess over the first two terms of the bound, measured on an MI355X: 0.0 for both; worst err/bound 0.395 (hd64, S = 4096) and
    0.416 (hd72, S = 1024)."""
    S = _maximum(hd)
    run_random(gpu, f"hd{hd} S={S} (the maximum)", hd, 1, S, S, 1, 1, 11000 + hd, False)


@pytest.mark.parametrize("hd, B, Sq, Sk, H, own_q, seed", sha.SELECTION_MAXIMA)
def test_small_head_admitted_maximum_key_selection(gpu, hd, B, Sq, Sk, H, own_q, seed):
    """The key-selection form at the same lengths: a permutation of all S keys, bit for bit. Smallest gaps: 52.0 (hd64, S = 4096),
    64.1 (hd72, S = 1024)."""
    assert Sq == Sk == _maximum(hd), "small_head_attention.SELECTION_MAXIMA must follow the header's bounds"
    run_selection(gpu, hd, B, Sq, Sk, H, own_q, seed)
