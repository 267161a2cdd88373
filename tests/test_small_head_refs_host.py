"""The references behind tests/test_small_head_attention_edges_gpu.py are code too: support_kernels.attention_ref generalised to
Sq != Sk and to a q shared by the batch, and the key-selection construction of small_head_attention.py (its precondition, its answer,
and that the comparison the GPU test makes rejects a wrong answer). No GPU."""
import pytest
import torch
import torch.nn.functional as F

import small_head_attention as sha
from support_kernels import BF16, F64, attention_ref, same_bits


def _rand(Bq, B, Sq, Sk, H, Dh, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Bq, Sq, H, Dh, generator=g).to(BF16), torch.randn(B, Sk, H, Dh, generator=g).to(BF16),
            torch.randn(B, Sk, H, Dh, generator=g).to(BF16))


@pytest.mark.parametrize("Bq, B, Sq, Sk, H, Dh, scale", [(2, 2, 5, 17, 2, 72, None), (2, 2, 17, 5, 3, 72, None), (1, 3, 1, 65, 2, 72, None),
                                                       (1, 3, 33, 1, 2, 72, 0.5), (2, 2, 65, 64, 1, 64, 0.05), (1, 1, 130, 63, 2, 128, None)])
def test_attention_ref_is_sdpa_in_fp64(Bq, B, Sq, Sk, H, Dh, scale):
    """Rectangular shapes, a shared q and a custom scale against torch's scaled_dot_product_attention on fp64 tensors; pv against the
    same function on |v|. Both evaluate in fp64, in another order: 1e-12 relative to the largest |v| is a few thousand fp64 ulps."""
    q, k, v = _rand(Bq, B, Sq, Sk, H, Dh, 10 * Sq + Sk)
    ref, pv = attention_ref(q, k, v, scale)
    assert ref.shape == pv.shape == (B, Sq, H * Dh) and ref.dtype == pv.dtype == F64
    heads = lambda t: t.double().expand(B, -1, -1, -1).transpose(1, 2)
    for got, vv in ((ref, v), (pv, v.abs())):
        want = F.scaled_dot_product_attention(heads(q), heads(k), heads(vv), scale=scale).transpose(1, 2).reshape(B, Sq, H * Dh)
        assert float((got - want).abs().max()) <= 1e-12 * float(v.float().abs().max())


def test_attention_ref_keeps_its_values_for_the_square_case():
    """What its callers from before the generalisation get: the loop it had, written out here, bit for bit."""
    B, S, H, Dh = 2, 65, 2, 128
    q, k, v = _rand(B, B, S, S, H, Dh, 3)
    for scale in (None, 0.05):
        ref, pv = attention_ref(q.float(), k.float(), v.float(), scale)
        qd, kd, vd = q.double(), k.double(), v.double()
        sc = Dh ** -0.5 if scale is None else scale
        for b in range(B):
            for h in range(H):
                p = torch.softmax(qd[b, :, h] @ kd[b, :, h].t() * sc, dim=-1)
                assert same_bits(ref[b, :, h * Dh:(h + 1) * Dh], p @ vd[b, :, h])
                assert same_bits(pv[b, :, h * Dh:(h + 1) * Dh], p @ vd[b, :, h].abs())


def test_attention_ref_refuses_a_batch_that_is_neither_one_nor_b():
    q, k, v = _rand(2, 3, 4, 4, 1, 64, 4)
    with pytest.raises(AssertionError):
        attention_ref(q, k, v)


@pytest.mark.parametrize("hd, B, Sq, Sk, H, own_q, seed", sha.SELECTION_CASES + sha.SELECTION_MAXIMA)
def test_key_selection_construction(hd, B, Sq, Sk, H, own_q, seed):
    """At every shape the GPU tests use: the inputs are exact in bf16 as built, pi covers what it has to, the gap precondition holds,
    and the fp64 reference IS v[pi], bit for bit (the chosen key's fp64 softmax weight is 1.0 and no other key moves the sum)."""
    q, k, v, pi = sha.selection_case(hd, B, Sq, Sk, H, seed)
    assert q.dtype == k.dtype == v.dtype == BF16 and q.shape == (B, Sq, H * hd) and k.shape == v.shape == (B, Sk, H * hd)
    assert bool((k.float().abs() == 2).all()) and bool((q.float().abs() == 8).all())
    assert 0.5 <= float(v.float().abs().min()) and float(v.float().abs().max()) <= 2.0
    if Sq == Sk:
        assert all(sorted(pi[b, h].tolist()) == list(range(Sk)) for b in range(B) for h in range(H))
    else:
        need = {0, Sk - 1} | {key for j in range((Sk + 63) // 64) for key in (64 * j, 64 * j + 63, 64 * j - 1) if 0 <= key < Sk}
        assert need <= set(pi.flatten().tolist())
    gap, distinct = sha.selection_gap(q, k, pi, hd)
    print(f"hd{hd} B={B} Sq={Sq} Sk={Sk} H={H} seed {seed}: smallest gap {gap:.1f}")
    assert gap >= sha.MIN_GAP and distinct
    ref, _ = attention_ref(q.reshape(B, Sq, H, hd), k.reshape(B, Sk, H, hd), v.reshape(B, Sk, H, hd))
    want = sha.selection_expected(v, pi, hd)
    assert same_bits(ref, want.double())


@pytest.mark.parametrize("hd, Sq, Sk", [(64, 65, 65), (72, 17, 129)])
def test_key_selection_comparison_rejects_a_wrong_answer(hd, Sq, Sk):
    """The GPU test compares bits with selection_expected(v, pi). With the fp64 reference rounded to bf16 in the kernel's place: the
    right pi passes; a pi with two rows exchanged, a pi moved to the neighbouring key in one row, and two exchanged output columns
    (inside the first 64 and inside the 72 tail) all fail."""
    B, H = 2, 2
    q, k, v, pi = sha.selection_case(hd, B, Sq, Sk, H, 21)
    ref, _ = attention_ref(q.reshape(B, Sq, H, hd), k.reshape(B, Sk, H, hd), v.reshape(B, Sk, H, hd))
    got = ref.to(BF16)
    assert same_bits(got, sha.selection_expected(v, pi, hd))
    swapped = pi.clone()
    swapped[1, 0, [0, Sq - 1]] = swapped[1, 0, [Sq - 1, 0]]
    assert swapped[1, 0, 0] != pi[1, 0, 0]
    assert not same_bits(got, sha.selection_expected(v, swapped, hd))
    shifted = pi.clone()
    shifted[0, 1, Sq - 1] = (shifted[0, 1, Sq - 1] + 1) % Sk
    assert not same_bits(got, sha.selection_expected(v, shifted, hd))
    for swap in ((0, 1), (31, 32)) + (((64, 71),) if hd == 72 else ((62, 63),)):
        assert not same_bits(got, sha.selection_expected(v, pi, hd, swap=swap))


def test_key_selection_gap_sees_a_close_second_and_a_repeated_key():
    """selection_gap itself: an unchosen key made a copy of a chosen one gives a gap of 0 and is reported as a repeated row; one sign
    away from it, a gap of 32 / sqrt(hd)."""
    hd, Sq, Sk = 64, 17, 129
    q, k, v, pi = sha.selection_case(hd, 1, Sq, Sk, 1, 22)
    chosen = int(pi[0, 0, 0])
    other = next(key for key in range(Sk) if key not in set(pi.flatten().tolist()))
    near = k.clone()
    near[0, other] = k[0, chosen]
    gap, distinct = sha.selection_gap(q, near, pi, hd)
    assert gap == 0.0 and not distinct
    near[0, other, 5] = -near[0, other, 5]
    gap, distinct = sha.selection_gap(q, near, pi, hd)
    assert abs(gap - 32 / hd ** 0.5) < 1e-9 and distinct
