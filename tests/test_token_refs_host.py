"""CPU checks of the references and bounds that test_token_passes_gpu.py and test_e4m3_producers_gpu.py judge the kernels by
(tests/support_kernels.py): each bound accepts the correctly rounded fp64 value and REJECTS a reference perturbed the way a plausible
kernel bug would perturb the output, at the element where that bug would show. No GPU, no kernel: got = the right answer, rounded to the
output format; ref = the wrong one."""
import pytest
import torch

from support_kernels import (BF16, FP8, QK_COUNTED, QK_EPS, U23, check_bound, check_quant_rows, fold_zero, layernorm_ref, qk_norm_rope_ref,
                             qk_tables, qk_weights, quant_rows_rule, ulp_e4m3, vt8_expected, vt8_key_order)


def test_ulp_e4m3_is_the_spacing_of_the_grid():
    """Every finite e4m3 value and its upper neighbour are ulp_e4m3 apart (the lower one's ulp), subnormals and zero included."""
    vals = torch.arange(0, 0x7F, dtype=torch.uint8).view(FP8).float().double()        # 0 .. 448, ascending
    assert float(vals[-1]) == 448.0
    assert torch.equal(vals[1:] - vals[:-1], ulp_e4m3(vals[:-1]))
    assert float(ulp_e4m3(torch.tensor(0.001))) == 2.0 ** -9 and float(ulp_e4m3(torch.tensor(-300.0))) == 32.0


@pytest.mark.parametrize("D", [520, 3072])
def test_layernorm_bound_rejects_a_mean_over_d_minus_8(D):
    """The row sum divided by D - 8 (the last chunk's columns counted out of the divisor). Row 0 sums to zero, so its mean is right
    either way; row 1 is 100 + randn, and every element of it fails."""
    g = torch.Generator().manual_seed(D)
    half = torch.randn(D // 2, generator=g) * 3
    x = torch.stack([torch.cat([half, -half]), 100 + torch.randn(D, generator=g)])[None]
    shift, scale = torch.randn(1, D, generator=g), torch.randn(1, D, generator=g) * 0.5
    y, by = layernorm_ref(x, shift, scale)
    got = y.to(BF16)
    check_bound("right mean", got, y, 2.0 ** -8 * y.abs() + by)
    yw, byw = layernorm_ref(x, shift, scale, mean_div=D - 8)
    with pytest.raises(AssertionError, match=r"at \(0, 1, \d+\)"):
        check_bound("mean over D - 8", got, yw, 2.0 ** -8 * yw.abs() + byw)
    err = (got.double() - yw).abs() > 2.0 ** -8 * yw.abs() + byw
    assert not bool(err[0, 0].any()) and float(err[0, 1].float().mean()) > 0.9


def test_qk_bound_rejects_text_weights_on_row_t():
    """Row T (the first image row) normalised with the text weights: the sets are O(1) apart, so that row fails and no other."""
    B, S, T, H = 2, 9, 4, 2
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, H, 128, generator=g).to(BF16)
    w = qk_weights(3)
    cos, sin = qk_tables(S, T)
    ref, mag = qk_norm_rope_ref(x, w[0], w[2], T, cos, sin, QK_EPS)
    got = ref.to(BF16)
    bound = lambda r, m: 2.0 ** -8 * r.abs() + QK_COUNTED * U23 * m
    check_bound("right rows", got, ref, bound(ref, mag))
    refw, magw = qk_norm_rope_ref(x, w[0], w[2], T, cos, sin, QK_EPS, txt_rows=T + 1)
    with pytest.raises(AssertionError, match=rf"at \(\d+, {T}, \d+, \d+\)"):
        check_bound("text weights on row T", got, refw, bound(refw, magw))
    bad = (got.double() - refw).abs() > bound(refw, magw)
    assert bool(bad[:, T].any()) and not bool(bad[:, :T].any()) and not bool(bad[:, T + 1 :].any())


@pytest.mark.parametrize("D", [520, 3080])
def test_quant_checks_reject_a_chunk_left_out_of_the_row_maximum(D):
    """The row maximum sits in the first 8 columns of the last 512-column chunk; a maximum taken without those 8 columns gives a
    smaller scale: the scale is no longer the rule's bit for bit, and x / scale at that element is far above 448 against a byte
    that saturated. Every other byte of the row is consistent with the wrong scale, so that one element is the only failure."""
    g = torch.Generator().manual_seed(D)
    x = torch.randn(3, D, generator=g)
    c0 = (D - 1) // 512 * 512
    x[1, c0 + 3] = 2.0 * float(x[1].abs().max())
    x = x.to(BF16)
    q, sc = quant_rows_rule(x)
    check_quant_rows("right maximum", q, sc, x)
    qw, scw = quant_rows_rule(x, skip_cols=(c0, c0 + 8))            # what a kernel with that bug writes: bytes and scale
    assert not torch.equal(sc, scw) and torch.equal(sc[[0, 2]], scw[[0, 2]])
    with pytest.raises(AssertionError, match=rf"at \(1, {c0 + 3}\)"):
        check_quant_rows("chunk left out", qw, scw, x)
    t = x.double() / scw.double()[:, None]
    bad = (qw.float().double() - t).abs() > 0.5 * ulp_e4m3(t) + 2.0 ** -21 * t.abs()
    assert bad.nonzero().tolist() == [[1, c0 + 3]]


def test_vt8_comparison_rejects_two_swapped_keys():
    """The documented key order, and what the byte comparison sees when positions 5 and 38 of every tile are exchanged: exactly those
    positions differ, and channel 0 (v[j][0] = j % 16 - 8) names the keys."""
    order = vt8_key_order()
    assert sorted(order.tolist()) == list(range(64))
    assert order[:8].tolist() == [0, 1, 2, 3, 8, 9, 10, 11] and order[16:20].tolist() == [32, 33, 34, 35] and order[32:36].tolist() == [4, 5, 6, 7]
    B, S, H = 1, 70, 2
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B, S, H, 128, generator=g).to(BF16)
    v[0, 3, 1, 7], v[0, 4, 0, 9] = 1000.0, -480.0
    v[:, :, 0, 0] = ((torch.arange(S) % 16) - 8).to(BF16)[None, :]
    exp = vt8_expected(v)
    assert exp.shape == (B, H, 128, 128) and not bool(exp[..., 64:][..., order >= S - 64].any())                          # keys >= S are zero
    assert int(exp[0, 1, 7, order.tolist().index(3)]) == 0x7E and int(exp[0, 0, 9, order.tolist().index(4)]) == 0xFE       # saturated, not NaN
    wrong = vt8_expected(v, swap=(5, 38))
    diff = (exp != wrong).nonzero()
    assert len(diff) > 0 and set((diff[:, 3] % 64).tolist()) == {5, 38}
    row = fold_zero(exp[0, 0, 0]).view(FP8).float()
    assert row[:64].tolist() == [float(int(k) % 16 - 8) for k in order]
