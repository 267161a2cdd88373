"""csrc/ip_attention.hip (through ops.ip_attention / ops.ip_attention_gated: rt_ip_attention, _gated and _rows) judged PER ELEMENT against an
fp64 reference, where the rel-L2 tests of this kernel cannot see: the eps of the q RMSNorm, the bf16 rounding of the normalised q, the
row maximum and the padded-key mask at scores far from 0, and the layout of every key position and output column.

Reference (support_kernels.ip_attention_ref64): fp64 from the bf16 / fp32 values the kernel reads, with q^ = bf16(q rsqrt(mean(q^2) + eps) wq)
rounded in the reference as the kernel rounds it. The query data is built so that the rounding is decidable (settle_q: no element of the
fp64 q^ within 2^-18 relative of a bf16 midpoint; the kernel's fp32 evaluation is about 12 roundings of 2^-24 plus the device rsqrtf).
Bound, per element, total = term + old under accumulate:
    |got - total| <= [bf16 o] 2^-8 |total| + 2^-8 pv + 2 E_s pv + [accumulate] 3 x 2^-24 (|term| + |old|) + slack
pv = |c| sum_j p_j |v_j|, c = ip_scale x row weight x gate. First term: the bf16 rounding of the store. Second: P rounded to bf16 as the
second product's operand (unit roundoff 2^-8; the row sum is taken from the unrounded P in fp32, so the normaliser adds no second 2^-8).
Third: the fp32 score error E_s to first order, through a row's own shift and the normaliser's; E_s < 0.01 is asserted so that the
linearisation holds. slack: see ip_slack.

Every launch runs on guarded buffers: q in columns 2d:3d of a NaN-filled [B, N + 3, 7d] buffer, k and v views of one NaN-filled
[Bk, n_ip + 3, 2d + 64] buffer (rows >= n_ip must not reach the LDS image), the gate in columns 2d:3d of a NaN-filled [B, 6d] table, the
row weights inside a longer NaN-filled vector, o inside a sentinel-filled [B, N + 3, d + 16] buffer (the prior contents under
accumulate). After each launch: everything outside [:N, :d] keeps its bits, every input keeps its bits, a second launch repeats the bits."""
import pytest
import torch

from support_kernels import BF16, F32, F64, NAN, SENT, bf16_round64, check_bound, ip_attention_ref64, ip_qhat64, outside3_is, same_bits, twice

pytestmark = pytest.mark.gpu

# Worst excess of |got - total| over the other terms of the bound across every case of test_random_per_element (56 launches),
# test_score_offset (20) and test_eps_and_tiny_rows (8), measured on an MI355X (run this file with -s: every case prints its own
# excess): 0.0 in every case. Worst err/bound per test, same run: test_random_per_element 0.969 (bf16 o under accumulate, where the
# store's own rounding 2^-8 |total| is most of the bound; 0.795 among the fp32-o cases, where the P term is), test_score_offset 0.408
# (E_s up to 1.03e-3), test_eps_and_tiny_rows 0.667, test_one_hot_exact_forms' accumulate check 0.996 with bf16 o (a store that rounds
# by half an ulp at the bottom of a binade: 2^-8 |total| is attained, not exceeded) and 0.891 with fp32 o. With nothing measured to
# multiply by 4, the slack is 2^-20 max|c v| of the case's data (2.2e-6 ... 4.4e-5).
MEASURED_EXCESS = 0.0


def ip_slack(cvmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * cvmax


B, H, DH = 2, 2, 128
D = H * DH
SM = 128 ** -0.5                    # the kernel's default softmax scale
LOG2E = 1.4426950408889634
Q_MARGIN = 2.0 ** -18               # no fp64 q^ closer than this (relative) to a bf16 midpoint
VALUES = (0.25, 1.0, -1.5, 3.0)     # row weights: fractional, one, negative, above one


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


# ------------------------------------------------------------------------------------------------------------------------- data
def settle_q(q, wq, eps, what):
    """q [B, N, H, 128] bf16 with one bf16 ulp added (in magnitude) to every raw element whose fp64 q^ lies within Q_MARGIN of a bf16
    midpoint, repeated until none is left (a changed element moves its row's mean square, hence the loop). Asserts that this takes at
    most 10 rounds and changes fewer than 1 % of the elements."""
    q = q.clone()
    changed = torch.zeros(q.shape, dtype=torch.bool)
    for rounds in range(11):
        _, margin = bf16_round64(ip_qhat64(q, wq, eps))
        off = margin < Q_MARGIN
        if not off.any():
            break
        assert rounds < 10, f"{what}: {int(off.sum())} elements of q^ still within 2^-18 of a bf16 midpoint after 10 rounds"
        qi = q.view(torch.int16)
        qi[off] += 1                                  # sign-magnitude: the next bf16 value away from zero
        changed |= off
    share = float(changed.float().mean())
    print(f"[ip-edges] {what}: q settled in {rounds} rounds, {int(changed.sum())} of {q.numel()} elements changed")
    assert share < 0.01, f"{what}: {share:.2%} of the q elements nudged"
    assert bool(torch.isfinite(q.float()).all())
    return q


def random_q(N, g):
    """The distribution of the existing tests: N(0, 1) times a magnitude 0.1 .. 10 per row."""
    return (torch.randn(B, N, H, DH, generator=g) * 10.0 ** (torch.rand(B, N, 1, 1, generator=g) * 2.0 - 1.0)).to(BF16)


def random_wq(g):
    return (torch.rand(DH, generator=g) + 0.5).to(BF16)


def row_weights(N, entries, g):
    """[entries, N] fp32: VALUES in turn, about one row in five 0, row 0 never (N = 1 keeps its row)."""
    rows = torch.arange(N)
    w = torch.stack([torch.tensor(VALUES)[(rows + e) % 4] for e in range(entries)])
    w[torch.rand(entries, N, generator=g) < 0.2] = 0.0
    w[:, 0] = VALUES[2]
    return w


def scale_c(ip_scale, w, gate, N):
    """c [B, N, D] fp64 = fp32(ip_scale) x row weight x gate from the fp32 values the kernel reads; absent factors are 1."""
    c = torch.full((B, N, D), float(torch.tensor(ip_scale, dtype=F32)), dtype=F64)
    if w is not None:
        c = c * w.double().expand(B, N)[:, :, None]
    if gate is not None:
        c = c * gate.double()[:, None, :]
    return c


# ------------------------------------------------------------------------------------------------------------ launch and checks
def launch(ops, gpu, what, q, wq, k, v, *, o_f32, accumulate=False, gate=None, w=None, ip_scale=1.0, eps=1e-6, old_seed=0):
    """One guarded launch, twice. CPU tensors in: q [B, N, H, 128] bf16, k / v [B or 1, n, H, 128] bf16, gate [B, D] fp32 or None,
    w [B or 1, N] fp32 or None. Returns (got, old): the [B, N, D] output and (accumulate) the prior contents, on the CPU."""
    N, Bk, n = q.shape[1], k.shape[0], k.shape[1]
    odt = F32 if o_f32 else BF16
    qbuf = torch.full((B, N + 3, 7 * D), NAN, dtype=BF16)
    qbuf[:, :N, 2 * D : 3 * D] = q.reshape(B, N, D)
    kvbuf = torch.full((Bk, n + 3, 2 * D + 64), NAN, dtype=BF16)
    kvbuf[:, :n, :D], kvbuf[:, :n, D : 2 * D] = k.reshape(Bk, n, D), v.reshape(Bk, n, D)
    obuf0 = torch.full((B, N + 3, D + 16), SENT, dtype=odt)
    old = None
    if accumulate:
        old = (torch.randn(B, N, D, generator=torch.Generator().manual_seed(old_seed)) * 0.5).to(odt)
        obuf0[:, :N, :D] = old
    inputs = [qbuf.to(gpu), kvbuf.to(gpu), wq.to(gpu)]
    qd, kd, vd, wqd = inputs[0][:, :N, 2 * D : 3 * D], inputs[1][:, :n, :D], inputs[1][:, :n, D : 2 * D], inputs[2]
    gd = wd = None
    if gate is not None:
        gbuf = torch.full((B, 6 * D), NAN, dtype=F32)
        gbuf[:, 2 * D : 3 * D] = gate
        inputs.append(gbuf.to(gpu))
        gd = inputs[-1][:, 2 * D : 3 * D]
    if w is not None:
        wbuf = torch.full((w.shape[0], N + 8), NAN, dtype=F32)
        wbuf[:, 4 : 4 + N] = w
        inputs.append(wbuf.to(gpu))
        wd = inputs[-1][:, 4 : 4 + N]
    before = [t.clone() for t in inputs]

    def run():
        od = obuf0.to(gpu, copy=True)
        if gd is None:
            ops.ip_attention(qd, wqd, kd, vd, od[:, :N, :D], H, ip_scale=ip_scale, accumulate=accumulate, eps=eps, row_weights=wd)
        else:
            ops.ip_attention_gated(qd, wqd, kd, vd, od[:, :N, :D], H, ip_scale=ip_scale, gate=gd, accumulate=accumulate, eps=eps,
                                   row_weights=wd)
        torch.cuda.synchronize()
        return od

    od = twice(run)
    assert outside3_is(od, N, D, SENT), f"{what}: wrote outside [:N, :d] of the output"
    for t, t0 in zip(inputs, before):
        assert same_bits(t, t0), f"{what}: the kernel wrote to its inputs"
    return od[:, :N, :D].cpu(), old


def check_term(what, got, old, ref, c, v, o_f32, rows=None):
    """The per-element bound of the header over the rows selected by `rows` ([B, N] bool; None: all). ref = (term, pv, E_s) of
    ip_attention_ref64. Prints the part of the error that the slack has to carry before it asserts; returns (err/bound, excess)."""
    term, pv, e_s = ref
    N = term.shape[1]
    assert float(e_s.max()) < 0.01, f"{what}: E_s {float(e_s.max()):.3e}: the first-order score term does not hold"
    es = e_s.repeat_interleave(DH, dim=2)                                       # [B, N, H] -> [B, N, D]
    total = term if old is None else term + old.double()
    base = 2.0 ** -8 * pv + 2 * es * pv
    if not o_f32:
        base = base + 2.0 ** -8 * total.abs()
    if old is not None:
        base = base + 3 * 2.0 ** -24 * (term.abs() + old.double().abs())
    vd = v.double().reshape(v.shape[0], -1, D)
    slack = ip_slack(float((c.abs().amax(1) * vd.abs().amax(1)).max()))
    sel = torch.ones(B, N, dtype=torch.bool) if rows is None else rows
    g, t, b = got.double()[sel], total[sel], base[sel]
    excess = float(((g - t).abs() - b).max())
    print(f"[ip-edges] {what}: excess over the bound without slack {max(excess, 0.0):.3e} (slack {slack:.3e}, max E_s {float(e_s.max()):.2e})")
    return check_bound(what, g, t, b + slack), excess


# ----------------------------------------------------------------------------------------------------- 1. random data, per element
# (N, n_ip, fp32 o, accumulate, gate, row weights, shared k / v). n_ip covers the KB = 1 .. 4 edges and the switch from 128-row to
# 256-row workgroups (n_ip > 96); every N meets both workgroup sizes; every pair of the five switches appears in all four combinations
# (the first eight rows are an orthogonal array: a, b, c, a ^ b, a ^ c). check_table asserts all of this.
CASES = [
    (1, 1, 0, 0, 0, 0, 0),
    (17, 31, 0, 0, 1, 0, 1),
    (129, 32, 0, 1, 0, 1, 0),
    (257, 33, 0, 1, 1, 1, 1),
    (300, 64, 1, 0, 0, 1, 1),
    (1, 97, 1, 0, 1, 1, 0),
    (17, 128, 1, 1, 0, 0, 1),
    (129, 127, 1, 1, 1, 0, 0),
    (257, 97, 0, 0, 0, 1, 1),
    (300, 128, 0, 1, 1, 0, 0),
    (300, 65, 1, 0, 1, 0, 1),
    (129, 96, 1, 1, 0, 1, 0),
    (300, 127, 1, 1, 1, 1, 1),
    (257, 1, 0, 0, 1, 1, 0),
]


def check_table():
    assert {c[1] for c in CASES} == {1, 31, 32, 33, 64, 65, 96, 97, 127, 128}
    assert {(c[0], c[1] > 96) for c in CASES} == {(N, big) for N in (1, 17, 129, 257, 300) for big in (False, True)}
    for i in range(2, 7):
        for j in range(i + 1, 7):
            assert {(c[i], c[j]) for c in CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (i, j)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "N{}-n{}-f32{}-acc{}-gate{}-rows{}-shared{}".format(*CASES[i]))
def test_random_per_element(ops, gpu, idx):
    """One row of CASES: the existing tests' q distribution (settled), ip_scale 0.7 / -1.3 in turn, two key scales x two value regimes."""
    check_table()
    N, n_ip, o_f32, accumulate, gated, weighted, shared = CASES[idx]
    ip_scale = -1.3 if idx % 2 else 0.7
    g = torch.Generator().manual_seed(31200 + idx)     # with base 31000 one element of case 4 walks along midpoints for 10 rounds
    tag = f"random N={N} n_ip={n_ip} f32={o_f32} acc={accumulate} gate={gated} rows={weighted} shared={shared}"
    wq = random_wq(g)
    q = settle_q(random_q(N, g), wq, 1e-6, tag)
    Bk = 1 if shared else B
    gate = torch.randn(B, D, generator=g) if gated else None
    w = row_weights(N, B if idx % 4 < 2 else 1, g) if weighted else None
    c = scale_c(ip_scale, w, gate, N)
    zero = torch.zeros(B, N, dtype=torch.bool) if w is None else (w == 0).expand(B, N)
    assert int(zero.sum()) * 2 <= B * N, tag
    for kstd in (1.5, 6.0):                         # the existing score regime; a sharp softmax, where a truncated q^ shows
        k = (torch.randn(Bk, n_ip, H, DH, generator=g) * kstd).to(BF16)
        for positive in (False, True):              # v ~ N(0, 1); v = 0.5 + |N(0, 1)|: no cancellation, pv = |term|
            v = torch.randn(Bk, n_ip, H, DH, generator=g)
            v = (0.5 + v.abs() if positive else v).to(BF16)
            what = f"{tag} kstd={kstd} v{'>0' if positive else '~N'}"
            got, old = launch(ops, gpu, what, q, wq, k, v, o_f32=o_f32, accumulate=accumulate, gate=gate, w=w, ip_scale=ip_scale,
                              old_seed=idx)
            check_term(what, got, old, ip_attention_ref64(q, wq, k, v, c, SM, 1e-6), c, v, o_f32, rows=~zero)
            if zero.any():                          # rows worth nothing: bytes untouched under accumulate, +0 otherwise
                if accumulate:
                    assert same_bits(got[zero], old[zero]), what
                else:
                    assert same_bits(got[zero], torch.zeros_like(got[zero])), what


# ------------------------------------------------------------------------------------------- 2. every real score far from 0
@pytest.mark.parametrize("o_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("n_ip", [31, 33, 97, 127, 128])
def test_score_offset(ops, gpu, n_ip, o_f32):
    """Every query row is one direction u plus 0.3 noise, every key +-t u plus noise, t chosen so that all scaled scores lie in
    [100, 140] (exp2 without the row maximum overflows) or in [-140, -100] (a padded key let through, score 0, would own the softmax,
    and without the maximum the row is 0 / 0)."""
    N = 129
    g = torch.Generator().manual_seed(32000 + n_ip)
    wq = random_wq(g)
    u = torch.where(torch.rand(DH, generator=g) < 0.5, -1.0, 1.0)
    tag = f"offset n_ip={n_ip} f32={o_f32}"
    q = settle_q((u + 0.3 * torch.randn(B, N, H, DH, generator=g)).to(BF16), wq, 1e-6, tag)
    qh, _ = bf16_round64(ip_qhat64(q, wq, 1e-6))
    t = 120.0 / float(((qh * u.double()).sum(-1) * SM).median())                 # the median row's score against t u is 120
    noise = torch.randn(B, n_ip, H, DH, generator=g)
    v = torch.randn(B, n_ip, H, DH, generator=g).to(BF16)
    c = scale_c(0.7, None, None, N)
    for sign in (1.0, -1.0):
        k = (sign * t * u + noise).to(BF16)
        s = torch.einsum("bqhd,bkhd->bhqk", qh, k.double()) * SM * sign
        print(f"[ip-edges] {tag} sign {sign:+.0f}: t = {t:.3f}, scaled scores {sign * float(s.min()):.1f} .. {sign * float(s.max()):.1f}")
        assert 100.0 <= float(s.min()) and float(s.max()) <= 140.0, (tag, sign)
        what = f"{tag} sign {sign:+.0f}"
        got, _ = launch(ops, gpu, what, q, wq, k, v, o_f32=o_f32, ip_scale=0.7)
        check_term(what, got, None, ip_attention_ref64(q, wq, k, v, c, SM, 1e-6), c, v, o_f32)


# ------------------------------------------------------------------------------------------------- 3. eps and rows near it
@pytest.mark.parametrize("eps", [1e-6, 1e-3])
@pytest.mark.parametrize("o_f32", [False, True], ids=["bf16", "f32"])
def test_eps_and_tiny_rows(ops, gpu, o_f32, eps):
    """Rows 0 .. 15 all zero (only eps stands between the output and NaN: the expected term is c times the mean of v), rows 16 .. 31
    scaled by 2^-10 (mean(q^2) ~ 1e-6), rows 32 .. 47 by 2^-14, the rest of unit scale; eps goes through ops and into the reference."""
    N, n_ip = 64, 33
    g = torch.Generator().manual_seed(33000)
    wq = random_wq(g)
    q = torch.randn(B, N, H, DH, generator=g)
    q[:, :16] = 0.0
    q[:, 16:32] *= 2.0 ** -10
    q[:, 32:48] *= 2.0 ** -14
    tag = f"eps={eps:g} f32={o_f32}"
    q = settle_q(q.to(BF16), wq, eps, tag)
    assert not q[:, :16].any()
    k = (torch.randn(B, n_ip, H, DH, generator=g) * 3.0).to(BF16)      # score std ~3: the length of q^ decides how sharp the row is
    v = torch.randn(B, n_ip, H, DH, generator=g).to(BF16)
    c = scale_c(0.7, None, None, N)
    ref = ip_attention_ref64(q, wq, k, v, c, SM, eps)
    term, pv, e_s = ref
    mean_v = c[:, :16] * v.double().mean(1).reshape(B, 1, D)
    assert float((term[:, :16] - mean_v).abs().max()) < 1e-12                    # the reference itself: a zero row is the mean of v

    # a reference without eps must be far outside the bound on the tiny rows, or the comparison below could not tell
    wrong = ip_attention_ref64(q[:, 16:48], wq, k, v, c[:, 16:48], SM, 0.0)[0]
    bound = 2.0 ** -8 * pv + 2 * e_s.repeat_interleave(DH, dim=2) * pv + (0.0 if o_f32 else 2.0 ** -8 * term.abs())
    bound = bound + ip_slack(float((c.abs().amax(1) * v.double().reshape(B, n_ip, D).abs().amax(1)).max()))
    far = float(((wrong - term[:, 16:48]).abs() > 10 * bound[:, 16:48]).double().mean())
    print(f"[ip-edges] {tag}: the eps = 0 reference is more than 10 x the bound away in {far:.1%} of the tiny rows' elements")
    assert far >= 0.5, (tag, far)

    got, _ = launch(ops, gpu, tag, q, wq, k, v, o_f32=o_f32, ip_scale=0.7, eps=eps)
    assert bool(torch.isfinite(got.float()).all()), tag
    check_term(tag, got, None, ref, c, v, o_f32)
    check_term(f"{tag} zero rows vs mean(v)", got[:, :16], None, (mean_v, pv[:, :16], e_s[:, :16]), c[:, :16], v, o_f32)


# ------------------------------------------------------------------------------------------------------- 4. one-hot rows, exact
def hadamard128():
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < 128:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


@pytest.mark.parametrize("n_ip", [1, 33, 100, 128])
def test_one_hot_exact_forms(ops, gpu, n_ip):
    """Keys 16 x Hadamard rows, query row i a power of two times Hadamard row i % n_ip: that key wins by more than 180 log2 units,
    every other numerator is exactly 0, the row sum exactly 1.0f and the second product returns v_j exactly. Write mode is then
    fl(fl(v_j fl(ip_scale w)) gate) bit for bit (bf16: its round-to-nearest-even) at every key position and output column: the V^T row
    permutation, the P fragment order and the column layout. Accumulate may fuse the last product with the sum, so it is held to
    3 x 2^-24 (|c v_j| + |old|) (+ 2^-8 |total| for bf16) instead."""
    N = 300
    g = torch.Generator().manual_seed(34000 + n_ip)
    had = hadamard128()
    win = torch.arange(N) % n_ip
    e = torch.randint(-3, 4, (B, N, 1, 1), generator=g).double()
    q = (torch.exp2(e) * had[win][None, :, None, :]).expand(B, N, H, DH).to(BF16)
    k = (16.0 * had[:n_ip])[None, :, None, :].expand(B, n_ip, H, DH).to(BF16).contiguous()
    wq = random_wq(g)
    v = torch.randn(B, n_ip, H, DH, generator=g).to(BF16)
    qh, _ = bf16_round64(ip_qhat64(q, wq, 1e-6))
    s = torch.einsum("bqhd,bkhd->bhqk", qh, k.double()) * SM * LOG2E               # log2 units, [B, H, N, n_ip]
    assert bool((s.argmax(-1) == win).all())
    if n_ip > 1:
        top = s.topk(2, dim=-1).values
        gap = float((top[..., 0] - top[..., 1]).min())
        print(f"[ip-edges] one-hot n_ip={n_ip}: smallest gap to the runner-up {gap:.1f} log2 units")
        assert gap > 180.0, gap
    vj = v.reshape(B, n_ip, D)[:, win].float()                                   # [B, N, D]: the value row each query row returns
    gate = torch.randn(B, D, generator=g)
    w = torch.tensor(VALUES)[(torch.arange(N)[None, :] + torch.arange(B)[:, None]) % 4].contiguous()
    ipf = torch.tensor(-1.3, dtype=F32)
    for gated in (False, True):
        for weighted in (False, True):
            scale = (ipf * w if weighted else ipf.expand(B, N))[:, :, None]      # fl(ip_scale w), fp32
            want = vj * scale
            if gated:
                want = want * gate[:, None, :]
            cv = vj.double() * scale_c(-1.3, w if weighted else None, gate if gated else None, N)
            for o_f32 in (False, True):
                what = f"one-hot n_ip={n_ip} gate={gated} rows={weighted} f32={o_f32}"
                kw = dict(o_f32=o_f32, gate=gate if gated else None, w=w if weighted else None, ip_scale=-1.3)
                got, _ = launch(ops, gpu, what, q, wq, k, v, **kw)
                assert same_bits(got, want if o_f32 else want.to(BF16)), f"{what}: write mode is not fl(fl(v_j fl(ip_scale w)) gate)"
                got, old = launch(ops, gpu, what + " acc", q, wq, k, v, accumulate=True, old_seed=n_ip, **kw)
                total = cv + old.double()
                bound = 3 * 2.0 ** -24 * (cv.abs() + old.double().abs()) + (0.0 if o_f32 else 2.0 ** -8 * total.abs())
                check_bound(what + " acc", got, total, bound)
