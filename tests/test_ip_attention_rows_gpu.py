"""GPU tests of rt_ip_attention_rows: rt_ip_attention_gated with an fp32 weight per query row. The weight is multiplied into ip_scale
in fp32; a row of weight 0 is selected out (accumulate: bytes untouched, write: +0, its q row reaches no output); tiles and workgroups
of such rows are skipped. Buffers are guarded as in test_ip_adapter_gpu.py: q inside a wider row, canary rows and columns around o."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instantx_reference as ixr  # noqa: E402

KERNEL_BOUND = 5e-3            # the bound test_ip_attention_kernel_matches_fp32 holds rt_ip_attention to
H_K, B_K = 2, 2
D_K = H_K * 128
VALUES = (0.25, 1.0, -1.5, 3.0)
# A wave walks the tiles 64 rows apart (tile `it` of wave w starts at row 64·it + 16·w of the workgroup), so alternate TILES leave every
# wave with all of its tiles on or all off; alternate 64-row GROUPS, in both phases, are what makes a wave skip a tile and compute the
# next one (whose rows the skipped tile must still have put in flight) and the other way round.
PATTERNS = ("ones", "zeros", "first_wg_zero", "alternate_tiles", "alternate_groups", "alternate_groups_odd", "mixed_in_tile", "values")

# (N, n_ip, fp32 o, accumulate, gated, per-entry table). Every N of {1, 16, 17, 127, 129, 257, 300} (the tile edge, the edge of a
# 128-row and of a 256-row workgroup) meets both workgroup sizes (n_ip <= 96: 128 rows, TILES = 2; n_ip = 100, 128: 256 rows, TILES = 4);
# every n_ip of {1, 33, 100, 128} (KB = 1, 2, 4) meets both o dtypes, both modes, both gate settings and both table forms; every pair
# of the four switches appears in all four combinations.
CASES = [
    (1, 1, False, False, False, False),
    (1, 128, True, True, True, True),
    (16, 33, False, True, True, False),
    (16, 100, True, False, False, True),
    (17, 1, True, True, False, True),
    (17, 128, False, False, True, False),
    (127, 33, True, False, True, True),
    (127, 100, False, True, False, False),
    (129, 1, False, False, True, True),
    (129, 128, True, True, False, False),
    (257, 33, True, True, True, False),
    (257, 100, False, False, False, True),
    (300, 1, True, False, True, False),
    (300, 33, False, True, False, True),
    (300, 100, True, True, True, True),
    (300, 128, False, False, False, False),
    (257, 128, False, True, True, True),
    (129, 100, True, False, True, False),
    (127, 1, False, True, False, False),
    (300, 33, True, False, False, True),
]


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def weight_table(pattern, N, wg, entries, seed):
    """[entries, N] fp32, built per 16-row tile and per workgroup of `wg` rows; entry 1 of a per-entry table is another draw."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(VALUES)
    rows = torch.arange(N)
    out = []
    for e in range(entries):
        cyc = vals[(rows + e) % 4]
        if pattern == "ones":
            w = torch.ones(N)
        elif pattern == "zeros":
            w = torch.zeros(N)
        elif pattern == "values":
            w = cyc.clone()
        elif pattern == "alternate_tiles":
            w = torch.where((rows // 16 + e) % 2 == 0, torch.zeros(N), cyc)
        elif pattern.startswith("alternate_groups"):
            w = torch.where((rows // 64 + e + pattern.endswith("odd")) % 2 == 0, torch.zeros(N), cyc)
        elif pattern == "mixed_in_tile":
            w = torch.where(torch.rand(N, generator=g) < 0.5, torch.zeros(N), cyc)
        elif pattern == "first_wg_zero":
            w = torch.where(torch.rand(N, generator=g) < 0.4, torch.zeros(N), cyc)
            w[:wg] = 0.0
        out.append(w)
    return torch.stack(out)


def _inputs(N, n_ip, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16)
    q = bf(torch.randn(B_K, N, H_K, 128, generator=g) * 10.0 ** (torch.rand(B_K, N, 1, 1, generator=g) * 2.0 - 1.0))
    wq = bf(torch.rand(128, generator=g) + 0.5)
    k = bf(torch.randn(B_K, n_ip, H_K, 128, generator=g) * 1.5)
    v = bf(torch.randn(B_K, n_ip, H_K, 128, generator=g))
    table = torch.randn(B_K, 6 * D_K, generator=g)
    return g, q, wq, k, v, table


@pytest.mark.parametrize("N, n_ip, o_f32, accumulate, gated, per_entry", CASES)
def test_weighted_kernel(gpu, N, n_ip, o_f32, accumulate, gated, per_entry):
    from reptext_amd import ops

    d = D_K
    wg = 256 if n_ip > 96 else 128
    g, q, wq, k, v, table = _inputs(N, n_ip, 7000 * n_ip + N)
    gate = table[:, 2 * d : 3 * d] if gated else None
    ip_scale = -1.3 if (N + n_ip) % 2 else 0.7
    ref = ixr.ip_attention_gated_ref(q, wq, k, v, ip_scale, gate)              # the unweighted term, once per case
    odt = torch.float32 if o_f32 else torch.bfloat16
    qbuf = torch.randn(B_K, N, 7 * d, generator=g).to(torch.bfloat16)
    qbuf[..., 2 * d : 3 * d] = q.reshape(B_K, N, d)
    qdev = qbuf.to(gpu)
    ldo, rows_o = d + 16, N + 3
    obuf0 = (torch.randn(B_K, rows_o, ldo, generator=g) * 0.5).to(odt)
    wqd, kd, vd = wq.to(gpu), k.reshape(B_K, n_ip, d).to(gpu), v.reshape(B_K, n_ip, d).to(gpu)
    gd = table.to(gpu)[:, 2 * d : 3 * d] if gated else None

    def launch(qd, obuf, w, sl=slice(None)):
        """A fresh copy of obuf on the device, one launch over batch entries `sl`, the whole guarded buffer back on the host."""
        od = obuf[sl].to(gpu)
        wd = None if w is None else (w if w.shape[0] == 1 else w[sl]).to(gpu)
        ops.ip_attention_gated(qd[sl][..., 2 * d : 3 * d], wqd, kd[sl], vd[sl], od[:, :N, :d], H_K, ip_scale=ip_scale,
                               gate=None if gd is None else gd[sl], accumulate=accumulate, row_weights=wd)
        torch.cuda.synchronize()
        return od.cpu()

    for pattern in PATTERNS:
        tag = f"N={N} n_ip={n_ip} f32={o_f32} acc={accumulate} gated={gated} per_entry={per_entry} pattern={pattern}"
        w = weight_table(pattern, N, wg, B_K if per_entry else 1, seed=N + n_ip)
        wb = w.expand(B_K, N)
        zero = wb == 0
        obuf = obuf0.clone()
        if accumulate:      # -0.0 and NaN bit patterns in the prior contents of zero-weight rows: they must keep their bits
            inner = obuf[:, :N, :d]
            inner[zero & (torch.arange(N) % 3 == 0)] = -0.0
            nan = (torch.tensor([0x7FC00123], dtype=torch.int32) if o_f32 else torch.tensor([0x7FC1], dtype=torch.int16)).view(odt)
            inner[zero & (torch.arange(N) % 3 == 1)] = nan
        out = launch(qdev, obuf, w)

        # 6. canaries, q unmodified, a second launch gives the same bits
        assert torch.equal(bits(out[:, N:]), bits(obuf[:, N:])) and torch.equal(bits(out[:, :, d:]), bits(obuf[:, :, d:])), tag
        assert torch.equal(qdev.cpu(), qbuf), tag
        assert torch.equal(bits(launch(qdev, obuf, w)), bits(out)), tag
        got, old = out[:, :N, :d], obuf[:, :N, :d]
        # 1. a table of ones is the launch without a table
        if pattern == "ones":
            assert torch.equal(bits(out), bits(launch(qdev, obuf, None))), tag
        # 2. rows worth something: the fp32 term times w (plus the old contents)
        if (~zero).any():
            want = ref * wb[..., None] + (old.float() if accumulate else 0.0)
            err = rel_l2(got.float()[~zero], want[~zero])
            print(f"{tag}: rel_l2 over {int((~zero).sum())} weighted rows {err:.3e}")
            assert err < KERNEL_BOUND, (tag, err)
        # 3. / 4. rows worth nothing: untouched bytes when accumulating, +0 when writing
        if zero.any():
            if accumulate:
                assert torch.equal(bits(got)[zero], bits(old)[zero]), tag
            else:
                assert not bits(got)[zero].any(), tag
            # 5. NaN and Inf in the q rows of zero-weight rows (whole skipped tiles and rows inside computed tiles) change nothing
            qpois = qbuf.clone()
            qv = qpois[..., 2 * d : 3 * d]
            qv[zero & (torch.arange(N) % 2 == 0)] = float("nan")
            qv[zero & (torch.arange(N) % 2 == 1)] = float("inf")
            assert torch.equal(bits(launch(qpois.to(gpu), obuf, w)), bits(out)), tag
        # 7. entry b of the batched launch is its own batch-1 launch
        for b in range(B_K):
            assert torch.equal(bits(launch(qdev, obuf, w, slice(b, b + 1))), bits(out[b : b + 1])), (tag, b)


def test_rows_entry_rejects_bad_arguments_on_real_buffers(gpu):
    from reptext_amd import native, ops

    lib = native.load()
    d = D_K
    q = torch.zeros(1, 64, 7 * d, device=gpu, dtype=torch.bfloat16)
    wq = torch.ones(128, device=gpu, dtype=torch.bfloat16)
    o = torch.zeros(1, 64, d, device=gpu, dtype=torch.bfloat16)
    K = torch.ones(1, 4, d, device=gpu, dtype=torch.bfloat16)
    gate = torch.ones(1, 6 * d, device=gpu)
    w = torch.ones(1, 64 + 4, device=gpu)
    qv = q[..., 2 * d : 3 * d]
    with pytest.raises(ValueError, match="row_weights must be"):
        ops.ip_attention_gated(qv, wq, K, K, o, H_K, row_weights=w)                         # 68 columns for 64 rows
    with pytest.raises(ValueError, match="row_weights must be"):
        ops.ip_attention_gated(qv, wq, K, K, o, H_K, row_weights=w[:, :64].expand(2, 64))
    with pytest.raises(ValueError, match="row_weights must be"):
        ops.ip_attention_gated(qv, wq, K, K, o, H_K, row_weights=torch.ones(1, 128, device=gpu)[:, ::2])   # inner stride 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ip_attention_gated(qv, wq, K, K, o, H_K, row_weights=w[:, :64].cpu())

    def call(w_ptr=w.data_ptr(), swb=0, gate_ptr=None, sgb=0, n_ip=4, ldq=7 * d, N=64):
        return lib.rt_ip_attention_rows(qv.data_ptr(), ldq, 0, wq.data_ptr(), K.data_ptr(), K.data_ptr(), d, 0, gate_ptr, sgb, w_ptr, swb,
                                        o.data_ptr(), d, 0, 0, 0, 1, N, H_K, n_ip, 128 ** -0.5, 1.0, 1e-6, None)

    assert call(w_ptr=None) == -1 and call(swb=-1) == -1                                                # RT_E_BADARG: its own
    assert call(n_ip=0) == -1 and call(N=0) == -1 and call(ldq=128) == -1                               # ... and the gated entry's
    assert call(gate_ptr=gate.data_ptr(), sgb=-4) == -1
    assert call(n_ip=129) == -3                                                                         # RT_E_SHAPE
    assert call(w_ptr=w.data_ptr() + 2) == -2                                                           # RT_E_ALIGN: its own
    assert call(gate_ptr=gate.data_ptr() + 4, sgb=6 * d) == -2 and call(ldq=7 * d + 4) == -2            # ... and the gated entry's
    torch.cuda.synchronize()
    assert not o.any()                                                                                  # nothing was launched
    assert call(w_ptr=w.data_ptr() + 4, swb=3) == 0                                                     # 4-byte alignment and any stride >= 0 are enough
    torch.cuda.synchronize()
    assert o.any()
