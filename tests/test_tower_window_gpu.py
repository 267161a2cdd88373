"""The ControlNet tower on the active row window of its regional mask: attention for a range of the query rows inside
the full launch's cut (rt_attention_fwd_rows) against the fp32 oracle and against the whole launch, the windowed tower against the full
path, and the pipeline around both.

Tolerances: against the fp32 oracle the bound of test_kernels_gpu.test_attention (P rounded to bf16 before P·V, the output once more:
rel-L2 < 5e-3). Everything else is compared bitwise: GEMM, LayerNorm and zero-linear results do not depend on the tile that computes a
row, and the ranged attention launch is cut exactly as the whole launch is."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402

BF16 = torch.bfloat16
SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_single_layers=0, extra_condition_channels=64)
T, N, GRID = 64, 256, 16


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf16r(x):
    return x.to(BF16).to(torch.float32)


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


@pytest.fixture()
def attention_hip_only(gpu):
    """rt_attention_variant(0): csrc/attention.hip serves every full launch too, so full and windowed launches share one kernel."""
    from reptext_amd import native

    lib = native.load()
    prev = lib.rt_attention_variant(0)
    yield lib
    lib.rt_attention_variant(prev)


def _qkv(B, S, H, seed):
    d = H * 128
    qkv = bf16r(torch.randn(B, S, 3 * d, generator=torch.Generator().manual_seed(seed)))
    qkv[..., :d] *= 2.0                      # sharper softmax than N(0,1) scores
    return qkv


def _oracle_window(qkv, H, r0, r1):
    B, S, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (qkv[..., i * d : (i + 1) * d].reshape(B, S, H, 128) for i in range(3))
    return orc.attention(q[:, r0:r1], k, v)


# B, H, S, (r0, r1): the issue's two window cases (ragged in both dimensions; few items at offset 256), batch 2 with many heads, a window
# inside one wave's rows with a ragged key tile
WINDOW_CASES = [(1, 3, 320, (64, 200)), (1, 2, 1024, (256, 384)), (2, 24, 1152, (512, 768)), (1, 2, 200, (96, 128))]


@pytest.mark.parametrize("B,H,S,win", WINDOW_CASES)
def test_window_attention_against_the_oracle(ops, gpu, B, H, S, win):
    """Attention for the window's rows (ops.attention(rows=...)) against the fp32 oracle restricted to the window, at the bound of
    test_kernels_gpu.test_attention; repeatable; with the output over q. All rows as the range is the whole launch."""
    r0, r1 = win
    d = H * 128
    qkv = _qkv(B, S, H, S + H)
    ref = _oracle_window(qkv, H, r0, r1)
    dq = qkv.to(gpu, BF16)
    q, k, v = dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :]
    out = torch.zeros(B, S, d, device=gpu, dtype=BF16)
    ops.attention(q, k, v, out, H, rows=win)
    err = rel_l2(out[:, r0:r1].float().cpu(), ref)
    print(f"window attention B={B} H={H} S={S} window=[{r0},{r1}): rel-L2 vs fp32 oracle {err:.3e}")
    assert err < 5e-3
    again = torch.zeros_like(out)
    ops.attention(q, k, v, again, H, rows=win)
    assert torch.equal(again, out)
    full = torch.empty_like(out)
    ops.attention(q, k, v, full, H)
    allrows = torch.empty_like(out)
    ops.attention(q, k, v, allrows, H, rows=(0, S))
    assert torch.equal(allrows, full)
    inplace = dq.clone()
    ops.attention(inplace[..., :d], inplace[..., d : 2 * d], inplace[..., 2 * d :], inplace[..., :d], H, rows=win)
    assert torch.equal(inplace[:, r0:r1, :d], out[:, r0:r1]) and torch.equal(inplace[..., d:], dq[..., d:])


# B, S, H, (r0, r1): attention.hip unsplit / attention.hip at a ragged S / attention_v3 with its key split (the headline launch, a
# window that starts and ends inside items) / attention_v3, a window of one row / batch 2
ROWS_CASES = [(1, 320, 3, (64, 200)), (2, 700, 3, (130, 131)), (1, 4608, 24, (960, 1312)), (1, 1536, 24, (1535, 1536)), (2, 2304, 8, (0, 300))]


@pytest.mark.parametrize("B,S,H,rows", ROWS_CASES)
def test_attention_rows_are_the_full_launch_rows(ops, gpu, B, S, H, rows):
    """rt_attention_fwd_rows: the full launch's cut in which only the items that hold a row of the range work. The range's rows are
    bitwise those of the whole launch, whichever kernel and key split serve the shape; rows of untouched items are not written; the
    ticket counters are left at rest (a whole launch afterwards repeats its bits); in place over q."""
    r0, r1 = rows
    d = H * 128
    dq = _qkv(B, S, H, S + H).to(gpu, BF16)
    q, k, v = dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :]
    full = torch.empty(B, S, d, device=gpu, dtype=BF16)
    ops.attention(q, k, v, full, H)
    out = torch.full((B, S, d), 7.0, device=gpu, dtype=BF16)
    ops.attention(q, k, v, out, H, rows=rows)
    assert torch.equal(out[:, r0:r1], full[:, r0:r1])
    lo, hi = r0 // 256 * 256, min(S, (r1 + 255) // 256 * 256)                  # items are 128 or 256 rows: nothing beyond the 256-row cover
    assert bool((out[:, :lo] == 7.0).all()) and bool((out[:, hi:] == 7.0).all())
    written = out[:, lo:hi] != 7.0
    assert torch.equal(out[:, lo:hi][written], full[:, lo:hi][written])       # what else was written is the whole launch's value too
    again = torch.empty_like(full)
    ops.attention(q, k, v, again, H)
    assert torch.equal(again, full)
    inplace = dq.clone()
    ops.attention(inplace[..., :d], inplace[..., d : 2 * d], inplace[..., 2 * d :], inplace[..., :d], H, rows=rows)
    assert torch.equal(inplace[:, r0:r1, :d], full[:, r0:r1]) and torch.equal(inplace[..., d:], dq[..., d:])
    with pytest.raises(Exception):
        ops.attention(q, k, v, out, H, rows=(r1, r0))


# ------------------------------------------------------------------------------------------- the tower
def _box_rowscale(boxes, batch=None):
    """f32 row scales [N] (or [batch, N], one box per entry) of grid boxes (r0, r1, c0, c1), with fractional values on the edges."""
    out = []
    for r0, r1, c0, c1 in boxes:
        m = torch.zeros(GRID, GRID)
        m[r0:r1, c0:c1] = 1.0
        m[r0, c0:c1] = 0.25
        m[r1 - 1, c0:c1] = 0.625
        out.append(m.reshape(-1))
    return out[0] if batch is None else torch.stack(out)


def _tower(gpu, seed):
    from reptext_amd.controlnet import FluxControlNetModel

    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    cn.load_state_dict(orc.init_mmdit_params(SMALL_CN, seed, controlnet=True))
    return cn


def _tower_inputs(gpu, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, BF16)
    return dict(hidden_states=r(B, N, 64), encoder_hidden_states=r(B, T, 256), pooled_projections=r(B, 64),
                timestep=torch.full((B,), 0.7, device=gpu), guidance=torch.full((B,), 3.5, device=gpu),
                img_ids=orc.latent_image_ids(32, 32).to(gpu), txt_ids=torch.zeros(T, 3, device=gpu), return_dict=False)


def _run_lines(cn, kw, hints, rowscales, window, gpu, B):
    """The loop's tower calls of one step: line 0 overwrites the sample buffers, the later lines add. Buffers as the pipeline
    prepares them: zero for the windowed path, arbitrary (here NaN) for the full path, which overwrites every row."""
    d = cn.inner_dim
    bufs = [torch.zeros(B, N, d, device=gpu, dtype=BF16) if window is not None else torch.full((B, N, d), float("nan"), device=gpu, dtype=BF16)
            for _ in range(len(cn.transformer_blocks))]
    for k, (hint, rs) in enumerate(zip(hints, rowscales)):
        cn(controlnet_cond=hint, conditioning_scale=0.75, _rowscale=rs.to(gpu), _accumulate_into=bufs, _overwrite=(k == 0), _window=window, **kw)
    torch.cuda.synchronize()
    return bufs


TOWER_CASES = {
    "one line": (1, [[(3, 7, 2, 12)]]),
    "two lines that accumulate": (1, [[(3, 5, 2, 12)], [(6, 8, 4, 15)]]),
    "batch 2, a box per image": (2, [[(2, 4, 1, 9), (5, 8, 3, 16)]]),
}


@pytest.mark.parametrize("case", list(TOWER_CASES))
def test_windowed_tower_equals_the_full_path_on_the_window_and_is_zero_outside(ops, gpu, attention_hip_only, case):
    """Reduced width (d = 512, H = 4, 2 double blocks, T = 64, N = 256), attention.hip serving the launches: every sample row inside
    the window has the bits of the full path and every row outside reads zero — where the full path holds (W·h + b)·scale·0 = ±0."""
    from reptext_amd.controlnet import active_row_window

    B, lines = TOWER_CASES[case]
    rowscales = [_box_rowscale(boxes, batch=None if B == 1 else B) for boxes in lines]
    window = active_row_window(rowscales, N)
    assert window is not None and window[0] % 16 == 0 and (window[1] - window[0]) * 2 <= N
    cn = _tower(gpu, 11)
    kw = _tower_inputs(gpu, B, 12)
    g = torch.Generator().manual_seed(13)
    hints = [torch.randn(B, N, 128, generator=g).to(gpu, BF16) for _ in lines]
    full = _run_lines(cn, kw, hints, rowscales, None, gpu, B)
    calls = []
    real = ops.attention
    ops.attention = lambda *a, **k: (calls.append(k.get("rows")), real(*a, **k))[1]
    try:
        win = _run_lines(cn, kw, hints, rowscales, window, gpu, B)
    finally:
        ops.attention = real
    # per line: block 0 whole, the last block only the items of its launch that hold a window row
    assert calls == [None, (T + window[0], T + window[1])] * len(lines)
    r0, r1 = window
    for i, (f, w) in enumerate(zip(full, win)):
        assert bool(torch.isfinite(f.float()).all()) and float(f[:, r0:r1].float().abs().max()) > 0, i
        assert torch.equal(w[:, r0:r1], f[:, r0:r1]), f"sample {i}: window rows differ from the full path"
        assert float(w[:, :r0].float().abs().max()) == 0.0 and float(w[:, r1:].float().abs().max()) == 0.0, i
        assert float(f[:, :r0].float().abs().max()) == 0.0 and float(f[:, r1:].float().abs().max()) == 0.0, i      # ±0 in the full path


def test_tower_refuses_a_window_it_cannot_honour(gpu):
    cn = _tower(gpu, 21)
    kw = _tower_inputs(gpu, 1, 22)
    hint = torch.zeros(1, N, 128, device=gpu, dtype=BF16)
    bufs = [torch.zeros(1, N, cn.inner_dim, device=gpu, dtype=BF16) for _ in range(2)]
    rs = _box_rowscale([(3, 7, 2, 12)]).to(gpu)
    with pytest.raises(ValueError, match="_window"):
        cn(controlnet_cond=hint, _rowscale=None, _accumulate_into=bufs, _overwrite=True, _window=(32, 128), **kw)
    with pytest.raises(ValueError, match="_window"):
        cn(controlnet_cond=hint, _rowscale=rs, _accumulate_into=bufs, _overwrite=True, _window=(32, 288), **kw)
    cn._fp8_attention = True
    with pytest.raises(ValueError, match="_window"):
        cn(controlnet_cond=hint, _rowscale=rs, _accumulate_into=bufs, _overwrite=True, _window=(32, 128), **kw)


# ------------------------------------------------------------------------------------------- the pipeline
def _pipe(gpu, seed):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    tr.load_state_dict(orc.init_mmdit_params(SMALL_T, seed))
    cn.load_state_dict(orc.init_mmdit_params(SMALL_CN, seed + 1, controlnet=True))
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _mask(box):
    from PIL import Image

    m = np.zeros([256, 256], dtype=np.uint8)
    m[box[0] : box[1], box[2] : box[3]] = 255
    return Image.fromarray(m)


def _inputs(gpu, seed, boxes):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, BF16)
    return dict(prompt_embeds=r(1, T, 256), pooled_prompt_embeds=r(1, 64), control_image=[r(1, N, 128) for _ in boxes], latents=r(1, N, 64),
                height=256, width=256, num_inference_steps=3, guidance_scale=3.5, control_mask=[_mask(b) for b in boxes],
                controlnet_conditioning_step=2, output_type="latent")


BOX_A = [(40, 100, 30, 200), (70, 120, 60, 240)]      # two text lines, pixel boxes (y0, y1, x0, x1): token rows 2..7 of 16
BOX_B = [(150, 200, 30, 200), (170, 230, 60, 240)]    # moved down: token rows 9..14


def test_pipeline_window_eager_graph_and_a_moved_box(gpu, attention_hip_only, monkeypatch):
    """Reduced-size pipeline, two text lines, tower off after step 2 of 3. The windowed loop gives the latents of the full path; eager
    equals graph replay; a call with the box moved — the sample buffers then hold the first box's
    rows — equals a fresh pipeline given that mask, eager and replayed, and going back to the first box is served by its graph."""
    from reptext_amd import pipeline as pl

    pipe = _pipe(gpu, 31)
    kw_a, kw_b = _inputs(gpu, 32, BOX_A), _inputs(gpu, 32, BOX_B)
    pipe.capture_graphs = False
    monkeypatch.setattr(pl, "TOWER_WINDOW", False)
    full_a = pipe(**kw_a).images.clone()
    assert pipe._tower_window_used is None
    monkeypatch.setattr(pl, "TOWER_WINDOW", True)
    eager_a = pipe(**kw_a).images.clone()
    win_a = pipe._tower_window_used
    assert win_a is not None and (win_a[1] - win_a[0]) * 2 <= N
    assert torch.equal(eager_a, full_a)
    pipe.capture_graphs = True
    assert torch.equal(pipe(**kw_a).images, eager_a)           # signature remembered
    assert torch.equal(pipe(**kw_a).images, eager_a)           # captured + replayed
    assert torch.equal(pipe(**kw_a).images, eager_a)
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 1
    # the box moves: another window, another signature
    fresh = _pipe(gpu, 31)
    fresh.capture_graphs = False
    ref_b = fresh(**kw_b).images.clone()
    win_b = fresh._tower_window_used
    assert win_b is not None and win_b != win_a
    assert torch.equal(pipe(**kw_b).images, ref_b)             # eager, on buffers that hold box A's rows
    assert pipe._tower_window_used == win_b
    assert torch.equal(pipe(**kw_b).images, ref_b)             # captured + replayed
    assert torch.equal(pipe(**kw_b).images, ref_b)
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 2
    assert torch.equal(pipe(**kw_a).images, eager_a)           # back: graph A on buffers that hold box B's rows
    assert torch.equal(pipe(**kw_b).images, ref_b)
    monkeypatch.setattr(pl, "TOWER_WINDOW", False)
    assert torch.equal(fresh(**kw_b).images, ref_b)            # and the full path agrees for the moved box too


# ------------------------------------------------------------------------------------------- full size: the one numeric change
def test_full_size_sample_4_stays_within_the_two_kernel_figure(ops, gpu):
    """The bound the issue sets on the last tower block, at the headline shape (RepText tower, d = 3072, H = 24, T = 512, N = 4096, a
    glyph box of the benchmark's size, 5 of 6 blocks evaluated): the rel-L2 between the windowed and the full-path sample 4 must not exceed
    the rel-L2 between the two bf16 kernels' outputs on the same input (block 4's own q, k, v; 4.58e-4 on MI355X). The windowed block runs
    its attention inside the full launch's own cut (attention_v3 with its key split here), so sample 4 is bitwise the full path's, like
    samples 0-3."""
    from reptext_amd import native
    from reptext_amd.config import reptext_controlnet_config
    from reptext_amd.controlnet import FluxControlNetModel, active_row_window

    lib = native.load()
    Tt, Nn, Hh = 512, 4096, 24
    m = torch.zeros(64, 64)
    m[7:12, 6:18] = 1.0                                   # the benchmark's glyph box: 72 tokens, 5 grid rows
    m[6, 6:18], m[12, 6:18] = 0.28, 0.09
    rs = m.reshape(-1)
    win = active_row_window([rs], Nn)
    assert win == (384, 800)
    cfg = reptext_controlnet_config()
    cn = FluxControlNetModel(**cfg, device=gpu, dtype=BF16).random_init_(seed=1)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, BF16)
    kw = dict(hidden_states=r(1, Nn, 64), encoder_hidden_states=r(1, Tt, 4096), pooled_projections=r(1, 768), controlnet_cond=r(1, Nn, 128),
              timestep=torch.full((1,), 0.7, device=gpu), guidance=torch.full((1,), 3.5, device=gpu) if cfg.get("guidance_embeds") else None,
              img_ids=orc.latent_image_ids(128, 128).to(gpu), txt_ids=torch.zeros(Tt, 3, device=gpu), return_dict=False,
              _rowscale=rs.to(gpu), _overwrite=True, _blocks_needed=(5, 0))

    def run(window):
        bufs = [torch.zeros(1, Nn, cn.inner_dim, device=gpu, dtype=BF16) for _ in range(len(cn.transformer_blocks))]
        cn(_accumulate_into=bufs, _window=window, **kw)
        torch.cuda.synchronize()
        return bufs

    cap, real, count = {}, ops.attention, [0]

    def spy(q, k, v, out, H, *a, **k2):
        count[0] += 1
        if count[0] == 5:                                 # block 4 of the full path
            cap["qkv"] = (q.clone(), k.clone(), v.clone())
        return real(q, k, v, out, H, *a, **k2)

    ops.attention = spy
    try:
        full = run(None)
    finally:
        ops.attention = real
    q, k, v = cap["qkv"]
    prev = lib.rt_attention_variant(-1)
    try:
        o3, o1 = torch.empty_like(q), torch.empty_like(q)
        lib.rt_attention_variant(1)
        ops.attention(q, k, v, o3, Hh)
        lib.rt_attention_variant(0)
        ops.attention(q, k, v, o1, Hh)
    finally:
        lib.rt_attention_variant(prev)
    reference = rel_l2(o1.float(), o3.float())
    wnd = run(win)
    r0, r1 = win
    for i in range(4):
        assert torch.equal(wnd[i], full[i]), i            # blocks 0-3 run whole: only their zero-linears are windowed
    assert float(wnd[4][:, :r0].float().abs().max()) == 0.0 and float(wnd[4][:, r1:].float().abs().max()) == 0.0
    got = rel_l2(wnd[4].float(), full[4].float())
    print(f"sample 4 windowed vs full: rel-L2 {got:.3e}; attention.hip vs attention_v3 on block 4's q, k, v: {reference:.3e}")
    assert got <= reference
    assert torch.equal(wnd[4], full[4])
