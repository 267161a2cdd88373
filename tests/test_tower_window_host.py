"""The active row window of the ControlNet tower (controlnet.active_row_window): the contiguous run of image rows outside which the
regional masks of all text lines and batch entries are zero, rounded outward to ROW_WINDOW_ALIGN rows; None where the full path is
taken. Host logic only: CPU tensors, no kernel."""
import numpy as np
import torch
import torch.nn.functional as F

from reptext_amd import controlnet as cnm
from reptext_amd.controlnet import ROW_WINDOW_ALIGN as A, active_row_window

GRID = 64                 # 1024 x 1024 pixels -> 64 x 64 tokens
N = GRID * GRID


def box_mask(r0, r1, c0, c1, batch=1):
    """[batch, N, 1] mask, 1 on grid rows [r0, r1) x columns [c0, c1)."""
    m = torch.zeros(batch, GRID, GRID)
    m[:, r0:r1, c0:c1] = 1.0
    return m.reshape(batch, N, 1)


def expect(first, last):
    """Window of the rows first..last (inclusive), rounded outward."""
    return first // A * A, min(N, (last + A) // A * A)


def test_alignment_is_a_multiple_of_the_mfma_tile_rows():
    assert A % 16 == 0 and N % A == 0


def test_one_box():
    w = active_row_window([box_mask(10, 13, 7, 50)], N)
    assert w == expect(10 * GRID + 7, 12 * GRID + 49)
    assert w[0] % A == 0 and w[1] % A == 0 and w[0] <= 10 * GRID + 7 and w[1] > 12 * GRID + 49
    m = box_mask(10, 13, 7, 50).reshape(-1)
    assert float(m[: w[0]].abs().sum()) == 0.0 and float(m[w[1] :].abs().sum()) == 0.0        # nothing non-zero is left outside


def test_window_is_clipped_to_the_rows():
    assert active_row_window([box_mask(62, 64, 40, 64)], N) == (62 * GRID + 40 - (62 * GRID + 40) % A, N)
    assert active_row_window([box_mask(0, 2, 0, 10)], N) == (0, expect(0, GRID + 9)[1])


def test_two_lines_give_the_union():
    a, b = box_mask(5, 7, 3, 30), box_mask(20, 23, 10, 60)
    assert active_row_window([a, b], N) == expect(5 * GRID + 3, 22 * GRID + 59)
    assert active_row_window([b, a], N) == active_row_window([a, b], N)
    # one line without any non-zero row adds nothing; all lines zero is the full path
    assert active_row_window([a, torch.zeros(1, N, 1)], N) == active_row_window([a], N)


def test_batch_two_with_different_boxes_gives_the_union():
    m = torch.zeros(2, GRID, GRID)
    m[0, 8:10, 4:20] = 1.0
    m[1, 15:17, 30:50] = 1.0
    w = active_row_window([m.reshape(2, N, 1)], N)
    assert w == expect(8 * GRID + 4, 16 * GRID + 49)
    assert active_row_window([m.reshape(2, N)], N) == w                 # [B, N] row scales, the form the loop hands to the tower


def test_fractional_bilinear_edges_count_as_non_zero():
    """The pipeline's mask: a pixel box divided by 255 and resized x1/16 (bilinear); its edge tokens hold fractions."""
    px = np.zeros([1024, 1024], dtype=np.float32)
    px[200:300, 120:700] = 1.0                      # neither edge on a token boundary: rows 12.5 .. 18.75 of the grid
    m = F.interpolate(torch.from_numpy(px)[None, None], scale_factor=1 / 16, mode="bilinear").reshape(1, N, 1)
    nz = (m.reshape(-1) != 0).nonzero().flatten()
    assert 0.0 < float(m.reshape(-1)[nz].min()) < 1.0      # the case is what it claims to be
    w = active_row_window([m], N)
    assert w == expect(int(nz[0]), int(nz[-1]))
    assert w[0] <= int(nz[0]) and int(nz[-1]) < w[1]
    tiny = torch.zeros(1, N, 1)
    tiny[0, 1000] = 1e-30                           # any non-zero value counts, however small
    assert active_row_window([tiny], N) == expect(1000, 1000)
    assert active_row_window([tiny.to(torch.bfloat16)], N) == expect(1000, 1000)


def test_all_zero_all_ones_and_wide_windows_take_the_full_path():
    assert active_row_window([], N) is None
    assert active_row_window([torch.zeros(1, N, 1)], N) is None
    assert active_row_window([torch.ones(1, N, 1)], N) is None
    assert active_row_window([box_mask(0, 33, 0, 64)], N) is None                 # 33 of 64 grid rows: more than half
    assert active_row_window([box_mask(0, 32, 0, 64)], N) == (0, N // 2)          # exactly half is still windowed
    assert active_row_window([box_mask(2, 4, 0, 9), box_mask(60, 62, 0, 9)], N) is None    # two small boxes far apart: their union is wide


def test_cache_serves_repeats_and_does_not_go_stale(monkeypatch):
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append(1), real(self))[1])
    cnm._ROW_SPAN_CACHE.clear()
    m = box_mask(10, 12, 5, 40)
    w = active_row_window([m], N)
    assert len(reads) == 1
    assert active_row_window([m], N) == w and len(reads) == 1                    # same tensor, same version: no read
    assert active_row_window([m.reshape(1, N, 1)], N) == w and len(reads) == 1   # a view of it (what a caller reshapes per call) too
    m.reshape(GRID, GRID)[10:12, 5:40] = 0.0                                     # modified in place: the version counter moved
    m.reshape(GRID, GRID)[30:31, 0:20] = 0.5
    w2 = active_row_window([m], N)
    assert w2 == expect(30 * GRID, 30 * GRID + 19) and w2 != w and len(reads) == 2
    other = box_mask(50, 51, 0, 64)                                              # replaced by a tensor with another box
    assert active_row_window([other], N) == expect(50 * GRID, 50 * GRID + 63) and len(reads) == 3
    assert active_row_window([m], N) == w2 and len(reads) == 3                   # both stay cached
    # the cache keeps its tensors alive, so an address cannot come back with other contents under an old key
    for _ in range(12):
        t = box_mask(1, 2, 0, 5)
        assert active_row_window([t], N) == expect(GRID, GRID + 4)
        del t
    assert len(cnm._ROW_SPAN_CACHE) <= 8


def test_pipeline_switch_and_tower_capability():
    from reptext_amd import pipeline
    from reptext_amd.controlnet import FluxControlNetModel

    assert pipeline.TOWER_WINDOW is True
    cn = FluxControlNetModel(num_layers=1, num_single_layers=0, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=32,
                             in_channels=64, device="cpu", dtype=torch.bfloat16)
    assert cn.supports_row_window()
    cn._fp8_attention = True
    assert not cn.supports_row_window()                  # the e4m3 levels keep the full path
    cn._fp8_attention, cn._fp8_linears = False, "ln"
    assert not cn.supports_row_window()


def test_native_rows_entry_validates_on_the_host():
    """rt_attention_fwd_rows rejects bad arguments before any launch."""
    from reptext_amd import native

    lib = native.load()
    assert lib.rt_attention_fwd_rows(None, None, None, None, 0, 0, 0, 0, 1, 128, 1, 1.0, 0, 128, None, 0, None) == -1
    for lo, hi in ((-1, 64), (0, 257), (64, 64), (128, 64)):                                   # 0 <= row_lo < row_hi <= S
        assert lib.rt_attention_fwd_rows(16, 16, 16, 16, 128, 0, 128, 0, 1, 256, 1, 1.0, lo, hi, None, 0, None) == -1
    assert lib.rt_attention_fwd_rows(16, 16, 16, 16, 64, 0, 128, 0, 1, 256, 1, 1.0, 0, 64, None, 0, None) == -3       # ld < H * 128
    assert lib.rt_attention_fwd_rows(16, 16, 16, 16, 132, 0, 128, 0, 1, 256, 1, 1.0, 0, 64, None, 0, None) == -2      # ld % 8
