"""The reference loop of the loop tests (tests/loop_reference.py) against what it is held to: without extensions it returns the bits
of ``oracle.flux_oracle.denoise_loop``. Small configs on the CPU; no kernel runs here."""
import pytest
import torch

from oracle import flux_oracle as orc

from loop_reference import denoise_loop_reference
from test_guidance_host import SMALL_CN, SMALL_T

BF16 = torch.bfloat16


@pytest.mark.parametrize("store", [None, BF16], ids=["fp32", "bf16_storage"])
def test_without_extensions_the_reference_is_the_oracle_loop(store):
    """B = 2, two text lines — one with a shared [1,N,1] mask, one with a per-image [B,N,1] mask — for 2 of 3 steps, so the loop sums
    two towers, rounds per added tower and runs a step without any."""
    B, N, T = 2, 64, 16
    tp = orc.init_mmdit_params(SMALL_T, seed=931)
    cp = orc.init_mmdit_params(SMALL_CN, seed=932, controlnet=True)
    g = torch.Generator().manual_seed(933)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).float()
    pe, pooled, lat0, hints = r(B, T, 256), r(B, 64), r(B, N, 64), [r(B, N, 128), r(B, N, 128)]
    masks = [(torch.arange(N) % 3 == 0).float().reshape(1, N, 1), (torch.rand(B, N, 1, generator=g) > 0.5).float()]
    assert not torch.equal(masks[1][0], masks[1][1])
    sig = orc.flow_sigmas(3, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    args = (tp, SMALL_T, cp, SMALL_CN, lat0, pe, pooled, hints, masks, sig, orc.latent_image_ids(16, 16), torch.zeros(T, 3), 3.5, 0.8, 2)
    with orc.stored_as(store):
        want, got = orc.denoise_loop(*args), denoise_loop_reference(*args)
        towers_felt = orc.denoise_loop(*args[:-1], 0)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert bool(torch.isfinite(want).all()) and not torch.equal(want, towers_felt) and not torch.equal(want, lat0)
