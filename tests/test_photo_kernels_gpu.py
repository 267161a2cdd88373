"""The photo flow's three kernels (csrc/photo.hip) per element against their fp64 restatements (tests/photo_reference.py), their
bitwise properties, and their refusals.

rt_resize_aa: (taps_h + taps_w + 4)·2^-24·max(|mul| + |add|, 1) per case, from the case's own tap counts — the result is a convex
combination of values of magnitude <= 1 accumulated in fp32; a window resampled to its own size is mul·(x/255) + add bit for bit.
rt_gaussian_blur_f32: (2R + 5)·2^-24 per pass; exact zeros farther than R from the input's support; ones stay ones within the bound
(and exactly: a pixel whose whole neighbourhood is 1 comes out as 1.0).
rt_composite_u8: alpha 0 is the photo, alpha 1 is rt_image_out's byte, outside the rectangle the photo, all bitwise; with random alpha
the byte is rint of the fp64 value wherever that value is farther than 1e-3 from a half-integer (the fp32 evaluation carries a few ulp
of 255, about 6e-5), the excluded share is asserted (<= 1 %, a property of the seeded inputs: 0.2 % expected) and excluded bytes are
within 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from photo_reference import (composite_ref, distance_to_half_integer, gaussian_blur_bound, gaussian_blur_ref, resize_aa_bound,  # noqa: E402
                             resize_aa_ref)

G = lambda seed: torch.Generator().manual_seed(seed)
PHOTO = torch.randint(0, 256, (61, 83, 3), generator=G(1), dtype=torch.uint8)           # H = 61, W = 83
WIDE = torch.randint(0, 256, (20, 230, 3), generator=G(2), dtype=torch.uint8)
GRAY = torch.randint(0, 256, (61, 83), generator=G(3), dtype=torch.uint8)
PLANAR = torch.rand(3, 37, 53, generator=G(4)) * 2 - 1

RESIZE_CASES = {
    "down": (PHOTO, (5, 7, 40, 33), (16, 24), 1.0, 0.0),
    "up": (PHOTO, (5, 7, 40, 33), (70, 90), 1.0, 0.0),
    "whole_photo": (PHOTO, (0, 0, 83, 61), (20, 28), 1.0, 0.0),
    "bottom_right_corner": (PHOTO, (53, 36, 30, 25), (12, 14), 1.0, 0.0),
    "one_pixel": (PHOTO, (10, 10, 1, 1), (4, 4), 1.0, 0.0),
    "9_to_8_rows_200_to_16_columns": (WIDE, (15, 6, 200, 9), (8, 16), 1.0, 0.0),
    "one_channel": (GRAY, (5, 7, 40, 33), (16, 24), 1.0, 0.0),
    "planar_up": (PLANAR, (0, 0, 53, 37), (64, 96), 1.0, 0.0),
    "planar_down": (PLANAR, (0, 0, 53, 37), (11, 13), 1.0, 0.0),
    "mul_add": (PHOTO, (5, 7, 40, 33), (16, 24), 2.0, -1.0),
}


@pytest.mark.parametrize("case", list(RESIZE_CASES))
def test_resize_aa_per_element(gpu, case):
    from reptext_amd import ops

    x, window, size, mul, add = RESIZE_CASES[case]
    want = resize_aa_ref(x, window, size, mul, add)
    got = ops.resize_aa(x.to(gpu), window, size, mul, add)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == ((1 if x.dim() == 2 else 3), *size)
    err = float((got.cpu().double() - want).abs().max())
    bound = resize_aa_bound(window, size, mul, add)
    print(f"rt_resize_aa [{case}]: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_resize_aa_to_the_own_size_is_the_identity_bitwise(gpu):
    from reptext_amd import ops

    for window, mul, add in (((3, 2, 41, 29), 1.0, 0.0), ((30, 6, 53, 55), 2.0, -1.0), ((0, 0, 83, 61), 0.37, 0.11)):
        x0, y0, cw, ch = window
        want = (PHOTO[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1).float() / 255.0) * mul + add
        assert torch.equal(ops.resize_aa(PHOTO.to(gpu), window, (ch, cw), mul, add).cpu(), want)
    assert torch.equal(ops.resize_aa(GRAY.to(gpu), None, (61, 83)).cpu(), (GRAY.float() / 255.0)[None])
    assert torch.equal(ops.resize_aa(PLANAR.to(gpu), (7, 3, 41, 29), (29, 41), 2.0, -1.0).cpu(), PLANAR[:, 3:32, 7:48] * 2.0 - 1.0)


BLUR_H, BLUR_W = 37, 45
BOX = (15, 22, 18, 27)                 # rows 15..21, columns 18..26


def blur_inputs():
    rnd = (torch.rand(BLUR_H, BLUR_W, generator=G(5)) > 0.5).float()
    corner = torch.zeros(BLUR_H, BLUR_W); corner[BLUR_H - 1, 0] = 1.0
    box = torch.zeros(BLUR_H, BLUR_W); box[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 1.0
    return {"random": rnd, "corner": corner, "box": box, "ones": torch.ones(BLUR_H, BLUR_W)}


@pytest.mark.parametrize("sigma", [0.5, 2.0, 4.3])
def test_gaussian_blur_per_element(gpu, sigma):
    from reptext_amd import ops

    R, bound = int(np.ceil(3 * sigma)), gaussian_blur_bound(sigma)
    for name, plane in blur_inputs().items():
        got = ops.gaussian_blur(plane.to(gpu), sigma).cpu()
        err = float(np.abs(got.double().numpy() - gaussian_blur_ref(plane.numpy(), sigma)).max())
        print(f"rt_gaussian_blur_f32 [sigma {sigma}, {name}]: max |err| {err:.3e}, bound {bound:.3e}")
        assert got.dtype == torch.float32 and got.shape == plane.shape and err <= bound
        if name == "ones":
            assert float((got - 1.0).abs().max()) <= bound
            assert bool((got == 1.0).all())                              # more than the bound: the weights add up to exactly 1 in the kernel's order
        if name == "box":
            yy, xx = torch.meshgrid(torch.arange(BLUR_H), torch.arange(BLUR_W), indexing="ij")
            dist = torch.maximum(torch.maximum(BOX[0] - yy, yy - (BOX[1] - 1)), torch.maximum(BOX[2] - xx, xx - (BOX[3] - 1)))
            assert int((dist > R).sum()) > 0 and bool((got[dist > R] == 0.0).all()) and bool((got[dist <= R] > 0.0).all())
            deep = torch.minimum(torch.minimum(yy - BOX[0], BOX[1] - 1 - yy), torch.minimum(xx - BOX[2], BOX[3] - 1 - xx)) >= R
            assert bool((got[deep] == 1.0).all()) and (int(deep.sum()) > 0) == (R <= 3)
        if name == "corner":                                            # the replicated border: the corner keeps more than an interior impulse
            interior = torch.zeros(BLUR_H, BLUR_W); interior[18, 22] = 1.0
            assert float(got[BLUR_H - 1, 0]) > float(ops.gaussian_blur(interior.to(gpu), sigma)[18, 22])
    plane = blur_inputs()["random"].to(gpu)
    assert ops.gaussian_blur(plane, 0.0) is plane


def image_out_bytes(gen, gpu):
    """The uint8 [h, w, C] that rt_image_out writes for ``gen`` [C, h, w] (its input is the decoder's haloed NHWC buffer)."""
    from reptext_amd import native

    C, h, w = gen.shape
    x = torch.zeros(1, h + 2, w + 2, C, device=gpu)
    x[0, 1:-1, 1:-1] = gen.to(gpu).permute(1, 2, 0)
    out = torch.empty(1, h, w, C, device=gpu, dtype=torch.uint8)
    native.call("rt_image_out", x.data_ptr(), None, out.data_ptr(), 1, h, w, C, C, torch.cuda.current_stream().cuda_stream)
    return out[0].cpu()


def rectangles(H, W):
    return {"left": (0, 5, 20, 10), "right": (W - 20, 5, 20, 10), "top": (30, 0, 20, 10), "bottom": (30, H - 10, 20, 10),
            "whole": (0, 0, W, H), "one_pixel": (41, 17, 1, 1), "last_pixel": (W - 1, H - 1, 1, 1)}


@pytest.mark.parametrize("W", [83, 84])
@pytest.mark.parametrize("C", [3, 1])
def test_composite_bitwise_properties(gpu, W, C):
    from reptext_amd import ops

    H = 37
    photo = torch.randint(0, 256, (H, W, C), generator=G(10 + W + C), dtype=torch.uint8)
    # the same bytes at an address that is not 16-byte aligned: the byte-wise form of the launch
    shifted = torch.empty(H * W * C + 1, dtype=torch.uint8, device=gpu)[1:].view(H, W, C).copy_(photo)
    assert shifted.data_ptr() % 16 != 0
    for name, (x0, y0, cw, ch) in rectangles(H, W).items():
        gen = torch.rand(C, ch, cw, generator=G(7)) * 2.4 - 1.2
        inside = torch.zeros(H, W, dtype=torch.bool); inside[y0:y0 + ch, x0:x0 + cw] = True
        for src in (photo.to(gpu), shifted):
            zero = ops.composite_u8(src, gen.to(gpu), torch.zeros(ch, cw, device=gpu), (x0, y0, cw, ch)).cpu()
            assert torch.equal(zero, photo), name
            one = ops.composite_u8(src, gen.to(gpu), torch.ones(ch, cw, device=gpu), (x0, y0, cw, ch)).cpu()
            assert torch.equal(one[~inside], photo[~inside]), name
            assert torch.equal(one[y0:y0 + ch, x0:x0 + cw], image_out_bytes(gen, gpu)), name


@pytest.mark.parametrize("W", [83, 84])
def test_composite_per_element(gpu, W):
    from reptext_amd import ops

    H, C, window = 37, 3, (9, 4, 61, 29)
    x0, y0, cw, ch = window
    g = G(20)
    photo = torch.randint(0, 256, (H, W, C), generator=g, dtype=torch.uint8)
    gen = torch.rand(C, ch, cw, generator=g) * 2.4 - 1.2
    alpha = torch.rand(ch, cw, generator=g)
    v = composite_ref(photo.numpy(), gen.numpy(), alpha.numpy(), window)
    got = ops.composite_u8(photo.to(gpu), gen.to(gpu), alpha.to(gpu), window).cpu().numpy().astype(np.float64)
    near_half = distance_to_half_integer(v) <= 1e-3
    share = float(near_half[y0:y0 + ch, x0:x0 + cw].mean())
    print(f"rt_composite_u8 [W {W}]: {share:.3%} of the rectangle within 1e-3 of a half-integer")
    assert share <= 0.01
    assert np.array_equal(got[~near_half], np.rint(v)[~near_half])
    assert float(np.abs(got - v).max()) <= 1.0


def test_refusals_without_a_launch():
    """Every refusal returns its code with a null stream and made-up pointers: nothing is dereferenced, nothing is launched."""
    from reptext_amd import native

    lib = native.load()
    P, BAD, SHAPE = 4096, native.RT_E_BADARG, native.RT_E_SHAPE
    big = 1 << 40

    def resize(inp=P, u8=1, C=3, H=61, W=83, x0=5, y0=7, cw=40, ch=33, out=P, OH=16, OW=24, ws=P, ws_bytes=big):
        return lib.rt_resize_aa(inp, u8, C, H, W, x0, y0, cw, ch, out, OH, OW, 1.0, 0.0, ws, ws_bytes, None)

    for kw in (dict(inp=None), dict(out=None), dict(ws=None), dict(H=0), dict(OW=0), dict(cw=0), dict(ch=-1), dict(x0=-1), dict(x0=44), dict(y0=29),
               dict(ws_bytes=16), dict(ws=P + 4)):
        assert resize(**kw) == BAD, kw
    for kw in (dict(C=2), dict(C=4), dict(OW=2), dict(OH=2), dict(H=70000, ch=69000, OH=66000)):
        assert resize(**kw) == SHAPE, kw
    assert native.RT_RESIZE_AA_MAX_SCALE == 16
    assert lib.rt_resize_aa_ws_bytes(3, 33, 24) >= 3 * 33 * 24 * 4 and lib.rt_resize_aa_ws_bytes(0, 33, 24) == 0

    def blur(inp=P, out=2 * P, H=37, W=45, sigma=2.0, ws=3 * P, ws_bytes=big):
        return lib.rt_gaussian_blur_f32(inp, out, H, W, sigma, ws, ws_bytes, None)

    for kw in (dict(inp=None), dict(out=None), dict(ws=None), dict(H=0), dict(W=-3), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(ws_bytes=37 * 45 * 4 - 1), dict(out=P)):
        assert blur(**kw) == BAD, kw
    for kw in (dict(sigma=32.5), dict(sigma=1e9), dict(H=65536)):
        assert blur(**kw) == SHAPE, kw
    assert native.RT_BLUR_MAX_RADIUS == 96

    def composite(photo=P, out=2 * P, H=37, W=83, C=3, x0=9, y0=4, cw=61, ch=29, gen=P, alpha=P):
        return lib.rt_composite_u8(photo, out, H, W, C, x0, y0, cw, ch, gen, alpha, None)

    for kw in (dict(photo=None), dict(out=None), dict(gen=None), dict(alpha=None), dict(H=0), dict(cw=0), dict(x0=23), dict(y0=9), dict(x0=-1)):
        assert composite(**kw) == BAD, kw
    for kw in (dict(C=2), dict(C=4)):
        assert composite(**kw) == SHAPE, kw
    with pytest.raises(native.NativeCallError, match="rt_composite_u8 failed: RT_E_SHAPE"):
        native.call("rt_composite_u8", P, 2 * P, 37, 83, 2, 9, 4, 61, 29, P, P, None)
