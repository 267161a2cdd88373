"""fp64 restatements of the photo flow's three kernels (csrc/photo.hip), for tests/test_photo_*.py.

``resize_aa_ref`` is ``torch.nn.functional.interpolate(window.double(), size, mode="bilinear", antialias=True, align_corners=False)`` on the
CPU, which runs in float64; ``gaussian_blur_ref`` and ``composite_ref`` are numpy. ``aa_tap_count`` restates the tap rule only to size
the tolerance of a case: the largest number of taps one output sample has on an axis."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def aa_tap_count(n_in: int, n_out: int) -> int:
    scale = n_in / n_out
    support = max(scale, 1.0)
    most = 0
    for i in range(n_out):
        center = scale * (i + 0.5)
        xmin = max(0, int(center - support + 0.5))
        most = max(most, min(n_in, int(center + support + 0.5)) - xmin)
    return most


def resize_aa_bound(window, size, mul=1.0, add=0.0) -> float:
    """(taps_h + taps_w + 4)·2^-24·max(|mul| + |add|, 1): a convex combination of values in [0, 1] accumulated in fp32, tap by tap."""
    _, _, cw, ch = window
    return (aa_tap_count(ch, size[0]) + aa_tap_count(cw, size[1]) + 4) * 2.0 ** -24 * max(abs(mul) + abs(add), 1.0)


def _planar_window(x, window) -> torch.Tensor:
    """float64 [C, h, w] of the window (x0, y0, w, h) of a uint8 [H,W] / [H,W,C] image (as x/255) or an fp32 [C,H,W] image."""
    x = torch.as_tensor(x)
    if x.dtype == torch.uint8:
        x = (x if x.dim() == 3 else x[..., None]).permute(2, 0, 1).double() / 255.0
    else:
        x = x.double()
    x0, y0, cw, ch = window
    return x[:, y0:y0 + ch, x0:x0 + cw]


def resize_aa_ref(x, window, size, mul=1.0, add=0.0) -> torch.Tensor:
    w = _planar_window(x, window)
    r = F.interpolate(w[None], size=tuple(size), mode="bilinear", antialias=True, align_corners=False)[0]
    assert r.dtype == torch.float64
    return mul * r + add


def gaussian_weights(sigma: float) -> np.ndarray:
    R = int(math.ceil(3.0 * sigma))
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * sigma * sigma))
    return w / w.sum()


def gaussian_blur_ref(plane, sigma: float) -> np.ndarray:
    """Separable, radius ceil(3·sigma), replicated borders, float64."""
    p = np.asarray(plane, dtype=np.float64)
    w = gaussian_weights(sigma)
    R = len(w) // 2
    H, W = p.shape
    rows = np.pad(p, ((0, 0), (R, R)), mode="edge")
    tmp = sum(w[k] * rows[:, k:k + W] for k in range(2 * R + 1))
    cols = np.pad(tmp, ((R, R), (0, 0)), mode="edge")
    return sum(w[k] * cols[k:k + H, :] for k in range(2 * R + 1))


def gaussian_blur_bound(sigma: float) -> float:
    """(2R + 5)·2^-24 per pass, two passes: 2R + 1 fp32 accumulations and the fp32 weights, on values in [0, 1]."""
    return 2 * (2 * int(math.ceil(3.0 * sigma)) + 5) * 2.0 ** -24


def composite_ref(photo, gen, alpha, window) -> np.ndarray:
    """float64 [H, W, C], unrounded: the photo outside the window; inside (1 − a)·src + a·clamp(gen/2 + 0.5, 0, 1)·255."""
    out = np.asarray(photo).astype(np.float64)
    x0, y0, cw, ch = window
    g = np.clip(np.asarray(gen, dtype=np.float64) / 2.0 + 0.5, 0.0, 1.0) * 255.0           # [C, ch, cw]
    a = np.asarray(alpha, dtype=np.float64)[..., None]
    src = out[y0:y0 + ch, x0:x0 + cw]
    out[y0:y0 + ch, x0:x0 + cw] = (1.0 - a) * src + a * g.transpose(1, 2, 0)
    return out


def distance_to_half_integer(v: np.ndarray) -> np.ndarray:
    return np.abs(v - np.floor(v) - 0.5)
