"""The photo pipeline (reptext_amd/pipeline_photo.py) on the GPU, with the reduced models of test_repaint_gpu.py and the small VAE.

A 200x264 photo, a 40x60 mask box, one text line whose conditioning images have the photo's size, working size 64x96 (N = 24 tokens),
padding_mask_crop 16, mask_blur 4, 4-step grid of which strength 0.75 runs 3. The region is (76, 64, 184, 136): 108x72, resampled by
1.125. Hints' posteriors are drawn from the global RNG and the source's from ``generator``: both are re-seeded before every call.

(i) the photo's size comes back and every pixel farther than ceil(3·4) from the box is the photo's, bit for bit; (ii) deep inside the box
(alpha exactly 1) the bytes are rint of the resampled decoded image; (iii) the latents are those of a plain repaint call on hand-made
working-size tensors; (iv) photo size = working size, the whole photo as region, no blur: the plain repaint call's bytes inside the mask, the
photo's outside; (v) eager = captured = replay, one graph key, the plain call's; (vi) repaint and base calls on the same object are
what they were before the photo calls."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

pytestmark = pytest.mark.gpu

from test_true_cfg_gpu import graph_keys  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, vae_pair  # noqa: E402,F401

PH, PW = 200, 264
H, W = 64, 96
N, T = 24, 64
BOX = (80, 120, 100, 160)                  # rows 80..119, columns 100..159
PAD, BLUR, R = 16, 4.0, 12
REGION = (76, 64, 184, 136)
WINDOW = (76, 64, 108, 72)
BF16 = torch.bfloat16


def box_image(box, h=PH, w=PW):
    m = np.zeros([h, w], dtype=np.uint8); m[box[0]:box[1], box[2]:box[3]] = 255
    return Image.fromarray(m)


def edges_image(box, h=PH, w=PW):
    im = Image.new("RGB", (w, h), (255, 255, 255))
    ImageDraw.Draw(im).rectangle((box[2] + 4, box[0] + 4, box[3] - 5, box[1] - 5), outline=(0, 0, 0))
    return im


def random_photo(seed, h=PH, w=PW):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).numpy()


def photo_pipe(gpu, seed, vae):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline_photo import FluxControlNetPhotoPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16).random_init_(seed)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16).random_init_(seed + 1)
    pipe = FluxControlNetPhotoPipeline(FlowMatchEulerDiscreteScheduler(), vae, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(seed)
    return pipe, (lambda *s: torch.randn(*s, generator=g).to(gpu, BF16))


def common(r):
    return dict(prompt_embeds=r(1, T, 256), pooled_prompt_embeds=r(1, 64), height=H, width=W, num_inference_steps=4, guidance_scale=3.5,
                controlnet_conditioning_step=2, latents=r(1, N, 64), strength=0.75)


def photo_call(r, photo):
    line = box_image(BOX)
    return dict(common(r), image=photo, control_image=[edges_image(BOX)], control_position=[line], control_mask=[line],
                padding_mask_crop=PAD, mask_blur=BLUR)


def working_size_call(kw, gpu):
    """The plain repaint call's arguments for ``kw``, made by hand: every image through ops.resize_aa, masks binarised at 0.5."""
    from reptext_amd import ops

    up = lambda im: torch.from_numpy(np.array(im)).to(gpu)
    binary = lambda im: ops.resize_aa(up(im), WINDOW, (H, W))[0] >= 0.5
    line = binary(kw["control_mask"][0])
    out = {k: v for k, v in kw.items() if k not in ("padding_mask_crop", "mask_blur")}
    out.update(image=ops.resize_aa(up(kw["image"]), WINDOW, (H, W))[None], mask_image=line.float()[None, None],
               control_image=[ops.resize_aa(up(kw["control_image"][0]), WINDOW, (H, W), 2.0, -1.0)[None]],
               control_position=[(binary(kw["control_position"][0]).float() * 2.0 - 1.0)[None, None]],
               control_mask=[Image.fromarray((line.to(torch.uint8) * 255).cpu().numpy())])
    return out


def run(call, pipe, kw, **more):
    torch.manual_seed(1234)
    return call(pipe, **{**kw, **more}, generator=torch.Generator().manual_seed(42)).images


def photo_run(pipe, kw, **more):
    return run(type(pipe).__call__, pipe, kw, **more)


def repaint_run(pipe, kw, **more):
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline

    return run(FluxControlNetRepaintPipeline.__call__, pipe, kw, **more)


def base_run(pipe, kw, **more):
    from reptext_amd.pipeline import FluxControlNetPipeline

    return run(FluxControlNetPipeline.__call__, pipe, {k: v for k, v in kw.items() if k not in ("image", "mask_image", "strength")}, **more)


def distance_to_box(box, h, w):
    """Chebyshev distance of every pixel to the box (0 inside), and the depth inside it (0 outside, 1 on its edge)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.maximum(np.maximum(box[0] - yy, yy - (box[1] - 1)), np.maximum(box[2] - xx, xx - (box[3] - 1)))
    depth = np.minimum(np.minimum(yy - box[0], box[1] - 1 - yy), np.minimum(xx - box[2], box[3] - 1 - xx)) + 1
    return np.maximum(out, 0), np.maximum(depth, 0)


def no_photo_left(pipe, photo):
    """Nothing of a call on the pipeline: no call state, no array, and no tensor of the photo's or the region's pixel size."""
    assert_no_call_state(pipe)
    sizes = {(PH, PW), (REGION[3] - REGION[1], REGION[2] - REGION[0]), tuple(photo.shape[:2])}
    for name, v in vars(pipe).items():
        assert not isinstance(v, (np.ndarray, Image.Image)), name
        if isinstance(v, torch.Tensor):
            assert v.dtype != torch.uint8 and not any(tuple(v.shape[i:i + 2]) in sizes for i in range(v.dim() - 1)), name


def test_region_of_the_set_up():
    from reptext_amd.pipeline_photo import photo_crop_region

    assert photo_crop_region((BOX[2], BOX[0], BOX[3], BOX[1]), PW, PH, PAD, W, H) == REGION


def test_photo_call_keeps_the_photo_and_pastes_the_resampled_result(vae_pair, gpu):
    """(i), (ii), (iii) and the three output types."""
    from reptext_amd import ops

    _, vae = vae_pair
    pipe, r = photo_pipe(gpu, 911, vae)
    pipe.capture_graphs = False
    photo = random_photo(7)
    kw = photo_call(r, photo)
    out = photo_run(pipe, kw, output_type="pil")
    assert len(out) == 1 and out[0].size == (PW, PH) and out[0].mode == "RGB"
    got = np.array(out[0])
    dist, depth = distance_to_box(BOX, PH, PW)
    # (i) farther than the feather's radius from the box: the photo's bytes — in particular everything outside the region
    assert np.array_equal(got[dist > R], photo[dist > R])
    outside_region = np.ones([PH, PW], dtype=bool); outside_region[REGION[1]:REGION[3], REGION[0]:REGION[2]] = False
    assert bool((dist[outside_region] > R).all()) and float((got[depth > 0] != photo[depth > 0]).mean()) > 0.9
    # (iii) the loop saw what a plain repaint call on hand-made working-size tensors sees
    lat = photo_run(pipe, kw, output_type="latent")
    assert lat.shape == (1, N, 64) and lat.dtype == torch.float32
    assert torch.equal(lat, repaint_run(pipe, working_size_call(kw, gpu), output_type="latent"))
    # (ii) deep inside the box alpha is exactly 1: rint of the decoded image resampled to the region
    decoded = pipe.vae.decode_packed(lat.to(BF16), 2 * (H // 16), 2 * (W // 16))[0]
    gen = ops.resize_aa(decoded, None, (WINDOW[3], WINDOW[2])).cpu()
    want = torch.round((gen * 0.5 + 0.5).clamp(0, 1) * 255.0).to(torch.uint8).permute(1, 2, 0).numpy()
    inner = (depth > R)[REGION[1]:REGION[3], REGION[0]:REGION[2]]
    assert int(inner.sum()) == (40 - 2 * R) * (60 - 2 * R)
    assert np.array_equal(got[REGION[1]:REGION[3], REGION[0]:REGION[2]][inner], want[inner])
    # the other output types are the same bytes
    as_np = photo_run(pipe, kw, output_type="np")
    assert as_np.shape == (1, PH, PW, 3) and as_np.dtype == np.float32 and np.array_equal(np.rint(as_np[0] * 255.0).astype(np.uint8), got)
    as_pt = photo_run(pipe, kw, output_type="pt")
    assert as_pt.shape == (1, 3, PH, PW) and as_pt.is_cuda and np.array_equal(np.rint(as_pt[0].permute(1, 2, 0).cpu().numpy() * 255.0).astype(np.uint8), got)
    # PIL, array and device tensor are one photo; mask_image = the line's mask is the default (the union of the control masks)
    for image in (Image.fromarray(photo), torch.from_numpy(photo).to(gpu), [photo]):
        assert np.array_equal(np.array(photo_run(pipe, dict(kw, image=image), output_type="pil")[0]), got)
    assert np.array_equal(np.array(photo_run(pipe, dict(kw, mask_image=box_image(BOX)), output_type="pil")[0]), got)
    # one photo, a batch of two prompts: two results for it, each with the photo's bytes away from the mask
    two = photo_run(pipe, dict(kw, prompt_embeds=r(2, T, 256), pooled_prompt_embeds=r(2, 64), latents=r(2, N, 64)), output_type="pil")
    assert len(two) == 2 and not np.array_equal(np.array(two[0]), np.array(two[1]))
    assert all(np.array_equal(np.array(im)[dist > R], photo[dist > R]) and im.size == (PW, PH) for im in two)
    no_photo_left(pipe, photo)


def test_photo_at_the_working_size_without_blur_is_the_repaint_call_inside_the_mask(vae_pair, gpu):
    """(iv): nothing is resampled (the identity), alpha is the binary mask."""
    _, vae = vae_pair
    pipe, r = photo_pipe(gpu, 921, vae)
    pipe.capture_graphs = False
    photo = random_photo(8, H, W)
    box = (16, 48, 24, 72)
    line = box_image(box, H, W)
    kw = dict(common(r), image=Image.fromarray(photo), mask_image=line, control_image=[edges_image(box, H, W)], control_position=[line],
              control_mask=[line], output_type="np")
    plain = np.rint(repaint_run(pipe, kw)[0] * 255.0).astype(np.uint8)
    got = np.rint(photo_run(pipe, kw, padding_mask_crop=100, mask_blur=0.0)[0] * 255.0).astype(np.uint8)
    inside = np.array(line) > 0
    assert got.shape == (H, W, 3) and np.array_equal(got[inside], plain[inside]) and np.array_equal(got[~inside], photo[~inside])
    assert float((plain[~inside] != photo[~inside]).mean()) > 0.5            # the plain call's pixels outside the mask went through the VAE
    no_photo_left(pipe, photo)


def test_eager_capture_replay_are_one_result_under_the_repaint_calls_key(vae_pair, gpu):
    """(v) and (vi)."""
    _, vae = vae_pair
    pipe, r = photo_pipe(gpu, 931, vae)
    photo = random_photo(9)
    kw = photo_call(r, photo)
    work = working_size_call(kw, gpu)
    pipe.capture_graphs = False
    repaint_before = repaint_run(pipe, work, output_type="latent").clone()
    base_before = base_run(pipe, work, output_type="latent").clone()
    assert graph_keys(pipe) == []
    pipe.capture_graphs = True
    results = [np.array(photo_run(pipe, kw, output_type="pil")[0]) for _ in range(3)]        # seen, captured, replayed
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    keys = graph_keys(pipe)
    assert len(keys) == 1 and isinstance(pipe._graph_cache[keys[0]], dict)
    assert len([k for k in keys[0] if isinstance(k, tuple) and k[:1] == ("repaint",)]) == 1
    assert torch.equal(photo_run(pipe, kw, output_type="latent"), repaint_before)
    # the plain repaint call builds this very key: it replays the entry, and returns what it returned before the photo calls
    assert torch.equal(repaint_run(pipe, work, output_type="latent"), repaint_before) and graph_keys(pipe) == keys
    # the base call: its own key, its old result
    for _ in range(3):
        assert torch.equal(base_run(pipe, work, output_type="latent"), base_before)
    assert len(graph_keys(pipe)) == 2 and graph_keys(pipe)[0] == keys[0]
    assert torch.equal(repaint_run(pipe, work, output_type="latent"), repaint_before)
    assert np.array_equal(np.array(photo_run(pipe, kw, output_type="pil")[0]), results[0])
    no_photo_left(pipe, photo)
