"""The flow of the reference's infer.py (infer.py:25-134) on this build, end to end on one MI355X, without checkpoints or cv2.

Same steps: render each text line with PIL, bbox -> position / regional masks, Canny(50,100) inverted (reptext_amd.hints),
then FluxControlNetPipeline.__call__ with control_image / control_position / control_mask / control_glyph and a seeded generator.
Weights are random-init FLUX.1-dev / RepText shapes (no network); prompt embeddings are random tensors in place of the T5/CLIP
encoders, which sit outside the hot path. With real checkpoints on disk use `FluxControlNetModel.from_pretrained(path)` /
`FluxControlNetPipeline.from_pretrained(path, controlnet=...)` and pass `prompt=` instead.

    python tools/infer_demo.py [--size 1024] [--steps 30] [--depth-scale 1.0] [--out gpurun_out/result.jpg]
    python tools/infer_demo.py --ip-image photo.jpg   # adds an image prompt: CLIP ViT-L/14 vision encoder + a 4-token IP-Adapter, random weights
    python tools/infer_demo.py --ip-image photo.jpg --ip-layout instantx   # the InstantX layout instead: SigLIP-so400m encoder (1152-wide
                                              # pooler_output) + a 128-token adapter with a term in all 19 + 38 blocks, random weights
    python tools/infer_demo.py --ip-image style.jpg --ip-mask region.png --line-ip-image brass.jpg --line-ip-image ""   # regional image prompts:
                                              # the style reference confined to a region, a material photo for the first text line only
    python tools/infer_demo.py --union-image photo.jpg [--union-scale 0.7 --union-end 0.8]   # a second ControlNet (Union-Pro-2.0 shape,
                                              # random weights) steered by the device Canny of the photo, beside the RepText tower
    python tools/infer_demo.py --negative-prompt "blurry letters, extra text" --true-cfg-scale 3.5   # true CFG in the text-to-image flow:
                                              # internal batch 2, [negative, positive]; without text encoders the negative embeddings are
                                              # random tensors seeded by the text (with checkpoints: negative_prompt= goes through encode_prompt)
    python tools/infer_demo.py --negative-prompt "blurry letters" --true-cfg-scale 3.5 --guidance-interval 0 0.5 --apg-eta 0 --apg-norm-threshold 15 \
                               --apg-momentum -0.5   # a guider on the true-CFG call (pipe.guider): the negative half is evaluated on the first
                                              # half of the steps only (the others run at batch 1), and at those steps the guidance is projected
                                              # (APG); the four flags have an effect only with --negative-prompt
    python tools/infer_demo.py --pag-scale 3.0 --pag-layer transformer_blocks.8 [--pag-layer single_transformer_blocks.0]   # perturbed-attention
                                              # guidance, which needs no negative prompt: internal batch 2, [perturbed, positive]; in the named
                                              # blocks an image token of the first half reads the text and itself only; there is no default layer
                                              # set; --guidance-interval and the --apg flags apply as they do to --negative-prompt
    python tools/infer_demo.py --source-image photo.jpg [--strength 0.6]   # repaint: the two lines are rendered INTO the photo by latent-blend
                                              # inpainting (FluxControlNetRepaintPipeline): the last strength·steps steps from the noised
                                              # photo, the photo put back outside the lines' boxes after every step; no second tower, no CFG
                                              # doubling; combines with the flags above
    python tools/infer_demo.py --source-image photo.jpg --photo-crop 32 [--mask-blur 4]   # the photo flow (FluxControlNetPhotoPipeline): the
                                              # photo stays at ITS size; the lines are laid out and their hints rendered at that size, the
                                              # region around them (+ 32 pixels) is cut out and resampled to --size on the device, repainted,
                                              # resampled back and blended into the untouched photo under a mask feathered with sigma 4
    python tools/infer_demo.py --inpaint      # infer_inpaint.py's flow (infer_inpaint.py:48-155): second 68-channel tower, masked
                                              # background image, position mask = bbox+-5, true CFG with negative embeddings
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from PIL import ImageFont

from controlnet_flux import FluxControlNetModel
from pipeline_flux_controlnet import FluxControlNetPipeline
from reptext_amd import hints
from reptext_amd.config import flux_dev_transformer_config, flux_vae_config, reptext_controlnet_config, union_pro2_controlnet_config
from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
from reptext_amd.transformer import FluxTransformer2DModel
from reptext_amd.vae import AutoencoderKL

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--steps", type=int, default=30)            # infer.py:127
ap.add_argument("--depth-scale", type=float, default=1.0)
ap.add_argument("--out", default="gpurun_out/result.jpg")
ap.add_argument("--inpaint", action="store_true")
ap.add_argument("--ip-image", default=None, help="image prompt for the text-to-image flow (ip_adapter_image=)")
ap.add_argument("--ip-layout", choices=("xlabs", "instantx"), default="xlabs", help="adapter + encoder pair behind --ip-image")
ap.add_argument("--ip-mask", default=None, metavar="FILE", help="region of --ip-image: a grey image, white = full strength (ip_adapter_mask=)")
ap.add_argument("--line-ip-image", action="append", default=None, metavar="FILE",
                help="an image prompt of its own for a text line, confined to the line's box (control_ip_adapter_image=): repeatable, one per "
                     "text line in order; an empty string leaves a line without one")
ap.add_argument("--line-ip-scale", type=float, default=1.0, help="strength of the --line-ip-image prompts (control_ip_adapter_scale=)")
ap.add_argument("--union-image", default=None, help="photo whose Canny edges steer the second ControlNet (control_image_union=)")
ap.add_argument("--union-scale", type=float, default=0.7)
ap.add_argument("--union-end", type=float, default=0.8)
ap.add_argument("--negative-prompt", default=None, help="negative prompt of the text-to-image flow (true CFG; needs --true-cfg-scale > 1)")
ap.add_argument("--true-cfg-scale", type=float, default=1.0)
ap.add_argument("--guidance-interval", type=float, nargs=2, default=(0.0, 1.0), metavar=("START", "STOP"),
                help="with --negative-prompt: true CFG on this share of the steps that run only")
ap.add_argument("--apg-eta", type=float, default=1.0, help="projected guidance: weight of the difference's component parallel to the positive prediction")
ap.add_argument("--apg-norm-threshold", type=float, default=0.0, help="projected guidance: clamp of the difference's per-sample norm (0: none)")
ap.add_argument("--apg-momentum", type=float, default=0.0, help="projected guidance: beta of the running difference (APG's usual value: -0.5)")
ap.add_argument("--line-prompt", action="append", default=None, metavar="TEXT",
                help="a prompt of its own for a text line (control_prompt=): repeatable, one per text line in order; an empty string leaves a line without one")
ap.add_argument("--line-prompt-scale", action="append", default=None, type=float, metavar="W",
                help="with --line-prompt: the strength of that line's prompt (control_prompt_scale), repeatable, parallel to --line-prompt; "
                     "1 = as without it, in [1/64, 64]; a line whose --line-prompt is '' takes 1")
ap.add_argument("--pag-scale", type=float, default=0.0, help="perturbed-attention guidance (pag_scale): on iff > 0, needs --pag-layer; not with --negative-prompt or --line-prompt")
ap.add_argument("--pag-layer", action="append", default=None, metavar="NAME",
                help="a block whose attention is perturbed (pag_applied_layers), repeatable: transformer_blocks.<i> or single_transformer_blocks.<i>")
ap.add_argument("--line-isolation", action="store_true",
                help="with --line-prompt: region isolation (control_prompt_isolation=True) — a line's text reads only its own box and the boxes do not read each other")
ap.add_argument("--source-image", default=None, help="photo to render the text into (the repaint pipeline's image=; the mask is the union of the lines' boxes)")
ap.add_argument("--strength", type=float, default=0.6, help="share of the schedule a repaint runs")
ap.add_argument("--photo-crop", type=int, default=None, help="with --source-image: keep the photo at its size and repaint only the region around "
                "the text, this many pixels of padding around the lines' boxes (the photo pipeline's padding_mask_crop=)")
ap.add_argument("--mask-blur", type=float, default=4.0, help="sigma of the feather under which the photo flow blends the result into the photo")
ap.add_argument("--stochastic", action="store_true", help="stochastic sampling (the scheduler's stochastic_sampling): every step re-noises the "
                "predicted clean image to the next sigma, with noise drawn inside the step kernel from the generator's seed; not with --inpaint")
ap.add_argument("--stochastic-eta", type=float, default=1.0, metavar="E", help="with --stochastic: the share of fresh noise, in (0, 1] (stochastic_eta)")
a = ap.parse_args()
if a.stochastic and a.inpaint:
    ap.error("--stochastic: the inpaint pipeline does not support stochastic sampling")
dev, bf16 = torch.device("cuda:0"), torch.bfloat16
ct, cc = flux_dev_transformer_config(), reptext_controlnet_config()
if a.depth_scale != 1.0:
    ct["num_layers"] = max(1, int(ct["num_layers"] * a.depth_scale)); ct["num_single_layers"] = max(1, int(ct["num_single_layers"] * a.depth_scale))
    cc["num_layers"] = max(1, int(cc["num_layers"] * a.depth_scale))
controlnet = FluxControlNetModel(**cc, device=dev, dtype=bf16).random_init_(seed=1)
pipeline_class = FluxControlNetPipeline
if a.photo_crop is not None and not a.source_image:
    ap.error("--photo-crop needs --source-image")
if a.source_image and a.photo_crop is not None:
    from pipeline_flux_controlnet_photo import FluxControlNetPhotoPipeline as pipeline_class          # the same components
elif a.source_image:
    from pipeline_flux_controlnet_repaint import FluxControlNetRepaintPipeline as pipeline_class      # the same components

scheduler_config = dict(stochastic_sampling=True, stochastic_eta=a.stochastic_eta) if a.stochastic else {}
pipe = pipeline_class(FlowMatchEulerDiscreteScheduler(**scheduler_config), AutoencoderKL(**flux_vae_config(), device=dev, dtype=bf16).random_init_(seed=2),
                              None, None, None, None, FluxTransformer2DModel(**ct, device=dev, dtype=bf16).random_init_(seed=0), controlnet)
pipe.set_progress_bar_config(disable=True)

width = height = a.size
layout_w, layout_h = width, height              # the size at which the lines are laid out and their hints rendered
if a.photo_crop is not None:                    # the photo flow: at the photo's own size; --size stays the working size
    from PIL import Image

    layout_w, layout_h = Image.open(a.source_image).size
side = min(layout_w, layout_h)
font = ImageFont.truetype("DejaVuSans.ttf", max(side * 80 // 1024, 12))        # infer.py:39-41 uses Arial Unicode, 80 px
text_list = ["مرحبا", "RepText"]
line_gap = side * 330 // 1024 - side * 200 // 1024                              # the second line follows the font's size, not the photo's height
text_position_list = [(layout_w * 370 // 1024, layout_h * 200 // 1024), (layout_w * 370 // 1024, layout_h * 200 // 1024 + line_gap)]
text_color_list = [(255, 255, 255), (255, 255, 255)]
control_image_list, control_position_list, control_mask_list, control_glyph_all = hints.build_text_hints(
    text_list, text_position_list, text_color_list, font, layout_w, layout_h)

g = torch.Generator().manual_seed(1)
prompt_embeds = torch.randn(1, 512, 4096, generator=g).to(dev, bf16)
pooled = torch.randn(1, 768, generator=g).to(dev, bf16)
generator = torch.Generator(device="cuda").manual_seed(42)                      # infer.py:113

if a.inpaint:
    import numpy as np
    from PIL import Image
    from pipeline_flux_controlnet_inpaint import FluxControlNetPipeline as InpaintPipeline

    ci = dict(cc, extra_condition_channels=4)                                    # 64 + 4 hint channels (INP:807-813)
    controlnet_inpaint = FluxControlNetModel(**ci, device=dev, dtype=bf16).random_init_(seed=3)
    ipipe = InpaintPipeline(pipe.scheduler, pipe.vae, None, None, None, None, pipe.transformer, controlnet, controlnet_inpaint=controlnet_inpaint)
    ipipe.set_progress_bar_config(disable=True)
    yy, xx = np.mgrid[0:height, 0:width]
    background = Image.fromarray(np.stack([(xx * 255 // width), (yy * 255 // height), np.full_like(xx, 96)], axis=-1).astype(np.uint8))
    background = hints.resize_img(background, max_side=a.size, min_side=a.size)
    width, height = background.size
    imgs, pos, masks, glyph = hints.build_text_hints(text_list[:1], text_position_list[:1], [(0, 255, 0)], font, width, height, position_margin=5)
    neg_e, neg_p = torch.randn(1, 512, 4096, generator=g).to(dev, bf16), torch.randn(1, 768, generator=g).to(dev, bf16)
    for it in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        image = ipipe(prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled, negative_prompt_embeds=neg_e, negative_pooled_prompt_embeds=neg_p,
                      true_guidance_scale=3.5, control_image=imgs, control_position=pos, control_mask=masks, control_glyph=glyph,
                      controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30, control_image_inpaint=background,
                      control_mask_inpaint=masks[-1], controlnet_conditioning_scale_inpaint=1.0, width=width, height=height,
                      num_inference_steps=a.steps, guidance_scale=3.5, generator=generator).images[0]
        torch.cuda.synchronize()
        print(f"inpaint call {it}: {time.perf_counter() - t0:.2f} s, {a.steps} steps, {width}x{height}, CFG (internal batch 2), two towers")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    image.save(a.out)
    print("saved", a.out, image.size)
    sys.exit(0)

ip_kwargs = {}
if a.ip_mask and not a.ip_image:
    sys.exit("--ip-mask is the region of --ip-image: give both")
if a.ip_image or a.line_ip_image:
    from PIL import Image
    from reptext_amd.image_encoder import CLIPVisionModelWithProjection, SiglipVisionModel
    from tools.bench_ip_adapter import adapter_sd, adapter_sd_instantx

    if a.ip_layout == "instantx":
        pipe.image_encoder = SiglipVisionModel(device=dev, dtype=bf16).random_init_(seed=4)              # so400m shape, 1152-wide pooler_output
        pipe.load_ip_adapter(adapter_sd_instantx(pipe.transformer, 128, dev, seed=5))
    else:
        pipe.image_encoder = CLIPVisionModelWithProjection(device=dev, dtype=bf16).random_init_(seed=4)  # ViT-L/14 shape, 768-wide embeds
        pipe.load_ip_adapter(adapter_sd(pipe.transformer, 4, dev, seed=5))
    pipe.set_ip_adapter_scale(0.7)
    if a.ip_image:
        ip_kwargs = dict(ip_adapter_image=Image.open(a.ip_image))
    if a.ip_mask:
        ip_kwargs.update(ip_adapter_mask=Image.open(a.ip_mask).convert("L").resize((a.size, a.size)))
    if a.line_ip_image:
        if len(a.line_ip_image) != len(text_list):
            sys.exit(f"--line-ip-image: give one per text line ({len(text_list)}), got {len(a.line_ip_image)}")
        ip_kwargs.update(control_ip_adapter_image=[Image.open(f) if f else None for f in a.line_ip_image], control_ip_adapter_scale=a.line_ip_scale)

if a.union_image:
    import numpy as np
    from PIL import Image

    pipe.controlnet_union = FluxControlNetModel(**union_pro2_controlnet_config(num_layers=cc["num_layers"]), device=dev, dtype=bf16).random_init_(seed=6)
    photo = np.asarray(Image.open(a.union_image).convert("RGB").resize((width, height)))
    ip_kwargs.update(control_image_union=hints.canny_hint_device(photo, dev, 100, 200, invert=False),      # [1,3,H,W] in [-1,1]
                     controlnet_conditioning_scale_union=a.union_scale, control_guidance_end_union=a.union_end)

if a.negative_prompt is not None:
    import zlib

    gn = torch.Generator().manual_seed(zlib.crc32(a.negative_prompt.encode("utf-8")))     # no text encoders here: embeddings named by the text
    ip_kwargs.update(negative_prompt_embeds=torch.randn(1, 512, 4096, generator=gn).to(dev, bf16),
                     negative_pooled_prompt_embeds=torch.randn(1, 768, generator=gn).to(dev, bf16), true_cfg_scale=a.true_cfg_scale)
    from reptext_amd.guidance import TrueCFGGuider

    # a plain attribute of the pipeline; the default values are the plain CFG call
    pipe.guider = TrueCFGGuider(start=a.guidance_interval[0], stop=a.guidance_interval[1], eta=a.apg_eta, norm_threshold=a.apg_norm_threshold,
                                momentum=a.apg_momentum)
elif a.true_cfg_scale != 1.0:
    ip_kwargs.update(true_cfg_scale=a.true_cfg_scale)                               # logs one line: no negative prompt, CFG stays off

if a.line_prompt:
    import zlib

    if len(a.line_prompt) != len(text_list):
        sys.exit(f"--line-prompt: give one per text line ({len(text_list)}), got {len(a.line_prompt)}")
    named = lambda text: torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(zlib.crc32(text.encode("utf-8")))).to(dev, bf16)
    # no text encoders here: embeddings named by the text (control_prompt=[...] takes the strings themselves where a T5 is loaded)
    ip_kwargs.update(control_prompt_embeds=[named(t) if t else None for t in a.line_prompt], control_prompt_max_sequence_length=128)
if a.line_prompt_scale:
    if not a.line_prompt or len(a.line_prompt_scale) != len(a.line_prompt):
        sys.exit(f"--line-prompt-scale: give one per --line-prompt ({len(a.line_prompt or [])}), got {len(a.line_prompt_scale)}")
    ip_kwargs.update(control_prompt_scale=list(a.line_prompt_scale))
if a.line_isolation:
    ip_kwargs.update(control_prompt_isolation=True)                                 # without --line-prompt the pipeline refuses it by name

if a.pag_scale or a.pag_layer:
    ip_kwargs.update(pag_scale=a.pag_scale, pag_applied_layers=a.pag_layer)         # the pipeline refuses a scale without layers by name

if a.source_image:
    from PIL import Image

    ip_kwargs.update(image=Image.open(a.source_image).convert("RGB"), strength=a.strength)     # mask_image=None: the union of control_mask
    if a.photo_crop is not None:
        ip_kwargs.update(padding_mask_crop=a.photo_crop, mask_blur=a.mask_blur)

for it in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    image = pipe(**ip_kwargs, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled, control_image=control_image_list,
                 control_position=control_position_list, control_mask=control_mask_list, control_glyph=control_glyph_all,
                 controlnet_conditioning_scale=1.0, controlnet_conditioning_step=30, width=width, height=height,
                 num_inference_steps=a.steps, guidance_scale=3.5, generator=generator).images[0]
    torch.cuda.synchronize()
    print(f"call {it}: {time.perf_counter() - t0:.2f} s for {len(text_list)} text lines, {a.steps} steps, {width}x{height} (hint VAE-encodes + loop + decode)")
os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
image.save(a.out)
print("saved", a.out, image.size)
