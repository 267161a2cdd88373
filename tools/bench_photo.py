"""What the photo flow adds around the denoising loop, on the device and on the host: a synthetic 4000x3000 photo, a mask whose region is
1500x1500, one text line (edge hint, position, regional mask at the photo's size), working size 1024x1024.
  device ... what FluxControlNetPhotoPipeline does: upload photo, mask and the three conditioning images once as uint8; rt_resize_aa of each
             to the working size, masks re-binarised; after the loop rt_resize_aa of the decoded fp32 image back to the region,
             rt_gaussian_blur_f32 of the mask, rt_composite_u8 into a copy of the photo, download of the result.
  host ..... the same work with PIL: crop, resize(BILINEAR) (PIL's is antialiased), upload of the crops; after the loop download of the
             decoded uint8 image, resize to the region, GaussianBlur of the mask crop, Image.composite, paste into a copy of the photo.
The loop and the VAE are the same in both and are not run; the decoded image is a random tensor. The two paths alternate `--repeats`
times in one process, the order reversed every other repeat; every figure is a host clock around work that ends in a device synchronise.
Each kernel is also timed alone with device events over `--launches` launches: the bytes the operation needs (input window + output, no
workspace traffic) over that time, next to the float4 copy rate MI355X_MICROARCH gives (6.29 TB/s). The expectation to confirm or refute:
the device path is the cheaper one and small against one denoising step (70.5 ms at this size, profiles/repaint_bench.json).
Prints a table and one JSON line.  python tools/bench_photo.py [--repeats 3] [--out profiles/photo_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageFilter

PW, PH = 4000, 3000
BBOX = (1250, 750, 2686, 2186)          # x0, y0, x1, y1 of the mask: 1436 x 1436, + 32 of padding = the 1500 x 1500 region
PAD, BLUR, WORK = 32, 4.0, 1024
COPY_RATE_GBS = 6290.0                  # float4 copy, measured (MI355X_MICROARCH)
STEP_MS = 70.5                          # one denoising step at 1024², full depth (profiles/repaint_bench.json)


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(fn, launches):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None, help="also merge the result into this JSON file under 'photo'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photo.py measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    from reptext_amd import ops
    from reptext_amd.pipeline_photo import photo_crop_region

    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, (PH, PW, 3), dtype=np.uint8)
    mask = np.zeros([PH, PW], dtype=np.uint8); mask[BBOX[1]:BBOX[3], BBOX[0]:BBOX[2]] = 255
    edges = np.full([PH, PW, 3], 255, dtype=np.uint8); edges[BBOX[1] + 40:BBOX[3] - 40:7, BBOX[0] + 40:BBOX[2] - 40] = 0
    region = photo_crop_region(BBOX, PW, PH, PAD, WORK, WORK)
    window = (region[0], region[1], region[2] - region[0], region[3] - region[1])
    cw, ch = window[2], window[3]
    decoded = (torch.rand(3, WORK, WORK, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    decoded_u8 = ((decoded * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()

    def device_before():
        up = lambda a: torch.from_numpy(a).to(dev)
        p, m, e = up(photo), up(mask), up(edges)
        line = up(mask)                                                   # the line's position and regional mask: two more uploads
        region_mask = up(mask)
        binary = lambda t: ops.resize_aa(t, window, (WORK, WORK))[0] >= 0.5
        work = (ops.resize_aa(p, window, (WORK, WORK)), binary(m).float(), ops.resize_aa(e, window, (WORK, WORK), 2.0, -1.0),
                binary(line).float() * 2.0 - 1.0, binary(region_mask).to(torch.uint8) * 255)
        return p, m, work

    def device_after(p, m):
        gen = ops.resize_aa(decoded, None, (ch, cw))
        alpha = ops.gaussian_blur((m[region[1]:region[3], region[0]:region[2]] >= 128).float().contiguous(), BLUR)
        return ops.composite_u8(p, gen, alpha, window).cpu()

    photo_pil, mask_pil, edges_pil = Image.fromarray(photo), Image.fromarray(mask), Image.fromarray(edges)

    def host_before():
        crops = [im.crop(region).resize((WORK, WORK), Image.BILINEAR) for im in (photo_pil, mask_pil, edges_pil, mask_pil, mask_pil)]
        return [torch.from_numpy(np.array(c)).to(dev) for c in crops]

    def host_after():
        small = Image.fromarray(decoded_u8.cpu().numpy())
        gen = small.resize((cw, ch), Image.BILINEAR)
        alpha = mask_pil.crop(region).point(lambda v: 255 if v >= 128 else 0).filter(ImageFilter.GaussianBlur(BLUR))
        out = photo_pil.copy()
        out.paste(Image.composite(gen, photo_pil.crop(region), alpha), region[:2])
        return out

    p, m, _ = device_before(); device_after(p, m); host_before(); host_after()           # warm every shape
    res = {k: [] for k in ("device_before", "device_after", "host_before", "host_after")}
    ran_after = {"device": [], "host": []}
    for k in range(args.repeats):
        order = ("device", "host") if k % 2 == 0 else ("host", "device")
        for j, path in enumerate(order):
            ran_after[path].append(order[j - 1])
            if path == "device":
                t, (p, m, _) = clocked(device_before); res["device_before"].append(t)
                t, _ = clocked(lambda: device_after(p, m)); res["device_after"].append(t)
            else:
                t, _ = clocked(host_before); res["host_before"].append(t)
                t, _ = clocked(host_after); res["host_after"].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    total = {path: [a + b for a, b in zip(res[path + "_before"], res[path + "_after"])] for path in ("device", "host")}

    # ---- each kernel alone
    alpha_in = (m[region[1]:region[3], region[0]:region[2]] >= 128).float().contiguous()
    gen = ops.resize_aa(decoded, None, (ch, cw))
    alpha = ops.gaussian_blur(alpha_in, BLUR)
    kernels = {
        "rt_resize_aa u8 3ch region->work": (lambda: ops.resize_aa(p, window, (WORK, WORK)), cw * ch * 3 + 3 * WORK * WORK * 4),
        "rt_resize_aa u8 1ch region->work": (lambda: ops.resize_aa(m, window, (WORK, WORK)), cw * ch + WORK * WORK * 4),
        "rt_resize_aa f32 3ch work->region": (lambda: ops.resize_aa(decoded, None, (ch, cw)), 3 * WORK * WORK * 4 + 3 * cw * ch * 4),
        "rt_gaussian_blur_f32 region": (lambda: ops.gaussian_blur(alpha_in, BLUR), 2 * cw * ch * 4),
        "rt_composite_u8 photo": (lambda: ops.composite_u8(p, gen, alpha, window), 2 * PW * PH * 3 + 4 * cw * ch * 4),
    }
    per_kernel = {}
    for name, (fn, nbytes) in kernels.items():
        ms = kernel_ms(fn, args.launches)
        per_kernel[name] = {"ms": round(ms, 4), "needed_MB": round(nbytes / 1e6, 2), "GBs": round(nbytes / ms / 1e6, 1),
                            "share_of_copy_rate": round(nbytes / ms / 1e6 / COPY_RATE_GBS, 3)}

    result = {"tool": "bench_photo", "device": torch.cuda.get_device_name(0), "photo": f"{PW}x{PH}", "region": f"{cw}x{ch}", "work": f"{WORK}x{WORK}",
              "mask_blur": BLUR, "ms": {k: [round(t, 2) for t in v] for k, v in res.items()},
              "ms_total": {k: [round(t, 2) for t in v] for k, v in total.items()},
              "median_ms": {**{k: round(med(v), 2) for k, v in res.items()}, **{k + "_total": round(med(v), 2) for k, v in total.items()}},
              "spread_ms": {**{k: round(max(v) - min(v), 2) for k, v in res.items()}, **{k + "_total": round(max(v) - min(v), 2) for k, v in total.items()}},
              "ran_after": ran_after, "host_over_device": round(med(total["host"]) / med(total["device"]), 2),
              "device_total_over_one_step": round(med(total["device"]) / STEP_MS, 3), "one_step_ms": STEP_MS,
              "kernels": per_kernel, "copy_rate_GBs": COPY_RATE_GBS,
              "note": "kernel ms include the op's allocations (output, workspace); GB/s = needed bytes (input window + output) / ms"}
    print("ms around the loop (before + after), one figure per repeat", flush=True)
    for path in ("device", "host"):
        print(f"  {path:6s}: " + "  ".join(f"{b:.1f} + {a:.1f} = {t:.1f}" for b, a, t in zip(res[path + '_before'], res[path + '_after'], total[path]))
              + f"   median {med(total[path]):.1f}, spread {max(total[path]) - min(total[path]):.1f}", flush=True)
    for name, k in per_kernel.items():
        print(f"  {name:36s} {k['ms']:.4f} ms  {k['needed_MB']:8.2f} MB  {k['GBs']:8.1f} GB/s  ({k['share_of_copy_rate']:.1%} of the copy rate)", flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["photo"] = result
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
