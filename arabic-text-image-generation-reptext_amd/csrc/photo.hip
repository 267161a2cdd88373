// The photo flow's pixel work on the device (reptext_amd/pipeline_photo.py): cut a window out of a full-size photo and resample it to
// the working size, resample the decoded image back, feather the mask, and blend the result into the untouched photo.
//
// rt_resize_aa restates ATen's _upsample_bilinear2d_aa (align_corners = False) on a window, as if the window were the whole image. Per
// axis: scale = in/out, support = max(scale, 1), center = scale·(i + 0.5), taps xmin = max(0, int(center − support + 0.5)) up to
// min(in, int(center + support + 0.5)), triangle weights max(0, 1 − |(j + xmin − center + 0.5)/max(scale, 1)|) normalised to sum 1.
// The tap range and the weights are formed in fp64 and the normalised weight is rounded to fp32 once; the samples are accumulated in
// fp32, first along x into the workspace [C][ch][OW], then along y. A tap at the very edge of the support has weight 0, so a tap range
// that differs from ATen's by rounding differs by a zero term. At scale 1 the taps are (i, i + 1) with weights (1, 0): a window
// resampled to its own size is the sample itself, and what is written is mul·(x/255) + add with each operation rounded once.
//
// rt_gaussian_blur_f32: separable, radius R = ceil(3σ), weights exp(−k²/(2σ²)) in fp32 normalised to sum 1 (formed on the host, passed
// by value), replicated borders; rows then columns through LDS tiles. A sum of zeros is +0, so an output farther than R from every
// non-zero input is exactly 0; the weights sum to exactly 1 in the kernel's order of addition, so a pixel whose whole neighbourhood is
// 1 comes out as exactly 1.
//
// rt_composite_u8: the photo's bytes are walked as one flat array, 16 per thread (one 16-byte load and store where photo and out are
// 16-byte aligned, byte by byte where they are not and for the last n % 16 bytes, in the same launch). Outside the rectangle a byte is
// copied; inside, g = clamp(gen/2 + 0.5, 0, 1)·255 as rt_image_out writes it, v = (1 − a)·src + a·g with every product and sum rounded
// once, out = rint(v) clamped: a = 0 is the photo's byte, a = 1 is rt_image_out's byte.
#include <math.h>
#include "rt_common.h"

namespace {

constexpr int RESIZE_MAX_SCALE = RT_RESIZE_AA_MAX_SCALE;
constexpr int BLUR_MAX_R = RT_BLUR_MAX_RADIUS;
constexpr int BLUR_TX = 256;     // outputs of a row tile
constexpr int BLUR_CW = 64, BLUR_CH = 32;   // a column tile: 64 columns by 32 rows, 256 threads, 8 outputs each

// The taps of output index i on an axis of `in` samples resampled to `out`: first tap, tap count, and 1 / (sum of the raw weights).
struct Taps { int first, count; double center, invscale, inv_total; };

__device__ __forceinline__ double tri(double x) { x = fabs(x); return x < 1.0 ? 1.0 - x : 0.0; }

__device__ __forceinline__ Taps aa_taps(int i, int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = scale >= 1.0 ? scale : 1.0;
  Taps t;
  t.center = scale * ((double)i + 0.5);
  t.invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
  const int lo = (int)(t.center - support + 0.5), hi = (int)(t.center + support + 0.5);
  t.first = lo < 0 ? 0 : lo;
  t.count = (hi > in ? in : hi) - t.first;
  double total = 0.0;
  for (int j = 0; j < t.count; ++j) total += tri(((double)(j + t.first) - t.center + 0.5) * t.invscale);
  t.inv_total = 1.0 / total;      // the tap nearest the centre weighs at least 1/2
  return t;
}
__device__ __forceinline__ float aa_weight(const Taps& t, int j) {
  return (float)(tri(((double)(j + t.first) - t.center + 0.5) * t.invscale) * t.inv_total);
}

// along x: window rows of the source -> tmp [C][ch][OW]. One thread per (row, ox), all C channels.
template <bool U8, int C>
__global__ void resize_aa_rows_kernel(const void* __restrict__ in, int H, int W, int x0, int y0, int cw, int ch, float* __restrict__ tmp, int OW) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (ox >= OW) return;
  const Taps t = aa_taps(ox, cw, OW);
  float acc[C] = {};
  for (int j = 0; j < t.count; ++j) {
    const float w = aa_weight(t, j);
    const int64_t px = (int64_t)(y0 + y) * W + (x0 + t.first + j);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float s;
      if (U8) s = __fdiv_rn((float)static_cast<const uint8_t*>(in)[px * C + c], 255.0f);
      else s = static_cast<const float*>(in)[(int64_t)c * H * W + px];
      acc[c] = fmaf(s, w, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) tmp[((int64_t)c * ch + y) * OW + ox] = acc[c];
}

// along y: tmp [C][ch][OW] -> out [C][OH][OW] = mul·r + add
template <int C>
__global__ void resize_aa_cols_kernel(const float* __restrict__ tmp, int ch, float* __restrict__ out, int OH, int OW, float mul, float add) {
#pragma clang fp contract(off)      // mul·r + add in plain operators: product and sum rounded once each (the taps are explicit fmaf)
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
  if (ox >= OW) return;
  const Taps t = aa_taps(oy, ch, OH);
  float acc[C] = {};
  for (int j = 0; j < t.count; ++j) {
    const float w = aa_weight(t, j);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(tmp[((int64_t)c * ch + t.first + j) * OW + ox], w, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[((int64_t)c * OH + oy) * OW + ox] = mul * acc[c] + add;
}

struct BlurWeights { float w[BLUR_MAX_R + 1]; };   // w[|k|], normalised

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The 2R + 1 taps around c[0], `step` elements apart, summed from the outermost pair inwards, the centre last: blur_weights() forms the
// centre weight against exactly this order, so that where all taps are 1 the sum is exactly 1.
__device__ __forceinline__ float blur_taps(const float* c, int step, int R, const BlurWeights& bw) {
  float acc = 0.f;
  for (int k = R; k >= 1; --k) {
    acc = fmaf(c[-k * step], bw.w[k], acc);
    acc = fmaf(c[k * step], bw.w[k], acc);
  }
  return fmaf(c[0], bw.w[0], acc);
}

__global__ __launch_bounds__(BLUR_TX) void blur_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int R, BlurWeights bw) {
  __shared__ float s[BLUR_TX + 2 * BLUR_MAX_R];
  const int y = blockIdx.y, xb = blockIdx.x * BLUR_TX, tid = threadIdx.x;
  const float* row = in + (int64_t)y * W;
  for (int i = tid; i < BLUR_TX + 2 * R; i += BLUR_TX) s[i] = row[clampi(xb - R + i, 0, W - 1)];
  __syncthreads();
  const int x = xb + tid;
  if (x >= W) return;
  out[(int64_t)y * W + x] = blur_taps(s + tid + R, 1, R, bw);
}

__global__ __launch_bounds__(256) void blur_cols_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int R, BlurWeights bw) {
  extern __shared__ float s[];      // [BLUR_CH + 2R][BLUR_CW]
  const int tx = threadIdx.x & (BLUR_CW - 1), ty = threadIdx.x / BLUR_CW;
  const int x = blockIdx.x * BLUR_CW + tx, yb = blockIdx.y * BLUR_CH;
  const int xs = x < W ? x : W - 1;
  for (int r = ty; r < BLUR_CH + 2 * R; r += 256 / BLUR_CW) s[r * BLUR_CW + tx] = in[(int64_t)clampi(yb - R + r, 0, H - 1) * W + xs];
  __syncthreads();
  if (x >= W) return;
  for (int o = ty; o < BLUR_CH; o += 256 / BLUR_CW) {
    const int y = yb + o;
    if (y >= H) break;
    out[(int64_t)y * W + x] = blur_taps(s + (o + R) * BLUR_CW + tx, BLUR_CW, R, bw);
  }
}

// one byte of the photo: channel c of pixel (y, x)
__device__ __forceinline__ uint8_t composite_byte(uint8_t src, int x, int y, int c, int x0, int y0, int cw, int ch, const float* __restrict__ gen,
                                                  const float* __restrict__ alpha) {
#pragma clang fp contract(off)
  const int rx = x - x0, ry = y - y0;
  if (rx < 0 || rx >= cw || ry < 0 || ry >= ch) return src;
  const int64_t p = (int64_t)ry * cw + rx;
  const float a = alpha[p];
  const float g = fminf(fmaxf(gen[(int64_t)c * ch * cw + p] * 0.5f + 0.5f, 0.f), 1.f) * 255.f;      // rt_image_out's expression (·0.5 is exact)
  const float v = (1.0f - a) * (float)src + a * g;
  return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 255.f));
}

__global__ void composite_u8_kernel(const uint8_t* __restrict__ photo, uint8_t* __restrict__ out, int H, int W, int C, int x0, int y0, int cw, int ch,
                                    const float* __restrict__ gen, const float* __restrict__ alpha, int vec) {
  const int64_t n = (int64_t)H * W * C, chunks = (n + 15) / 16;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b0 = i * 16;
    const int len = n - b0 < 16 ? (int)(n - b0) : 16;
    const int64_t pix = b0 / C;
    int c = (int)(b0 - pix * C), y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
    const bool wide = vec && len == 16;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (wide) v = *reinterpret_cast<const u32x4*>(photo + b0);
    // every byte is tested against the rectangle: a chunk may hold the end of one row and the start of the next
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < len) {
        const uint8_t src = wide ? (uint8_t)(v[k >> 2] >> (8 * (k & 3))) : photo[b0 + k];
        const uint32_t r = composite_byte(src, x, y, c, x0, y0, cw, ch, gen, alpha);
        if (wide) v[k >> 2] = (v[k >> 2] & ~(0xffu << (8 * (k & 3)))) | (r << (8 * (k & 3)));
        else out[b0 + k] = (uint8_t)r;
        if (++c == C) { c = 0; if (++x == W) { x = 0; ++y; } }
      }
    }
    if (wide) *reinterpret_cast<u32x4*>(out + b0) = v;
  }
}

// w[|k|] = exp(−k²/(2σ²)) / total in fp32 for k != 0; the centre weight is 1 − (the fp32 sum of the others, in blur_taps' order). That
// difference is exact where the sum is >= 1/2 and within half an ulp of 1 otherwise, so the 2R + 1 weights add up to exactly 1 in the
// kernel's own arithmetic: a neighbourhood of ones gives 1.0f, not 1 − 2^-24 (the composite then writes the generated byte itself).
inline BlurWeights blur_weights(float sigma, int R) {
  BlurWeights bw;
  float total = 1.0f;
  for (int k = 1; k <= R; ++k) {
    bw.w[k] = expf(-(float)(k * k) / (2.0f * sigma * sigma));
    total += 2.0f * bw.w[k];
  }
  float others = 0.f;
  for (int k = R; k >= 1; --k) {
    bw.w[k] /= total;
    others += bw.w[k];
    others += bw.w[k];
  }
  bw.w[0] = 1.0f - others;
  for (int k = R + 1; k <= BLUR_MAX_R; ++k) bw.w[k] = 0.f;
  return bw;
}

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }
inline int window_ok(int H, int W, int x0, int y0, int cw, int ch) {
  return x0 >= 0 && y0 >= 0 && cw >= 1 && ch >= 1 && (int64_t)x0 + cw <= W && (int64_t)y0 + ch <= H;
}

}  // namespace

extern "C" {

int64_t rt_resize_aa_ws_bytes(int32_t C, int32_t ch, int32_t OW) {
  if (C < 1 || ch < 1 || OW < 1) return 0;
  return align256((int64_t)C * ch * OW * (int64_t)sizeof(float));
}

int rt_resize_aa(const void* in, int32_t in_u8, int32_t C, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t cw, int32_t ch, float* out,
                 int32_t OH, int32_t OW, float mul, float add, void* ws, int64_t ws_bytes, void* stream) {
  if (!in || !out || !ws || C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || cw < 1 || ch < 1 || !window_ok(H, W, x0, y0, cw, ch)) return RT_E_BADARG;
  if (ws_bytes < rt_resize_aa_ws_bytes(C, ch, OW) || !RT_ALIGNED(ws, 16)) return RT_E_BADARG;
  if (C != 1 && C != 3) return RT_E_SHAPE;
  if ((int64_t)cw > (int64_t)RESIZE_MAX_SCALE * OW || (int64_t)ch > (int64_t)RESIZE_MAX_SCALE * OH) return RT_E_SHAPE;
  if (ch > 65535 || OH > 65535) return RT_E_SHAPE;          // the row index is grid.y
  hipStream_t st = (hipStream_t)stream;
  float* tmp = static_cast<float*>(ws);
  const dim3 grid_rows((OW + 255) / 256, ch), grid_cols((OW + 255) / 256, OH);
  if (in_u8 && C == 3) hipLaunchKernelGGL((resize_aa_rows_kernel<true, 3>), grid_rows, dim3(256), 0, st, in, H, W, x0, y0, cw, ch, tmp, OW);
  else if (in_u8) hipLaunchKernelGGL((resize_aa_rows_kernel<true, 1>), grid_rows, dim3(256), 0, st, in, H, W, x0, y0, cw, ch, tmp, OW);
  else if (C == 3) hipLaunchKernelGGL((resize_aa_rows_kernel<false, 3>), grid_rows, dim3(256), 0, st, in, H, W, x0, y0, cw, ch, tmp, OW);
  else hipLaunchKernelGGL((resize_aa_rows_kernel<false, 1>), grid_rows, dim3(256), 0, st, in, H, W, x0, y0, cw, ch, tmp, OW);
  if (C == 3) hipLaunchKernelGGL(resize_aa_cols_kernel<3>, grid_cols, dim3(256), 0, st, (const float*)tmp, ch, out, OH, OW, mul, add);
  else hipLaunchKernelGGL(resize_aa_cols_kernel<1>, grid_cols, dim3(256), 0, st, (const float*)tmp, ch, out, OH, OW, mul, add);
  return rt_hip_status();
}

int rt_gaussian_blur_f32(const float* in, float* out, int32_t H, int32_t W, float sigma, void* ws, int64_t ws_bytes, void* stream) {
  if (!in || !out || !ws || H < 1 || W < 1 || !(sigma > 0.f)) return RT_E_BADARG;
  if (!(3.0f * sigma <= (float)BLUR_MAX_R) || H > 65535) return RT_E_SHAPE;
  if (ws_bytes < (int64_t)H * W * (int64_t)sizeof(float) || in == out) return RT_E_BADARG;
  const int R = (int)ceilf(3.0f * sigma);
  const BlurWeights bw = blur_weights(sigma, R);
  hipStream_t st = (hipStream_t)stream;
  float* tmp = static_cast<float*>(ws);
  hipLaunchKernelGGL(blur_rows_kernel, dim3((W + BLUR_TX - 1) / BLUR_TX, H), dim3(BLUR_TX), 0, st, in, tmp, H, W, R, bw);
  const size_t lds = (size_t)(BLUR_CH + 2 * R) * BLUR_CW * sizeof(float);      // at most 57344 bytes
  hipLaunchKernelGGL(blur_cols_kernel, dim3((W + BLUR_CW - 1) / BLUR_CW, (H + BLUR_CH - 1) / BLUR_CH), dim3(256), lds, st, (const float*)tmp, out, H, W, R, bw);
  return rt_hip_status();
}

int rt_composite_u8(const uint8_t* photo, uint8_t* out, int32_t H, int32_t W, int32_t C, int32_t x0, int32_t y0, int32_t cw, int32_t ch,
                    const float* gen, const float* alpha, void* stream) {
  if (!photo || !out || !gen || !alpha || H < 1 || W < 1 || C < 1 || !window_ok(H, W, x0, y0, cw, ch)) return RT_E_BADARG;
  if (C != 1 && C != 3) return RT_E_SHAPE;
  const int64_t chunks = ((int64_t)H * W * C + 15) / 16;
  const int vec = RT_ALIGNED(photo, 16) && RT_ALIGNED(out, 16);
  int64_t blocks = (chunks + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(composite_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, photo, out, H, W, C, x0, y0, cw, ch, gen, alpha, vec);
  return rt_hip_status();
}

}  // extern "C"
