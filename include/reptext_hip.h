/*
 * reptext_hip.h — C ABI of librt_reptext_hip.so, the MI355X (gfx950) kernels behind the
 * FLUX.1-dev + RepText-ControlNet denoising path and the AutoencoderKL decoder.
 *
 * Boundary rules:
 *   - extern "C", plain pointers and sizes only; no torch types cross this line.
 *   - every pointer is a DEVICE pointer (HBM) unless its comment says "host".
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     nothing here synchronises, allocates or frees (graph-capture safe).
 *   - return value: 0 = enqueued; negative = argument rejected (RT_E_*), positive = hipError_t.
 *   - bf16 tensors are raw uint16 bit patterns (torch.bfloat16 storage).
 *
 * Each entry replaces torch ops that the reference reaches through diffusers; the
 * reference call site it serves is cited as file:line relative to /root/reference/RepText
 * (CN = controlnet_flux.py, PIPE = pipeline_flux_controlnet.py, INP = ..._inpaint.py) and the
 * third-party math as SURVEY.md Appendix A.x.
 */
#ifndef REPTEXT_HIP_H
#define REPTEXT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_E_BADARG (-1)   /* null pointer / non-positive size */
#define RT_E_ALIGN (-2)    /* pointer or leading dimension not aligned as documented */
#define RT_E_SHAPE (-3)    /* shape outside what the kernel supports */

/* Library identity: returns a static string "reptext_hip <abi> gfx950". */
const char* rt_version(void);
/* ABI revision; bumped when any struct or entry point below changes. rt_abi_version() returns the RT_ABI_VERSION the library was
 * built with; the Python binding reads this header and refuses a library whose number differs from it. */
#define RT_ABI_VERSION 15
int rt_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Linear layers: C = epilogue(A · Wᵀ + bias), bf16 operands, fp32 accumulate on MFMA.
 * Replaces every nn.Linear on the path: CN:277,280,292,386,391; Appendix A.1 steps 3,6,7,8;
 * A.2 (proj_mlp, to_q/k/v fused, proj_out); A.3 (x_embedder, context_embedder, proj_out).
 *
 * Epilogue, applied per element (row m, column n) in this order:
 *   v = acc + bias[n]
 *   if n >= gelu_from:        v = gelu_tanh(v)                      (A.1 step 7 / A.2 act_mlp)
 *   if gate:                  v *= gate[(m / rows_per_batch) * gate_ld + n]   (adaLN-Zero gates)
 *   v *= alpha                                                      (CN:395 conditioning_scale)
 *   if rowscale:              v *= rowscale[batch_index * stride_rowscale + m % rows_per_batch]   (PIPE:1062 regional mask)
 *   if res:                   v += res[m*ldr + n]                   (residual stream)
 *   if add2:                  v += add2[m*ld2 + n]                  (A.3 ControlNet injection)
 *   C[m*ldc + n] = v   (bf16, or fp32 when out_f32)
 * `res`/`add2` may alias C. A group is one problem; up to RT_GEMM_MAX_GROUPS problems with the
 * same K-loop code are tiled into ONE launch (image stream + text stream of a double block).
 * Batched over `batch` with element strides (0 = shared).
 * ---------------------------------------------------------------------------------------- */
#define RT_GEMM_MAX_GROUPS 4

typedef struct rt_gemm_group {
  const void* A;        /* bf16 [batch][M][lda]          */
  const void* W;        /* bf16 [N][ldw]  (torch Linear weight layout) */
  void* C;              /* bf16|f32 [batch][M][ldc]       */
  const void* bias;     /* bf16 [N] or NULL               */
  const float* gate;    /* f32 [batch*..][gate_ld] or NULL */
  const void* res;      /* same dtype as C, or NULL       */
  const void* add2;     /* bf16 [batch][M][ld2] or NULL   */
  const float* rowscale;/* f32 [rows_per_batch] or NULL   */
  int64_t lda, ldw, ldc, ldr, ld2, gate_ld;
  int64_t strideA, strideC, strideR, stride2;  /* per-batch element strides */
  int32_t M, N, K;      /* K % 64 == 0, N % 4 == 0        */
  int32_t batch;
  int32_t rows_per_batch; /* rows sharing one gate vector; 0 => M */
  int32_t gelu_from;    /* first column that gets GELU-tanh; <= 0 => all, >= N => none; a value inside (0, N) must be a
                         * multiple of 4 (the epilogue decides per 4-column group), anything else is RT_E_SHAPE */
  int32_t out_f32;      /* C/res dtype: 0 bf16, 1 f32     */
  float alpha;
  /* fp8 operands (rt_gemm_fp8 only; ignored by rt_gemm_bf16): A and W hold OCP e4m3 bytes, lda/ldw/strideA count
   * BYTES = elements, K % 128 == 0, and the product is de-quantised before the bias:
   *   acc[m][n] * a_scale[b*M + m] * w_scale[n]      (either pointer may be NULL = 1.0) */
  const float* a_scale; /* f32 [batch*M], one per activation row (rt_layernorm_modulate_fp8 / rt_quantize_rows_fp8) */
  const float* w_scale; /* f32 [N], one per output channel (rt_quantize_rows_fp8 on the weight rows)              */
  int64_t stride_rowscale; /* elements between the rowscale vectors of consecutive batch entries; 0 = one vector shared by the
                            * batch (the reference's one mask per text line); > 0: a mask per image of a sharded batch        */
  /* MX block scales (ABI 8; rt_gemm_fp8 only, ignored by rt_gemm_bf16). An activation row carries one E8M0 byte s (value
   * 2^(s-127)) per 32 consecutive K-elements. Scale tensors are laid out for the consuming GEMM wave: planes of 1024 K-elements
   * (8 K-tiles; a last partial plane is allocated whole); inside a plane 64-row chunks of 2 KiB in the order
   * [K-tile][row & 15][32-block of the K-tile][row >> 4 & 3]:
   *   byte(r, k) = base + (k/1024)*plane + (r/64)*2048 + ((k%1024)/128)*256 + (r%16)*16 + ((k%128)/32)*4 + (r/16)%4,  r = b*rows + m
   * (rt_common.h: rt_mx_scale_offset). base 16-byte aligned, plane % 2048 == 0, rows % 64 == 0 (rows = row count between batch
   * entries; a view that starts at row r0 of every entry passes base + (r0/64)*2048, r0 % 64 == 0).
   *  a_bscale != NULL: A's block scales (column 0 of A = k 0 of the scale tensor), applied by the MFMA itself
   *    (v_mfma_scale_f32_16x16x128_f8f6f4's scale operand) before the fp32 accumulation; a_scale may be NULL (usual) or given as well.
   *  c8 != NULL: columns n >= c8_from are NOT written to C; the epilogue value v (after every term) is quantised per 32 columns —
   *    s = the smallest exponent byte with max|v| <= 448 * 2^(s-127) (rt_quantize_mx_fp8's rule) — and stored as
   *    e4m3(v * 2^(127-s)) at c8[b*stride_c8 + m*ldc8 + (n - c8_from)] with s at byte(b*c_bscale_rows + m, c_bscale_k0 + n - c8_from)
   *    of (c_bscale, c_bscale_plane): the next GEMM's A and a_bscale, with no pass in between (c_bscale_k0 = the column of that A
   *    at which c8 starts, % 32 == 0).
   *    c8_from % 256 == 0, (N - c8_from) % 32 == 0, ldc8 % 8 == 0, c8 8-byte aligned. */
  const uint8_t* a_bscale;
  int64_t a_bscale_plane, a_bscale_rows;
  uint8_t* c8;
  uint8_t* c_bscale;
  int64_t ldc8, stride_c8, c_bscale_plane, c_bscale_rows;
  int32_t c8_from, c_bscale_k0;
  /* Convolution form (ABI 8; rt_gemm_bf16, one group, batch 1): conv_ks = 1 or 3 turns the problem into a stride-1, pad k/2 convolution
   * over a zero-haloed NHWC image. A = the image [B][conv_h2][conv_w2][conv_cin] (conv_h2 = H+2, conv_w2 = W+2) read as a matrix of
   * M = B*conv_h2*conv_w2 pixel rows, lda = conv_cin (% 64 == 0); W = [N][ks][ks][conv_cin], K = ks*ks*conv_cin; C / res / add2 = the
   * output image in the same haloed pixel order (ldc = its channel count). K-tile kt multiplies channels c0.. of tap (dy,dx) of
   * every pixel p with the rows of A shifted by (dy-1)*conv_w2 + (dx-1) pixels; rows shifted out of the image read as zero; halo
   * pixels are computed and NOT stored (the halo of C stays as it is). Replaces torch.nn.functional.conv2d of the AutoencoderKL
   * ResnetBlock2D / conv_in / shortcut convolutions (A.7); rt_conv2d_nhwc routes its stride-1, non-upsampling calls here.
   * conv_inv_w2 / conv_inv_h2 are filled in by the library. */
  int32_t conv_ks, conv_cin, conv_w2, conv_h2;
  float conv_inv_w2, conv_inv_h2;
  /* Fused q/k RMSNorm + RoPE (ABI 12; rt_gemm_bf16, bf16 C): rope_cos != NULL makes the tiles whose columns lie in
   * [rope_q0, rope_q0 + rope_w) or [rope_k0, rope_k0 + rope_w) leave the epilogue as rt_qk_rmsnorm_rope would rewrite them:
   * the bf16 value bf16(acc + bias) of a 256x256 tile goes through LDS, then every 128-column head of a row is RMS-normalised with
   * rope_wq / rope_wk (bf16 [128], the norm weights of THIS group's rows) and rotated with cos/sin row rope_pos0 + m (m = row in the
   * batch entry; rope_pos0 = 0 for text rows and single blocks, T for the image rows of a double block). Bit-identical to the GEMM
   * followed by rt_qk_rmsnorm_rope (one shared device function); saves that pass's read and write of q and k (A.1 steps 3,5; A.2).
   * rope_q0 / rope_k0 / rope_w % 256 == 0, ranges inside N and disjoint, gelu_from >= their ends, no gate / res / add2 / rowscale,
   * alpha == 1, C 16-byte aligned with ldc, strideC % 8 == 0; cos / sin / weights 16-byte aligned. All-zero = no fused step. */
  const float* rope_cos;  /* f32 [positions][128] */
  const float* rope_sin;
  const void* rope_wq;    /* bf16 [128] */
  const void* rope_wk;
  int32_t rope_q0, rope_k0, rope_w, rope_pos0;
  float rope_eps;
  int32_t rope_reserved;  /* 0 */
} rt_gemm_group;

int rt_gemm_bf16(const rt_gemm_group* groups /* host */, int32_t ngroups, void* stream);

/* Which epilogue serves rt_gemm_bf16's interior 256x256 tiles (speed only: both give the same bits). 1 (default, env
 * RT_GEMM_EPILOGUE) = a tile that lies wholly inside M x N and on one side of gelu_from takes a straight-line epilogue when its
 * group writes bf16 C in 16-byte steps (C 16-byte aligned, ldc / strideC / N % 8 == 0) and has no term but the bias and GELU
 * (no gate / res / add2 / rowscale, alpha == 1); 0 = the general epilogue everywhere. mode < 0 only queries; returns the previous
 * mode. Read when a launch is enqueued. Added without an ABI bump: nothing existing changed. */
int rt_gemm_epilogue_variant(int32_t mode);

/* Skinny linear for the adaLN tables (ABI 12; csrc/gemm_skinny.hip): M <= 32 activation rows given as the two-term bf16 split
 * hi + lo of an fp32 vector (rt_silu_split_bf16), up to two problems that share them:
 *   C[m][n] = lo[m]·W[n] + (hi[m]·W[n] + bias[n])        C f32 [M][ldc], W bf16 [N][ldw], bias bf16 [N] or NULL
 * Every W fragment is loaded once and used for both products; one wave per 16 output columns, so N is spread over all CUs.
 * Bit-identical to rt_gemm_bf16 {A = hi, bias, out_f32} followed by rt_gemm_bf16 {A = lo, res = C, out_f32}: same MFMA, operand
 * roles and K order, one accumulator chain per product, the same epilogue operations. Replaces those pairs in
 * mmdit.ModulationTable (AdaLayerNormZero/ZeroSingle/Continuous `linear(silu(temb))` for all steps at once; A.1 step 1, A.2, A.3).
 * Rejected on the host: null hi / lo / groups / W / C, ngroups outside 1..2, M < 1 (RT_E_BADARG); M > 32, K % 256, N % 16,
 * lda / ldw < K, ldc < N (RT_E_SHAPE); hi / lo / W / C not 16-byte aligned, bias not 8-byte aligned, lda / ldw % 8, ldc % 4 (RT_E_ALIGN). */
typedef struct rt_skinny_group {
  const void* W;        /* bf16 [N][ldw]   */
  const void* bias;     /* bf16 [N] or NULL */
  float* C;             /* f32 [M][ldc]    */
  int64_t ldw, ldc;
  int32_t N;
  int32_t reserved;     /* 0 */
} rt_skinny_group;
int rt_gemm_skinny_bf16(const void* hi, const void* lo, int64_t lda, int32_t M, int32_t K,
                        const rt_skinny_group* groups /* host */, int32_t ngroups, void* stream);

/* Same contraction and epilogue on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, fp32 accumulate, block scales fixed to
 * 1.0): BASELINE config 5 ("fp8 weights"), the projections fed by LayerNorm (to_q/k/v, add_*_proj, ff.net.0, proj_mlp).
 * Tiling, LDS image and schedule are those of rt_gemm_bf16 with a 128-element K-tile (the same 128-byte tile rows). */
int rt_gemm_fp8(const rt_gemm_group* groups /* host */, int32_t ngroups, void* stream);

/* Row-wise e4m3 quantisation: scale[r] = max|x[r][:]| / 448 (1.0 for an all-zero row), out[r][c] = e4m3(x[r][c] / scale[r]).
 * x bf16 (x_f32 = 0) or f32 [rows][ldx], out bytes [rows][ldo]; D % 8 == 0, D <= 65536. Used once per weight matrix (rows =
 * output channels) and for activation rows that do not come out of a LayerNorm. */
int rt_quantize_rows_fp8(const void* x, int64_t ldx, int32_t x_f32, void* out, int64_t ldo, float* scale,
                         int32_t rows, int32_t D, void* stream);

/* MX block quantisation of activation rows (config 5, "mx" level): per 32 consecutive elements one E8M0 scale byte
 * s = the smallest with max|x| <= 448 * 2^(s-127), clamped to [1, 253]; out = e4m3(x * 2^(127-s)), round to nearest even.
 * x bf16 (x_f32 = 0) or f32 [rows][ldx]; out bytes [rows][ldo]; scales in rt_gemm_group's layout (byte(row, k) there; bscale
 * 16-byte aligned, plane % 2048 == 0 and >= ceil(rows/64)*2048). D % 256 == 0. The fused producers (rt_gemm_fp8's c8 output,
 * rt_attention_fp8_fwd_mx) apply the same rule to their fp32 results; this pass serves tensors no fused producer writes. */
int rt_quantize_mx_fp8(const void* x, int64_t ldx, int32_t x_f32, void* out, int64_t ldo, uint8_t* bscale, int64_t plane,
                       int32_t rows, int32_t D, void* stream);

/* Small-M linear on fp32 activations, bf16 weights (adaLN modulation, time/guidance/pooled MLPs):
 *   y[b][n] (+)= post( Σ_k pre(x[b][k]) · W[n][k] + bias[n] ),  pre/post ∈ {identity, SiLU}
 * Replaces AdaLayerNormZero/ZeroSingle/Continuous `linear(silu(temb))` (A.1 step 1, A.2, A.3) and
 * CombinedTimestepGuidanceTextProjEmbeddings' MLPs (CN:287-291, A.5). HBM-bound on W. */
int rt_gemv_bf16w(const float* x, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                  float* y, int64_t ldy, int32_t B, int32_t N, int32_t K,
                  int32_t silu_in, int32_t silu_out, int32_t accumulate, void* stream);

/* y[r][:] = (y[r][:] + a[r % B][:]) + b[r % B][:] in fp32, rows r < rows, D % 4 == 0 (ABI 12). b may be NULL (one term). Adds the
 * step-invariant guidance and pooled-text embeddings (B rows each, computed once) to the timestep embeddings of every step in the
 * order CombinedTimestepGuidanceTextProjEmbeddings adds them (A.5: (t + g) + p). y / a / b contiguous rows of D, 16-byte aligned. */
int rt_add_rows_f32(float* y, const float* a, const float* b, int32_t rows, int32_t B, int32_t D, void* stream);

/* Timesteps(256, flip_sin_to_cos=True, shift 0): out[b] = [cos(t·f_j) | sin(t·f_j)], f_j = exp(-ln(1e4)·j/half).
 * A.5; feeds CN:287-291. t is already multiplied by 1000 by the caller (CN:282-284). */
int rt_timestep_embedding(const float* t, float* out, int32_t B, int32_t dim, void* stream);

/* FluxPosEmbed (CN:65,316-317; A.5): ids f32 [S][3] -> cos,sin f32 [S][sum(axes_dim)], fp64 angles,
 * each frequency repeated twice (interleaved). axes_dim host pointer, 3 ints. */
int rt_rope_table(const float* ids, float* cos_out, float* sin_out, int32_t S,
                  const int32_t* axes_dim /* host[3] */, float theta, void* stream);

/* LayerNorm(no affine, eps) over the last dim then (1+scale)·x + shift with per-batch vectors.
 * A.1 step 2/7/8, A.2, A.3 norm_out. x is bf16 or f32 (x_f32), out bf16.
 * rows = batch*rows_per_batch rows of length D (D % 8 == 0, D <= 8192); row r of batch b reads
 * x + b*stride_xb + r*ldx. shift/scale f32 with per-batch stride mod_ld (NULL => plain LN). */
int rt_layernorm_modulate(const void* x, int64_t ldx, int64_t stride_xb, int32_t x_f32,
                          void* out, int64_t ldo, int64_t stride_ob,
                          const float* shift, const float* scale, int64_t mod_ld,
                          int32_t batch, int32_t rows_per_batch, int32_t D, float eps, void* stream);
/* Two row segments in ONE launch (ABI 12): segment i is what rt_layernorm_modulate computes for its own x / out / shift / scale,
 * leading dimensions and row count; a row's arithmetic is the same, so the result is bit-identical to two calls. Both segments
 * share x_f32, D and eps. Serves the image rows + text rows of a double block's norm1 / norm2 (A.1 steps 2, 7), whose text-row
 * launch alone is at the kernel's latency floor. */
typedef struct rt_ln_segment {
  const void* x;        /* bf16|f32 [batch][rows_per_batch][ldx] */
  void* out;            /* bf16 [batch][rows_per_batch][ldo]     */
  const float* shift;   /* f32 [batch][mod_ld] or NULL (then scale NULL too) */
  const float* scale;
  int64_t ldx, stride_xb, ldo, stride_ob, mod_ld;
  int32_t batch, rows_per_batch;
} rt_ln_segment;
int rt_layernorm_modulate_pair(const rt_ln_segment* segs /* host[2] */, int32_t x_f32, int32_t D, float eps, void* stream);
/* Same, quantising the modulated row to e4m3 on the way out: out bytes [rows][ldo] and row_scale f32 [batch*rows_per_batch]
 * (= max|y| / 448 of that row), the A operand and a_scale of rt_gemm_fp8. One HBM read of x, half the write bytes. */
int rt_layernorm_modulate_fp8(const void* x, int64_t ldx, int64_t stride_xb, int32_t x_f32,
                              void* out, int64_t ldo, int64_t stride_ob, float* row_scale,
                              const float* shift, const float* scale, int64_t mod_ld,
                              int32_t batch, int32_t rows_per_batch, int32_t D, float eps, void* stream);

/* RMSNorm(Dh, weight, eps) on q and k heads + interleaved-pair RoPE, in place on a fused
 * projection buffer (A.1 steps 3,5; A.2). Row (b,s) holds q at column q_off and k at k_off,
 * H heads of Dh=128 each. Rows s < T use the text weights (norm_added_q/k), others the image
 * weights; pass T = 0 for single-stream blocks. cos/sin f32 [S][128]. The weights are read as
 * 16-byte vectors: wq_img / wk_img, and wq_txt / wk_txt when T > 0, must be 16-byte aligned
 * (RT_E_ALIGN otherwise; with T = 0 the text weights are not looked at). */
int rt_qk_rmsnorm_rope(void* buf, int64_t ld, int64_t stride_b, int64_t q_off, int64_t k_off,
                       const void* wq_txt, const void* wk_txt, const void* wq_img, const void* wk_img,
                       const float* cosv, const float* sinv,
                       int32_t B, int32_t S, int32_t T, int32_t H, float eps, void* stream);

/* Joint (non-causal, unmasked) attention, softmax(QKᵀ·scale)V, Dh = 128, flash-style on MFMA
 * (A.1 step 6; torch SDPA in the reference). q/k/v/o are bf16 with a common row stride ld
 * (elements) and per-batch stride; head h lives at column h*128. o may alias q (the query rows of
 * a 128-row block are overwritten only after every workgroup that reads them has finished).
 *
 * `ws` (optional, 256-byte aligned, rt_attention_ws_bytes(B,S,H) bytes): workspace of the key-split
 * tail. When (heads x query blocks) does not fill a whole number of rounds of the chip's workgroup
 * slots, the key tiles of the last partial round are dealt evenly over all slots and the partial
 * (max, sum, O) triples are combined in-kernel by the last arriver, in a fixed order (bitwise
 * reproducible; every batch entry is cut identically, so results do not depend on B). The first
 * B*H*ceil(S/128) int32 of ws are ticket counters: zero them ONCE after allocation; the kernel
 * leaves them zero. ws == NULL runs every block as one full-length workgroup.
 * rt_attention_ws_bytes returns 0 when nothing would be split for this shape on this device. */
int64_t rt_attention_ws_bytes(int32_t B, int32_t S, int32_t H);
int rt_attention_fwd(const void* q, const void* k, const void* v, void* o,
                     int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                     int32_t B, int32_t S, int32_t H, float scale,
                     void* ws, int64_t ws_bytes, void* stream);

/* rt_attention_fwd in which only the 128- or 256-row items that hold a query row of [row_lo, row_hi) do any work: the same kernel,
 * grid, key split and workspace as rt_attention_fwd for (B, S, H), so rows row_lo..row_hi-1 of o get exactly the bits rt_attention_fwd
 * gives them. The other rows of those items are written too; rows of untouched items are left as they are (with o aliasing q: the raw
 * query). 0 <= row_lo < row_hi <= S. rt_attention_fwd is the range [0, S). Added without an ABI bump: nothing existing changed. */
int rt_attention_fwd_rows(const void* q, const void* k, const void* v, void* o,
                          int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                          int32_t B, int32_t S, int32_t H, float scale, int32_t row_lo, int32_t row_hi,
                          void* ws, int64_t ws_bytes, void* stream);

/* Region-masked joint attention (per-line prompts): rt_attention_fwd in which the keys fall into n_groups <= 32 contiguous groups
 * and every query row carries a 32-bit set of the groups it sees. group_end: HOST array of n_groups ascending key indices, group g =
 * keys [group_end[g-1], group_end[g]); the last is S, all others are multiples of 64 (a 64-key tile then lies in one group; the ends
 * travel by value in the kernel arguments). row_vis: DEVICE [B][S] words, batch stride stride_vis_b elements (0: one table for the
 * batch); row i of entry b attends key j iff bit g(j) of row_vis[b][i] is set. A row that sees no key gets zeros, never NaN.
 * HIDDEN KEYS AND VALUES MUST STILL BE FINITE: no tile is skipped, a hidden key's value row meets a zero numerator on the MFMA
 * (0 x NaN = NaN). scale > 0 is required (RT_E_BADARG): a hidden score is -inf times it. Always csrc/attention.hip's kernel (its
 * grouped instantiation) with the grid, key split, workspace (rt_attention_ws_bytes) and batch invariance of the dense launch of
 * (B, S, H); never attention_v3, rt_attention_variant does not affect it. With every bit set the output has the bits of that kernel's
 * dense launch. Added without an ABI bump: nothing existing changed. */
int rt_attention_fwd_grouped(const void* q, const void* k, const void* v, void* o,
                             int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                             int32_t B, int32_t S, int32_t H, float scale,
                             const int32_t* group_end, int32_t n_groups, const uint32_t* row_vis, int64_t stride_vis_b,
                             void* ws, int64_t ws_bytes, void* stream);

/* Joint attention with a class id per KEY (region isolation of per-line prompts): rt_attention_fwd_grouped with visibility decided
 * per key instead of per 64-key tile. key_class: DEVICE [B][S] bytes, values 0..31, batch stride stride_class_b bytes (0: one table
 * for the batch); row_vis as above. Row i of entry b attends key j iff bit key_class[b][j] of row_vis[b][i] is set (only the low 5
 * bits of a class byte are read). Keys >= S are masked whatever lies behind the table; a row that sees no key gets zeros. A class
 * table that is constant on every 64-key tile is a group table: the output then has the bits of rt_attention_fwd_grouped.
 * Alignment and padding: row_vis 4-byte aligned (RT_E_ALIGN). key_class is read a byte at a time, bytes [0, S) of each entry and no
 * other: no alignment of base or stride and no padding is asked. RT_E_BADARG: a null table, scale <= 0, a negative stride.
 * Otherwise rt_attention_fwd_grouped's contract: hidden keys and values must be finite, o may alias q, the grid, key split and
 * workspace of the dense launch of (B, S, H), never attention_v3. Added without an ABI bump: nothing existing changed. */
int rt_attention_fwd_keyed(const void* q, const void* k, const void* v, void* o,
                           int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                           int32_t B, int32_t S, int32_t H, float scale,
                           const uint32_t* row_vis, int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b,
                           void* ws, int64_t ws_bytes, void* stream);

/* rt_attention_fwd_keyed with a self rule (perturbed-attention guidance): row i of entry b sees key j iff bit key_class[b][j] of
 * row_vis[b][i] is set OR j == i. The self rule holds for every row and costs nothing for a row that sees its own class anyway; with
 * every word 0 each row sees its own key alone and the output is v. A row always sees a key, so no row gets zeros. Arguments,
 * refusals, grid, key split and workspace are rt_attention_fwd_keyed's (one more instantiation of csrc/attention.hip's kernel; never
 * attention_v3). Added without an ABI bump: nothing existing changed. */
int rt_attention_fwd_keyed_self(const void* q, const void* k, const void* v, void* o,
                                int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                                int32_t B, int32_t S, int32_t H, float scale,
                                const uint32_t* row_vis, int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b,
                                void* ws, int64_t ws_bytes, void* stream);

/* rt_attention_fwd_grouped / rt_attention_fwd_keyed with an additive bias per key CLASS (a strength per line prompt): the logit of
 * (row i, key j) is scale * q_i.k_j + key_bias[b][c(j)] in natural-log units, c(j) = key j's group index (grouped) or class byte
 * (keyed); i.e. the softmax weight of every key of class c is multiplied by exp(key_bias[b][c]). key_bias: DEVICE fp32 [B][32],
 * batch stride stride_bias_b elements (0: one table for the batch); all 32 entries of a row are read, whichever classes occur, and
 * must be FINITE (an infinite or NaN bias is not a mask: visibility is row_vis's alone). Visibility is unchanged: a hidden key stays
 * hidden whatever its bias, a row that sees no key gets zeros. A table of zeros gives the bits of the unbiased entry. The same
 * constant on every class that occurs leaves the softmax what it was (up to rounding). RT_E_BADARG: a null table or a negative stride;
 * RT_E_ALIGN: a table that is not 4-byte aligned; otherwise the sibling's contract, grid, key split and workspace (two further
 * instantiations of csrc/attention.hip's kernel; never attention_v3). Added without an ABI bump: nothing existing changed. */
int rt_attention_fwd_grouped_biased(const void* q, const void* k, const void* v, void* o,
                                    int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                                    int32_t B, int32_t S, int32_t H, float scale,
                                    const int32_t* group_end, int32_t n_groups, const uint32_t* row_vis, int64_t stride_vis_b,
                                    void* ws, int64_t ws_bytes, void* stream, const float* key_bias, int64_t stride_bias_b);
int rt_attention_fwd_keyed_biased(const void* q, const void* k, const void* v, void* o,
                                  int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                                  int32_t B, int32_t S, int32_t H, float scale,
                                  const uint32_t* row_vis, int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b,
                                  void* ws, int64_t ws_bytes, void* stream, const float* key_bias, int64_t stride_bias_b);

/* Which kernel serves rt_attention_fwd (speed only; both are tested against the same references): 1 (default, env RT_ATTN_V3) =
 * shapes with S % 256 == 0 and S >= 1536 run csrc/attention_v3.hip — one wave per SIMD, 64 query rows per wave, O / Q / row sums
 * in asm-owned accumulator registers, hand-placed MFMA gaps (S = 4608: 247 vs 264 us) —, everything else csrc/attention.hip;
 * 0 = attention.hip always; 2 = attention_v3 wherever S % 256 == 0. mode < 0 only queries; returns the previous mode. */
int rt_attention_variant(int32_t mode);

/* BASELINE config 5, "CDNA4 fp8 MFMA attention": the same joint attention with e4m3 q, k, v and softmax numerators on
 * v_mfma_scale_f32_32x32x64_f8f6f4 (fp32 scores, statistics and accumulators; bf16 output). Static quantisation: q and k
 * (RMS-normalised) are stored as e4m3(16·x), v is cast as is, no calibration pass.
 * rt_attention_fp8_prep replaces rt_qk_rmsnorm_rope on this path: from the fused projection buffer (row (b,s): q at q_off,
 * k at k_off, v at v_off, H heads of 128) it writes qk8 = [B][S][2·H·128] bytes (normalised, rotated q | k) and
 * vt8 = [B][H][128][S64] bytes (S64 = S rounded up to 64; Vᵀ with the keys of every 64-key tile permuted into MFMA operand
 * order, zero beyond S); rt_attention_fp8_vt_bytes gives vt8's size. buf is not modified. The norm weights follow
 * rt_qk_rmsnorm_rope's rule: wq_img / wk_img, and wq_txt / wk_txt when T > 0, 16-byte aligned or RT_E_ALIGN. */
int64_t rt_attention_fp8_vt_bytes(int32_t B, int32_t S, int32_t H);
int rt_attention_fp8_prep(const void* buf, int64_t ld, int64_t stride_b, int64_t q_off, int64_t k_off, int64_t v_off,
                          const void* wq_txt, const void* wk_txt, const void* wq_img, const void* wk_img,
                          const float* cosv, const float* sinv, void* qk8, void* vt8,
                          int32_t B, int32_t S, int32_t T, int32_t H, float eps, void* stream);
int rt_attention_fp8_fwd(const void* qk8, const void* vt8, void* o, int64_t ldo, int64_t stride_ob,
                         int32_t B, int32_t S, int32_t H, float scale, void* stream);
/* The same attention with the output written as the NEXT projection's e4m3 A operand (config 5, "mx" level): o8[b][q][h*128 + d]
 * = e4m3(o * 2^(127-s)) with one E8M0 byte s per (row, 32 columns) in rt_gemm_group's scale layout (rt_quantize_mx_fp8's rule
 * applied to the fp32 output; no bf16 store and no quantisation pass in between): byte(b*bscale_rows + q, bscale_k0 + h*128 + d).
 * bscale_rows % 64 == 0, bscale_k0 % 128 == 0. Replaces `F.scaled_dot_product_attention` + the operand cast of to_out /
 * proj_out (A.1 steps 6-7, A.2) on the e4m3 path. */
int rt_attention_fp8_fwd_mx(const void* qk8, const void* vt8, void* o8, int64_t ldo8, int64_t stride_ob8, uint8_t* bscale,
                            int64_t plane, int64_t bscale_rows, int32_t bscale_k0, int32_t B, int32_t S, int32_t H, float scale,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters merged into the bf16 weights (ABI 10; csrc/lora.hip). The reference's pipeline is a FluxLoraLoaderMixin
 * (PIPE:15,163) and scales the adapters per call from joint_attention_kwargs["scale"] (PIPE:908-925, CN:263-276); here the
 * adapters are folded into the Linear weights in place, outside the denoising loop, from a kept pristine copy W0, so the loop
 * (and a captured graph of it) runs the unchanged GEMMs on the same buffers. Bound by memory: W0 is read and W written once.
 * ---------------------------------------------------------------------------------------- */
typedef struct rt_lora_term {
  const void* B;    /* bf16 [N][ldb]: lora_B rows, r columns zero-padded to a multiple of 32 */
  const void* At;   /* bf16 [K][lda]: lora_A TRANSPOSED, same padding */
  int64_t ldb, lda;
  int32_t r_pad;    /* % 32 == 0, >= 32 */
  float scale;      /* fp32 coefficient c (adapter weight x call scale x alpha/r) */
} rt_lora_term;
#define RT_LORA_MAX_TERMS 8
/* W[n][k] = bf16( W0[n][k] + sum_t scale_t * sum_j B_t[n][j] * At_t[k][j] ), fp32 accumulation, ONE rounding.
 * nterms == 0 copies W0 to W bit for bit. W may alias W0. K % 8 == 0, N >= 1, 16-byte aligned rows.
 * Rejected on the host: null pointers (RT_E_BADARG), nterms > RT_LORA_MAX_TERMS, r_pad % 32 or K % 8 (RT_E_SHAPE), W0 / W / B / At
 * not 16-byte aligned or a leading dimension not a multiple of 8 (RT_E_ALIGN); ld0 / ldw < K, ldb / lda < r_pad (RT_E_BADARG). */
int rt_lora_merge_bf16(const rt_lora_term* terms /* host */, int32_t nterms, const void* W0, int64_t ld0,
                       void* W, int64_t ldw, int32_t N, int32_t K, void* stream);

/* ------------------------------------------------------------------------------------------
 * IP-Adapter image prompt (csrc/ip_attention.hip): the cross-attention term a FLUX double block adds to its image stream,
 *   o (+)= ip_scale * softmax( bf16(rmsnorm(q) * wq) * K^T * sm_scale ) * V          (heads of 128, concatenated along columns)
 * q: the block's RAW image-stream query projection, bf16 rows of ldq elements (e.g. the fused q|k|v buffer: ldq = 3*H*128), head h at
 * column h*128; it is NOT modified. The RMSNorm (eps, weight wq = norm_q.weight bf16[128]) is computed in fp32 from the raw row and
 * rounded to bf16 as the MFMA operand. k, v: bf16 [B|1][n_ip][ldkv], head h at column h*128; stride_kvb = 0 shares one image prompt
 * between the batch entries. o: bf16 or f32 (o_f32) rows of ldo elements; accumulate != 0 adds to what o holds. Only the first N rows
 * and H*128 columns of each batch entry of o are touched. One pass, no online softmax: keys are padded to a multiple of 32 inside
 * the kernel and the padding is masked. Any N >= 1.
 * Rejected on the host: null pointers, B / N / H / n_ip < 1, sm_scale <= 0, a leading dimension < H*128 (RT_E_BADARG); n_ip > 128 (RT_E_SHAPE);
 * pointers not 16-byte aligned, ldq / ldkv / the bf16 ldo or a batch stride not a multiple of 8 (f32 o: of 4) (RT_E_ALIGN). */
int rt_ip_attention(const void* q, int64_t ldq, int64_t stride_qb, const void* wq,
                    const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
                    void* o, int64_t ldo, int64_t stride_ob, int32_t o_f32, int32_t accumulate,
                    int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale, float eps, void* stream);
/* ABI 14. The same kernel body with an optional fp32 column gate (the InstantX adapter form, ip_adapter.py):
 *   o (+)= gate[b][h*128 + c] * ( ip_scale * softmax( bf16(rmsnorm(q) * wq) * K^T * sm_scale ) * V )
 * gate: fp32 [B][>= H*128] with batch stride stride_gb (elements), e.g. the gate_msa chunk of a row of the adaLN modulation table, so
 * that a double block accumulates its gated term straight onto the fp32 (or bf16) residual rows in one launch; NULL = no gate, which
 * is rt_ip_attention bit for bit. The product with the gate is formed in fp32 before the write or accumulate. q may be any strided
 * view: a single block passes column 2*H*128 of its fused [k|v|q|mlp] buffer with ldq = 7*H*128 and N = all S rows. K is used as
 * given (this adapter form stores it already RMS-normalised); there is no K norm in the kernel.
 * Rejected on the host as rt_ip_attention, and: a negative stride_gb (RT_E_BADARG); gate not 16-byte aligned or stride_gb % 4 (RT_E_ALIGN). */
int rt_ip_attention_gated(const void* q, int64_t ldq, int64_t stride_qb, const void* wq,
                          const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
                          const float* gate, int64_t stride_gb,
                          void* o, int64_t ldo, int64_t stride_ob, int32_t o_f32, int32_t accumulate,
                          int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale, float eps, void* stream);
/* rt_ip_attention_gated with an fp32 weight per query row (a regional image prompt):
 *   o[b][r] (+)= gate[b] * ( (ip_scale * row_w[b][r]) * softmax(...) * V )
 * row_w: fp32 [B|1][N], batch stride stride_wb (elements; 0 = one table for the batch). Any finite value: fractional, above 1 or
 * negative. The weight is multiplied into ip_scale in fp32 before the gate and before any rounding, so a table of 1.0f gives the bits
 * of rt_ip_attention_gated. A row of weight 0 is selected out, not multiplied: with accumulate its output elements are neither read
 * nor written, without it they are written as +0, and nothing of its q row (NaN or Inf included) reaches any output. A 16-row tile
 * whose rows are all 0 loads no q and runs no RMSNorm and no MFMA; a workgroup (128 rows, 256 for n_ip > 96) whose rows are all 0
 * does not stage K / V either: the launch costs what its non-zero rows cost. gate stays optional (NULL).
 * Rejected on the host as rt_ip_attention_gated, and: row_w NULL (use rt_ip_attention_gated) or stride_wb < 0 (RT_E_BADARG); row_w
 * not 4-byte aligned (RT_E_ALIGN). */
int rt_ip_attention_rows(const void* q, int64_t ldq, int64_t stride_qb, const void* wq,
                         const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
                         const float* gate, int64_t stride_gb, const float* row_w, int64_t stride_wb,
                         void* o, int64_t ldo, int64_t stride_ob, int32_t o_f32, int32_t accumulate,
                         int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale, float eps, void* stream);
/* y[i] = bf16( 0.5 x[i] (1 + erf(x[i] / sqrt 2)) ): the exact GELU of the InstantX image projection (rt_gemm_group's epilogue has the
 * tanh form only). x fp32, y bf16, n elements; once per call, outside the loop. Null pointers or n < 1: RT_E_BADARG. */
int rt_gelu_erf_bf16(const float* x, void* y, int64_t n, void* stream);
/* y[b][r][0..D) = bf16( y[b][r][:] + x[b][r][:] ) on bf16 views with their own leading dimensions and batch strides (elements): adds a
 * single block's IP-Adapter term onto the attention output inside the fused [k|v|q|mlp] buffer (ldy = 7*H*128) before proj_out.
 * Rejected on the host: null pointers, batch / rows < 1, D < 8, ld < D, a negative batch stride (RT_E_BADARG); D % 8 (RT_E_SHAPE);
 * pointers not 16-byte aligned, a leading dimension or batch stride not a multiple of 8 (RT_E_ALIGN). */
int rt_add_bf16_2d(const void* x, int64_t ldx, int64_t stride_xb, void* y, int64_t ldy, int64_t stride_yb,
                   int32_t batch, int32_t rows, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prompt encoders (PIPE:232-347: T5-XXL encoder -> prompt_embeds [B,512,4096], CLIP-L text model ->
 * pooled_prompt_embeds [B,768]). Once per prompt, outside the loop. Matrix work is rt_gemm_bf16; attention (head dim 64)
 * is assembled per head from rt_gemm_bf16 / rt_softmax_rows_bias / rt_transpose_bf16 / rt_gemm_bf16.
 * ---------------------------------------------------------------------------------------- */
/* out[i][:] = table[clamp(ids[i])][:] — nn.Embedding lookup of bf16 rows (T5 `shared`, CLIP token_embedding). ids: device int32. */
int rt_embedding_gather(const void* table, int64_t ld, const int32_t* ids, void* out, int64_t ldo,
                        int32_t n, int32_t D, int32_t vocab, void* stream);
/* T5LayerNorm: out = x * rsqrt(mean(x^2) + eps) * w, x bf16 or f32 (x_f32), w/out bf16. No mean subtraction, no bias. */
int rt_rmsnorm_rows(const void* x, int64_t ldx, int32_t x_f32, const void* w, void* out, int64_t ldo,
                    int32_t rows, int32_t D, float eps, void* stream);
/* p = softmax(scale·s + bias) row-wise: s f32 [rows][lds], bias f32 [rows][ldb] or NULL (T5 relative-position bias, CLIP causal
 * mask as -inf), p bf16 [rows][ldp] with columns cols..cols_out-1 zero-filled (K padding of the P·V GEMM). A fully masked row
 * gives zeros. */
int rt_softmax_rows_bias(const float* s, int64_t lds, const float* bias, int64_t ldb, void* p, int64_t ldp,
                         int32_t rows, int32_t cols, int32_t cols_out, float scale, void* stream);
/* T5 v1.1 gated-GELU tail: out[r][c] = x[r][c] · x[r][F+c], bf16 (one half already activated by the GEMM epilogue). */
int rt_gated_mul(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t rows, int32_t F, void* stream);
/* CLIP quick_gelu in place on n bf16 values: x · sigmoid(1.702 x). */
int rt_quick_gelu(void* x, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * CLIP vision encoder (ABI 13; image_encoder.py: `CLIPVisionModelWithProjection`, the image encoder behind the pipeline's
 * ip_adapter_image=). Once per image prompt, outside the loop. Matrix work is rt_gemm_bf16, norms rt_layernorm_modulate.
 * ---------------------------------------------------------------------------------------- */
/* Self-attention with heads of 64, non-causal, no bias (csrc/attention_small_head.hip):
 *   o[b][s][h*64 .. h*64+63] = softmax(scale * q_h k_h^T) v_h        for every batch entry b, head h and row s < S
 * q / k / v: bf16 views of one fused [B][S][ld] buffer (common row stride ld and batch stride stride_b, in elements; ld = 3*H*64 for
 * the fused q|k|v projection), head h at column h*64; o: bf16 [B][S][ldo]. Both products on v_mfma_f32_16x16x32_bf16; scores, row
 * maximum, row sum and accumulators fp32; P rounded to bf16 as the second product's operand; online softmax over key tiles of 64,
 * o normalised once at the end; keys past S are padded inside the kernel and masked. Only rows < S and columns < H*64 of each batch
 * entry of o are written; no atomics: two runs give the same bits. Any 1 <= S <= RT_ATTENTION_HD64_MAX_S. Replaces, with one
 * launch, the per-(batch, head) rt_gemm_bf16 -> rt_softmax_rows_bias -> rt_transpose_bf16 -> rt_gemm_bf16 chain and its
 * [S][S] fp32 score matrix (1536 launches per image for ViT-L/14's 24 layers x 16 heads).
 * Rejected on the host: null pointers, B / S / H < 1, scale <= 0, ld or ldo < H*64, a negative batch stride (RT_E_BADARG);
 * S > RT_ATTENTION_HD64_MAX_S, B or H > 65535 (RT_E_SHAPE); pointers not 16-byte aligned, ld / ldo / a batch stride not a multiple of
 * 8 (RT_E_ALIGN). */
#define RT_ATTENTION_HD64_MAX_S 4096
int rt_attention_hd64(const void* q, const void* k, const void* v, int64_t ld, int64_t stride_b,
                      void* o, int64_t ldo, int64_t stride_ob,
                      int32_t B, int32_t S, int32_t H, float scale, void* stream);
/* im2col of CLIPVisionEmbeddings.patch_embedding (Conv2d(3, d, kernel p, stride p, no bias)), feeding rt_gemm_bf16:
 *   out[b*G*G + gy*G + gx][c*p*p + dy*p + dx] = bf16(x[b][c][gy*p + dy][gx*p + dx]),   columns 3*p*p .. Kp-1 = 0
 * x: f32 (x_f32) or bf16 NCHW [B][3][G*p][G*p], contiguous; out: bf16 [B*G*G][Kp], Kp = 3*p*p rounded up to the GEMM's K % 64
 * (588 -> 640 for p = 14); the weight [d][3][p][p] is reshaped and zero-padded to [d][Kp] once by the caller.
 * Rejected on the host: null pointers, B / G / p < 1, Kp < 3*p*p (RT_E_BADARG); p > 1024, G > 4096, more than 2^31 - 256 16-byte
 * chunks of output (RT_E_SHAPE); Kp % 64, out not 16-byte aligned, x not aligned to its element (RT_E_ALIGN). */
int rt_patchify_nchw(const void* x, int32_t x_f32, void* out, int32_t B, int32_t G, int32_t p, int32_t Kp, void* stream);

/* ------------------------------------------------------------------------------------------
 * SigLIP vision encoder (ABI 15; image_encoder.py: `SiglipVisionModel`, the image encoder of the InstantX IP-Adapter). Once per
 * image prompt, outside the loop. Matrix work is rt_gemm_bf16, norms rt_layernorm_modulate, patches rt_patchify_nchw.
 * ---------------------------------------------------------------------------------------- */
/* Attention with heads of 72, non-causal, no bias, separate query and key counts (csrc/attention_small_head.hip):
 *   o[b][s][h*72 .. h*72+71] = softmax(scale * q_h k_h^T) v_h        for every batch entry b, head h and query row s < Sq, over Sk keys
 * q: bf16 [B][Sq][ldq] with batch stride stride_qb (elements); stride_qb == 0 is allowed: one set of query rows shared by the
 * batch (the probe of the attention-pooling head). k / v: bf16 views of one [B][Sk][ldkv] buffer (common row stride ldkv and batch
 * stride stride_kvb; ldq = ldkv = 3*H*72 for the fused q|k|v projection), head h at column h*72 (144 bytes per head: 16-byte
 * chunks stay aligned); o: bf16 [B][Sq][ldo]. Both products on v_mfma_f32_16x16x32_bf16 (columns 64..71 in a third k-step whose
 * other lanes hold zeros); scores, row maximum, row sum and accumulators fp32; P rounded to bf16 as the second product's operand,
 * the row sum taken from the unrounded P; online softmax over key tiles of 64, o normalised once at the end; keys past Sk are
 * padded inside the kernel and masked; nothing is read outside rows < Sq / Sk and columns < H*72 of the inputs. Only rows < Sq and
 * columns < H*72 of each batch entry of o are written; no atomics: two runs give the same bits, and a row's bits do not depend on
 * the workgroup size the host picks. Any 1 <= Sq, Sk <= RT_ATTENTION_HD72_MAX_S.
 * Rejected on the host: null pointers, B / Sq / Sk / H < 1, scale <= 0, ldq, ldkv or ldo < H*72, a negative batch stride
 * (RT_E_BADARG); Sq or Sk > RT_ATTENTION_HD72_MAX_S, B or H > 65535 (RT_E_SHAPE); pointers not 16-byte aligned, a leading
 * dimension or batch stride not a multiple of 8 (RT_E_ALIGN). */
#define RT_ATTENTION_HD72_MAX_S 1024
int rt_attention_hd72(const void* q, int64_t ldq, int64_t stride_qb,
                      const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
                      void* o, int64_t ldo, int64_t stride_ob,
                      int32_t B, int32_t Sq, int32_t Sk, int32_t H, float scale, void* stream);

/* FlowMatchEulerDiscreteScheduler.step (PIPE:1109; A.6): x = bf16(f32(x) + dsigma·f32(v)), in place; the product and the sum are each
 * rounded to fp32 (no fused multiply-add), as torch computes it. */
int rt_euler_step(void* x, const void* v, float dsigma, int64_t n, void* stream);

/* True-CFG mix of the inpaint pipeline (INP:1264-1270): out = uncond + s·(text − uncond); bf16. */
int rt_cfg_mix(const void* v_uncond, const void* v_text, void* out, float s, int64_t n, void* stream);

/* The step on an fp32 master copy of the latents (pipeline._denoise_eager, through scheduler.step_master_), one kernel. diffusers
 * computes the step in fp32 and rounds the STATE back to bf16 every step; keeping the state in fp32 removes 28 accumulated roundings
 * (the fp32 CPU reference path keeps fp32 throughout). Per element i, all in fp32:
 *   vel  = v_text ? u + s·(t − u) : v          u = v, t = v_text: bf16 widened, under true CFG the halves [negative, positive] of the
 *                                              transformer's output; the mix is never rounded to bf16 (rt_cfg_mix would round it
 *                                              once per step before the fp32 state consumes it); s unused without v_text
 *   r    = x + dsigma·vel
 *   keep = (1 − sigma_next)·src + sigma_next·noise
 *   x[i] = mask ? (1 − m)·keep + m·r : r,  m = mask[i % n_mask]
 *   x_bf16[i] = bf16(x[i]) when given: the copy the next model call reads
 * The three entries below are views of this one step and run instantiations of one kernel: rt_euler_step_f32 has neither v_text nor
 * a mask, rt_cfg_euler_step_f32 has v_text, rt_repaint_euler_step_f32 has the mask (the latent blend of a repaint, LoopExtras.repaint)
 * and v_text or not. With t == u the mix is u exactly, for any s, so rt_cfg_euler_step_f32 is then rt_euler_step_f32.
 * n_mask is n or the per-sample length: one mask serves the batch. keep and the blend are computed without fused multiply-adds, so for
 * finite inputs m = 1 is the step without a mask bit for bit, m = 0 gives keep as torch computes it, and sigma_next = 0 gives src there.
 * NULL x / v (v_uncond) / src / noise / mask, NULL v_text where it is not nullable, n < 1 or n_mask < 1: RT_E_BADARG;
 * n % n_mask != 0: RT_E_SHAPE. */
int rt_euler_step_f32(float* x, const void* v, void* x_bf16 /* nullable */, float dsigma, int64_t n, void* stream);
int rt_cfg_euler_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16 /* nullable */,
                          float s, float dsigma, int64_t n, void* stream);
int rt_repaint_euler_step_f32(float* x, const void* v, const void* v_text /* nullable */, void* x_bf16 /* nullable */,
                              const float* src, const float* noise, const float* mask, float s, float dsigma, float sigma_next,
                              int64_t n, int64_t n_mask, void* stream);
/* The second-order multistep form of the same step (Adams–Bashforth 2 in sigma; scheduler.FlowMatchMultistepScheduler), one more
 * instantiation family of the same kernel. hist is an fp32 buffer of the state's length that holds the velocity of the step before:
 *   vel2 = w != 0 ? vel + w·(vel − hist) : vel        w = dsigma_i / (2·dsigma_{i-1}), 0 for the first step of a run
 *   r    = x + dsigma·vel2                            then the blend and x_bf16 as above
 *   hist = vel                                        under true CFG the mixed fp32 velocity
 * With w == 0 hist is written and never read (it may be uninitialised) and x gets the bits of the entry above that the other
 * arguments select. src / noise / mask are all NULL or all given; without a mask pass n_mask = n.
 * NULL x / v / hist, n < 1, n_mask < 1, a mask without src and noise: RT_E_BADARG; n % n_mask != 0: RT_E_SHAPE.
 * Added without an ABI bump: nothing existing changed. */
int rt_multistep_step_f32(float* x, const void* v, const void* v_text /* nullable */, void* x_bf16 /* nullable */, float* hist, float w,
                          const float* src /* nullable */, const float* noise /* nullable */, const float* mask /* nullable */,
                          float s, float dsigma, float sigma_next, int64_t n, int64_t n_mask, void* stream);
/* Projected guidance (APG, as diffusers' guider is recalled; parity unpinned) in the same step: one more form of the velocity, which
 * needs three sums per SAMPLE over its n_s elements. With p = v_text, u = v_uncond (bf16, widened), all in fp32:
 *   d = (p − u) + beta·diff_old           beta = 0 on the first guided step of a run: diff is then written and never read
 *   a = Σ d²,  b = Σ d·p,  c = Σ p²
 *   k = tau > 0 and a > tau² ? tau/√a : 1;   alpha = c > 0 ? k·b/c : 0;   e = (eta − 1)·alpha
 *   vel = p + s_minus_1·(k·d + e·p)        then vel2, r, hist, the blend and x_bf16 as in rt_multistep_step_f32
 * Two launches, no atomics. rt_guidance_reduce_f32 writes d to diff (fp32 [B][n_s]) and, per chunk of RT_GUIDE_CHUNK elements of a
 * sample, one (a, b, c) triple to partials (fp32 [B][ceil(n_s / RT_GUIDE_CHUNK)][3], rt_guidance_ws_bytes(B, n_s) bytes; 0 for sizes
 * < 1). Where an element is added is a function of its index inside the sample alone: thread (i / 4) % 256 of chunk i / 4096 takes it
 * as its (4·((i % 4096) / 1024) + i % 4)-th term, a wave adds its lanes in a fixed xor butterfly, one thread adds the four waves. So
 * the sums have the same bits with 8- and 16-byte loads (n_s % 4 == 0, v_* 8-byte and diff 16-byte aligned) and one element at a
 * time, and do not depend on B or on the other samples. rt_projected_step_f32 adds a sample's partials in index order in double,
 * forms k and e in double, rounds each to float once (every workgroup of a sample: the same bits) and steps. v_uncond is not read by
 * it (d is in diff); it is in the list so that the pair takes one set of arguments. hist / src / noise / mask are optional as above;
 * m = mask[i % n_mask] over the flat index i of [B][n_s]. 16-byte groups are taken only when n_s % 4 == 0, so none straddles a sample.
 * NULL v_uncond / v_text / diff / partials (/ x), B < 1, n_s < 1, n_mask < 1, a mask without src and noise: RT_E_BADARG;
 * B > 65535, (B·n_s) % n_mask != 0: RT_E_SHAPE. Added without an ABI bump: nothing existing changed. */
#define RT_GUIDE_CHUNK 4096
int64_t rt_guidance_ws_bytes(int32_t B, int64_t n_s);
int rt_guidance_reduce_f32(const void* v_uncond, const void* v_text, float* diff, float beta, float* partials, int32_t B, int64_t n_s,
                           void* stream);
int rt_projected_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16 /* nullable */, const float* diff,
                          const float* partials, float s_minus_1, float eta, float tau, float* hist /* nullable */, float w,
                          const float* src /* nullable */, const float* noise /* nullable */, const float* mask /* nullable */,
                          float dsigma, float sigma_next, int32_t B, int64_t n_s, int64_t n_mask, void* stream);
/* Stochastic sampling (the scheduler's stochastic_sampling switch; diffusers' rule at eta = 1, recalled, parity unpinned): one more form
 * of the same step. vel is the velocity the step already has (plain, the mix, or the projected form); per element, every product and
 * sum rounded once:
 *   x0 = x − sigma·vel
 *   e  = x0 + vel                                             only where eta < 1: the noise the state holds at sigma
 *   n  = eta < 1 ? sqrt_1m_eta2·e + eta·z : z                 z: a fresh standard normal
 *   r  = (1 − sigma_next)·x0 + sigma_next·n                   then the blend and x_bf16 as above
 * sigma_next = 0 (the last step) gives r = x0: no z is drawn and rng is not read (it may be NULL). eta lies in (0, 1];
 * sqrt_1m_eta2 = sqrt(1 − eta²) comes from the host, formed in double.
 * z is drawn inside the kernel from Philox4x32-10 (csrc/philox.h): one call per group of four consecutive elements of a sample,
 *   counter = (g low, g high, step, subsequence)   g = (index inside the sample) / 4
 *   key     = (seed low, seed high ^ 0x53544F43)
 *   u = ((w >> 8) + 0.5)·2^-24;  z0 = r·cos θ, z1 = r·sin θ with r = sqrt(−2 ln u(w0)), θ = 2π·u(w1);  z2, z3 from w2, w3
 * with (seed, subsequence) = rng[b][0..1] (int64 [B][2], device memory) of the element's sample b. z depends on (seed, subsequence,
 * step, index inside the sample) alone: not on B, on the other samples, or on which path of the kernel takes the element (16-byte
 * groups only when n_s % 4 == 0 and the pointers are aligned; the one-element path runs Philox for the element's group and picks its
 * lane). There is no noise tensor and no generator state: step is a kernel scalar, the scheduler's absolute step index.
 * rt_normal_fill_f32 writes that z to out (fp32 [B][n_s]), the same bits.
 * The mask's rule is m = mask[i % n_mask] over the flat index i of [B][n_s], as in rt_projected_step_f32.
 * NULL x / v (v_uncond, v_text, diff, partials) / out, NULL rng with sigma_next != 0, B < 1, n_s < 1, n_mask < 1, a mask without src
 * and noise, eta outside (0, 1], step < 0: RT_E_BADARG; B > 65535, (B·n_s) % n_mask != 0: RT_E_SHAPE.
 * Added without an ABI bump: nothing existing changed. */
int rt_stochastic_step_f32(float* x, const void* v, const void* v_text /* nullable */, void* x_bf16 /* nullable */,
                           const float* src /* nullable */, const float* noise /* nullable */, const float* mask /* nullable */,
                           const int64_t* rng, float s, float sigma, float sigma_next, float eta, float sqrt_1m_eta2, int32_t step,
                           int32_t B, int64_t n_s, int64_t n_mask, void* stream);
int rt_projected_stochastic_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16 /* nullable */, const float* diff,
                                     const float* partials, float s_minus_1, float eta_guidance, float tau,
                                     const float* src /* nullable */, const float* noise /* nullable */, const float* mask /* nullable */,
                                     const int64_t* rng, float sigma, float sigma_next, float eta, float sqrt_1m_eta2, int32_t step,
                                     int32_t B, int64_t n_s, int64_t n_mask, void* stream);
int rt_normal_fill_f32(float* out, const int64_t* rng, int32_t B, int64_t n_s, int32_t step, void* stream);

/* _pack_latents / _unpack_latents (PIPE:550-570): [B][C][2h][2w] <-> [B][h*w][4C], channel order (c,dy,dx).
 * unpack also applies z/scaling + shift (PIPE:1137) and writes NHWC bf16 [B][H2][W2][C]. */
int rt_pack_latents(const void* nchw, void* packed, int32_t B, int32_t C, int32_t H2, int32_t W2, void* stream);
int rt_unpack_latents(const void* packed, void* nhwc, int32_t B, int32_t C, int32_t H2, int32_t W2,
                      float inv_scale, float shift, void* stream);

/* Elementwise helpers on the path. */
int rt_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);
int rt_cast_bf16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* hi = bf16(f(x)), lo = bf16(f(x) - hi), f = SiLU or identity: lets the adaLN projections of ALL denoising steps run as one
 * M = steps GEMM on MFMA (hi pass + lo pass accumulate) with fp32-activation accuracy (A.1 step 1, hoisted out of PIPE:1017). */
int rt_silu_split_bf16(const float* x, void* hi, void* lo, int64_t n, int32_t apply_silu, void* stream);
/* y[b][r][:] (+)= alpha · rowscale[r] · x[b][r][:]  — PIPE:1060-1087 masked sum over text lines; x bf16, y bf16 or f32 (y_f32). */
int rt_masked_accumulate(const void* x, void* y, const float* rowscale, float alpha,
                         int32_t batch, int32_t rows, int32_t D, int32_t accumulate, int32_t y_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * AutoencoderKL (PIPE:467,705,711 encode; PIPE:1139 decode; Appendix A.7).
 * Activations are zero-haloed NHWC bf16: [B][H+2][W+2][C]; the halo is allocated zeroed by the caller and never
 * written by these kernels, so 3x3 gathers need no bounds checks.
 * ---------------------------------------------------------------------------------------- */
/* GroupNorm(G groups, eps, affine gamma/beta bf16 [C]) + optional SiLU over the interior of x -> interior of y.
 * stats_ws: device scratch of rt_groupnorm_ws_bytes(B,H,W,G) bytes (8-byte aligned; need not be zeroed). All sums run in a
 * fixed order (no atomics): results are bitwise reproducible. C % 8 == 0, C % G == 0, 256 % (C/8) == 0, G <= 512, B·H <= 65535;
 * anything else is RT_E_SHAPE with nothing queued on the stream. */
int64_t rt_groupnorm_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t G);
int rt_groupnorm_silu_nhwc(const void* x, void* y, const void* gamma, const void* beta, void* stats_ws,
                           int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, float eps, int32_t silu, void* stream);
/* 3x3 / 1x1 convolution as implicit GEMM on MFMA. x haloed [B][Hs+2][Ws+2][Cin], w bf16 [Cout][k][k][Cin] (repacked
 * from OIHW), y haloed [B][Ho+2][Wo+2][Cout] bf16|f32, res (optional) like y in bf16.
 *   stride 1: pad k/2; upsample2x fuses a nearest-2x Upsample2D in front (Ho = 2Hs)
 *   stride 2: k = 3, pad (0,1,0,1) = diffusers Downsample2D (Ho = Hs/2)
 * Cin % 64 == 0 (callers zero-pad channels), Cout % 4 == 0.
 * Rejected on the host, before anything is queued: null x / w / y or a size < 1 (RT_E_BADARG); a kernel size, stride or channel
 * count outside the above, odd Hs / Ws with stride 2 (RT_E_SHAPE); x / w / y not 16-byte aligned, or a bias or res that is given
 * and not 8-byte aligned — whichever kernel serves the call (RT_E_ALIGN). */
int rt_conv2d_nhwc(const void* x, const void* w, const void* bias, const void* res, void* y,
                   int32_t B, int32_t Hs, int32_t Ws, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                   int32_t upsample2x, int32_t out_f32, void* stream);
/* Which kernel serves rt_conv2d_nhwc's stride-1, non-upsampling, bf16-output calls with Cout >= 64 (speed only: both accumulate every
 * output element in the same K order, results are bit-identical): 1 (default, env RT_CONV_GEMM) = rt_gemm_bf16's convolution form,
 * 0 = conv_nhwc_kernel. mode >= 0 sets it, mode < 0 only queries; returns the previous mode. */
int rt_conv2d_variant(int32_t mode);
/* Row softmax for the VAE mid-block attention (1 head, Dh = 512, computed as GEMM -> softmax -> GEMM):
 * p[r][:] = softmax(scale * s[r][:]), f32 in, bf16 out. cols % 4 == 0. */
int rt_softmax_rows(const float* s, void* p, int32_t rows, int32_t cols, float scale, void* stream);
/* Mid-block attention of the AutoencoderKL, flash-style (A.7: Attention(C, 1 head) over the H*W positions of the 1/8-scale grid;
 * PIPE:1139 decode, PIPE:467,705,711 encode): o = softmax(q k^T * scale) v with ONE head of C channels, C in {128, 256, 512}.
 * q/k/v: bf16 [B][HW][>=C] views with a common row stride ld and batch stride (elements) — the fused q|k|v projection buffer;
 * o: bf16 [B][HW][ldo]. HW % 32 == 0. No (HW x HW) buffer exists: the channels are split over the waves of a workgroup, which
 * exchange partial scores through LDS (csrc/vae_attention.hip). Replaces GEMM -> rt_softmax_rows -> rt_transpose_bf16 -> GEMM. */
int rt_vae_attention(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                     int32_t B, int32_t HW, int32_t C, float scale, void* stream);
/* out[c][r] = in[r][c], bf16 (V^T for the P·V GEMM). */
int rt_transpose_bf16(const void* in, void* out, int32_t R, int32_t C, int64_t ld_in, int64_t ld_out, void* stream);
/* Decoder tail: haloed NHWC f32 [B][H+2][W+2][Cp] -> NCHW f32 [B][C][H][W] (nchw, optional) and/or uint8 HWC
 * round(clamp(x/2+0.5,0,1)*255) (u8, optional) = VaeImageProcessor.postprocess (PIPE:1140). */
int rt_image_out(const float* x, float* nchw, uint8_t* u8, int32_t B, int32_t H, int32_t W, int32_t Cp, int32_t C, void* stream);
/* Encoder head / readout: NCHW f32 <-> haloed NHWC bf16 with channel padding to Cp. */
int rt_nchw_to_haloed_nhwc(const float* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Cp, void* stream);
int rt_haloed_nhwc_to_nchw(const void* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Cp, void* stream);
/* _unpack_latents + z/scaling + shift (PIPE:1136-1137) straight into the decoder's haloed NHWC input. */
int rt_unpack_latents_haloed(const void* packed, void* y, int32_t B, int32_t C, int32_t H2, int32_t W2, int32_t Cp,
                             float inv_scale, float shift, void* stream);


/* Hint-side resizes of the pipelines on the device, with torch.nn.functional.interpolate's rules
 * (align_corners=False, no antialias; the same fp32 expression order as ATen, so results are bit-identical):
 *   PIPE:1010-1012  regional mask / 255 -> bilinear x 1/16          (in_u8 = 1, in_scale = 255, scale = 1/16)
 *   INP:813         inpaint mask -> nearest, to the latent grid      (bilinear = 0, scale = 0: ratio = in/out)
 * `in`: uint8 (in_u8, divided by in_scale first) or f32 [planes][H][W]; out f32 [planes][OH][OW]; scale_h/scale_w > 0 are the
 * `scale_factor` torch was given (ratio = 1/scale), 0 = derive the ratio from the sizes. */
int rt_resize2d(const void* in, int32_t in_u8, float in_scale, float* out, int32_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW,
                float scale_h, float scale_w, int32_t bilinear, void* stream);
/* PIPE:645-654 / INP:640-647: out = 0.10 * latents + noise where the glyph mask (any channel of image > 0), bilinearly resized
 * to the latent grid, is > 0; noise elsewhere. image f32 [B][Cimg][H][W]; latents, noise, out f32 [B][Cl][OH][OW]. */
int rt_glyph_blend(const float* image, const float* latents, const float* noise, float* out, int32_t B, int32_t Cimg, int32_t H, int32_t W,
                   int32_t Cl, int32_t OH, int32_t OW, void* stream);

/* ------------------------------------------------------------------------------------------
 * Caller-side hint preparation on the device (csrc/hints.hip).
 * ---------------------------------------------------------------------------------------- */
/* cv2.Canny(image, low, high) of infer.py:16-22 (called at infer.py:98-100 on the rendered glyph) as cv::Canny documents it —
 * 3x3 Sobel with replicated borders taken per channel (the channel with the largest |dx|+|dy| supplies the gradient, first
 * channel on ties; no gray conversion), L1 magnitude, 4-sector non-maximum suppression with cv::Canny's tie rules, double
 * threshold, 8-connected hysteresis — bit-identical to reptext_amd/hints.py::canny_edges (parity with OpenCV itself is unpinned).
 * img: uint8 [H][W][C] (C = 1..4, interleaved); out: uint8 [H][W][out_channels], every channel = edge map {0,255}, or
 * 255 - edges when `invert` (infer.py:20-22: the hint is the inverted map repeated over 3 channels).
 * ws: rt_canny_ws_bytes(H, W) bytes of scratch, 256-byte aligned; need not be zeroed. Four kernels on `stream`, no host
 * round trip (hysteresis = one workgroup's breadth-first search over index frontiers in ws). */
int64_t rt_canny_ws_bytes(int32_t H, int32_t W);
int rt_canny_u8(const uint8_t* img, int32_t H, int32_t W, int32_t C, float low, float high, uint8_t* out, int32_t out_channels,
                int32_t invert, void* ws, int64_t ws_bytes, void* stream);
/* VaeImageProcessor.preprocess (PIPE:680,694,970) for uint8 images that already have the target size: img [B][H][W][C] ->
 * out f32 [B][C][H][W] = x / 255, then 2x - 1 when `normalize` (the same fp32 roundings numpy/torch take: bit-identical). */
int rt_preprocess_u8(const uint8_t* img, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t normalize, void* stream);

/* ------------------------------------------------------------------------------------------
 * The photo flow's pixel work (reptext_amd/pipeline_photo.py; csrc/photo.hip): crop + antialiased resample, the mask's
 * feather, and the blend of the result into the full-size photo. Added entries; the ABI revision is unchanged.
 * ---------------------------------------------------------------------------------------- */
#define RT_RESIZE_AA_MAX_SCALE 16   /* rt_resize_aa: the window may be at most this many times the output, per axis */
#define RT_BLUR_MAX_RADIUS 96       /* rt_gaussian_blur_f32: ceil(3·sigma) may be at most this, i.e. sigma <= 32 */
/* Crop + antialiased separable bilinear resample: the window (x0, y0, cw, ch) of `in` — uint8 [H][W][C] interleaved (in_u8, a sample
 * is x/255) or f32 [C][H][W] planar — to out f32 [C][OH][OW] = mul·r + add. The filter is ATen's _upsample_bilinear2d_aa
 * (align_corners = False) applied to the window as if it were the whole image: per axis scale = in/out, support = max(scale, 1),
 * center = scale·(i + 0.5), taps max(0, int(center − support + 0.5)) .. min(in, int(center + support + 0.5)), triangle weights
 * normalised to sum 1 (formed in fp64, rounded to fp32 once; fp32 accumulation, along x then along y). Upscaling is plain
 * bilinear; a window resampled to its own size is mul·(x/255) + add bit for bit (each operation rounded once).
 * ws: rt_resize_aa_ws_bytes(C, ch, OW) bytes, 16-byte aligned (the pass along x). Two kernels on `stream`.
 * Rejected on the host: null in / out / ws, a size < 1, a window not inside the image, ws too small or unaligned (RT_E_BADARG);
 * C not 1 or 3, cw > RT_RESIZE_AA_MAX_SCALE·OW or ch > RT_RESIZE_AA_MAX_SCALE·OH, ch or OH > 65535 (RT_E_SHAPE). */
int64_t rt_resize_aa_ws_bytes(int32_t C, int32_t ch, int32_t OW);
int rt_resize_aa(const void* in, int32_t in_u8, int32_t C, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t cw, int32_t ch, float* out,
                 int32_t OH, int32_t OW, float mul, float add, void* ws, int64_t ws_bytes, void* stream);
/* Separable Gaussian blur of one f32 plane [H][W] (the mask's feather): radius R = ceil(3·sigma), weights exp(−k²/(2·sigma²)) in
 * fp32 normalised to sum 1, replicated borders, rows then columns. An output farther than R (Chebyshev) from every non-zero input
 * is exactly 0, and one whose inputs within R are all 1 is exactly 1 (the taps are added from the outermost pair inwards and the
 * centre weight is 1 minus the fp32 sum of the others in that order). ws: H·W·4 bytes (the row pass); out must not be in.
 * Rejected on the host: null pointers, H / W < 1, sigma <= 0 or NaN, ws too small, out == in (RT_E_BADARG); 3·sigma >
 * RT_BLUR_MAX_RADIUS, H > 65535 (RT_E_SHAPE). */
int rt_gaussian_blur_f32(const float* in, float* out, int32_t H, int32_t W, float sigma, void* ws, int64_t ws_bytes, void* stream);
/* out uint8 [H][W][C] = photo uint8 [H][W][C] outside the rectangle (x0, y0, cw, ch); inside it, with gen f32 [C][ch][cw] in the
 * decoder's range and alpha f32 [ch][cw]: g = clamp(gen/2 + 0.5, 0, 1)·255 (rt_image_out's expression), v = (1 − a)·src + a·g with
 * every product and sum rounded once, out = rint(v) (half to even), clamped. alpha = 0 is the photo's byte, alpha = 1 the byte
 * rt_image_out writes for gen. Any W and any rectangle: 16-byte loads and stores where photo and out are 16-byte aligned, byte
 * accesses otherwise and for the last (H·W·C) % 16 bytes, in one launch. out must not overlap photo.
 * Rejected on the host: null pointers, a size < 1, a rectangle not inside the photo (RT_E_BADARG); C not 1 or 3 (RT_E_SHAPE). */
int rt_composite_u8(const uint8_t* photo, uint8_t* out, int32_t H, int32_t W, int32_t C, int32_t x0, int32_t y0, int32_t cw, int32_t ch,
                    const float* gen, const float* alpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REPTEXT_HIP_H */
