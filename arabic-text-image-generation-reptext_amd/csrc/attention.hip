// rt_attention_fwd — joint text+image attention of the MMDiT blocks: softmax(Q·Kᵀ·scale)·V, non-causal,
// no mask, head dim 128, bf16 in/out, fp32 scores/statistics/accumulators. Flash-style: the S×S score
// matrix never leaves the CU. Reference: torch SDPA as called by diffusers' FluxAttnProcessor (SURVEY.md
// Appendix A.1 step 6 / A.2), reached from controlnet_flux.py:343-348,376-380 and PIPE:1092.
//
// Work item = 128 query rows of one (batch, head); a workgroup = 4 waves, wave w owns query rows 32w..32w+31.
// Keys/values arrive in 64-row tiles by LDS-DMA into a 2-deep ring (K 16 KiB + V 16 KiB per slot).
//
// Both products run on v_mfma_f32_32x32x16_bf16 with the QUERY index on the lane:
//   Sᵀ[key][q]  = K · Qᵀ      A = K rows from LDS (ds_read_b128), B = Q rows held in registers
//   Oᵀ[d][q]   += Vᵀ · Pᵀ     A = Vᵀ via ds_read_b64_tr_b16 (hardware transpose), B = the Sᵀ accumulator
//                             registers themselves, exponentiated and packed to bf16 (no LDS round trip)
// so the softmax max/sum of a query row are lane-local apart from one lane<->lane+32 exchange, and the
// per-row rescale of O is a per-lane scalar multiply.
//
// Schedule inside a wave (per 64-key tile, two 32-key halves h0, h1):
//   Sᵀ(h0) | Sᵀ(h1) ∥ numerators of h0 | check h0 | Oᵀ += Vᵀ(h0)·Pᵀ(h0) ∥ numerators of h1 | check h1 | Oᵀ += Vᵀ(h1)·Pᵀ(h1)
// The numerators of a half are computed SPECULATIVELY against the running max m_run while the matrix pipe works on the
// next product; the row max of the half is taken beside them and checked afterwards. Only when some row's max outgrew
// m_run by more than RESCALE_THR (rare after the first tiles) a fix-up block rescales O and l and recomputes that half's
// numerators against the new max — so the common path has no branch between an MFMA chain and the vector work that
// overlaps it, and every numerator that reaches an MFMA was formed against the max O is normalised with.
//
// Placement (speed only, never correctness): the grid is one-dimensional per batch entry. Workgroups are dealt
// round-robin over the 8 XCDs, so blockIdx.x & 7 labels the XCD group; each group owns a CONTIGUOUS run of the
// (head, query block) items, i.e. whole heads (3 of 24 per XCD): K/V of a head are fetched into one XCD's L2 only.
//
// Key-split tail (attention_split.h, shared with attention_v3.hip): the items of the last, partly filled round of an XCD
// group are not run by full-length workgroups; their key tiles are dealt to all `spx` workgroup slots (2 per CU) in equal
// runs. A workgroup that covers only part of an item writes its unnormalised (m, l, Oᵀ) to a workspace record; the last
// one to finish an item combines its records in run order.
//
// rt_attention_fwd_grouped is the same kernel instantiated with GROUPED = true (region-masked attention for per-line prompts): keys in
// tile-aligned groups, one visibility word per query row, hidden lanes' scores set to -inf under a wave-uniform branch. Everything it adds
// stands under `if constexpr (GROUPED)`; the dense instantiation is the code it was.
//
// rt_attention_fwd_keyed is the third instantiation (KEYED: region isolation for per-line prompts): every KEY carries a class id byte and a
// row sees key j iff bit class[j] of its word is set. Per tile a lane holds the class of key 64t + lane (loaded one tile ahead); the
// distinct classes of the tile are walked with readlane / ballot (wave-uniform, one turn per class present) into a 64-bit visibility
// mask per row. A tile of one class takes the grouped code's hide branch; only a tile of several classes pays a bit test per score.
// Everything it adds stands under `if constexpr (KEYED)`.
//
// rt_attention_fwd_grouped_biased / rt_attention_fwd_keyed_biased are the fourth and fifth instantiation (BIASED: a strength per line
// prompt): an fp32 bias per key CLASS (the group index / the class byte) is added to the logits of that class's keys. The kernel works
// on RAW scores (scale_log2 is applied inside the exp2's fma), so a table entry is converted where it is read, once per class, to
// raw-score units (bias / scale). It is read by a scalar load — grouped: when the group advances; keyed: in the class walk — and only
// for a class whose bit is set in `nz`, the 32-bit set of the classes with a non-zero entry, taken once per workgroup: nothing is
// held per lane. The bias is added BEFORE the half's row maximum is taken, so that the speculative numerators, decide, the deferred
// rescale and the key-split records see an ordinary score: a record's m simply includes the bias, and the combine (which weighs
// records by exp2(m_j - M) and knows nothing of how a score came about) needs no change — checked against attention_split.h.
// A hidden or ragged score is -inf before the add and after it. A tile whose bias is 0 executes what its unbiased sibling executes.
// A keyed tile of several classes of which one has a bias (never in the pipeline's use: biased classes are text tokens, which fill
// whole tiles) loads, per lane, the class and the bias of key 64t + lane again and hands each score its own key's through v_readlane
// (no LDS memory: the 64 KiB are taken), out of line. Everything it adds stands under `if constexpr (BIASED)`.
//
// rt_attention_fwd_keyed_self is the sixth instantiation (SELF: perturbed-attention guidance): the keyed rule, and every row also sees
// the key of its own index. A wave's 32 query rows q0 + 32·wave .. +31 lie inside ONE key tile (q0 is a multiple of 128, a tile holds 64
// keys), so only that tile differs, under a wave-uniform test: after the class walk each row ORs bit (row - 64t) into its 64-bit mask
// (the row clamped as the word load is), and the tile takes the per-score path whenever a row hides part of it. Every other tile
// executes what the keyed instantiation executes; a key-split run that sees nothing already weighs 0 in the combine. Everything it
// adds stands under `if constexpr (SELF)`.
//
// LDS image of a K or V tile: 64 rows × 256 B; 16-B chunk c of row r lives at 256·r + 16·(c ^ f(r)),
// f(r) = ((r&3)<<2) | ((r>>2)&3): conflict-free for the row reads (K) and the transposed reads (V).
// LDS-DMA writes lane-linear, so the XOR is applied to each lane's source address.
#include "attention_split.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int DH = 128;
constexpr int BQ = 128;       // query rows per work item
constexpr int BKV = 64;       // keys per tile
constexpr int TILE_B = BKV * DH * 2;   // 16 KiB
constexpr int ATT_THREADS = 256;
constexpr float RESCALE_THR = 6.0f;   // log2 units: P <= 64 between rescales
constexpr int REC_WAVE_B = 64 * 64 * 4 + 64 * 8;   // one wave's partial: Oᵀ (64 registers × 64 lanes, fp32) + (m, l) per lane
constexpr int REC_B = 4 * REC_WAVE_B;              // 67 584 B per (workgroup, segment)

__host__ __device__ inline int group_slots(const SplitGeom& G, int xcd) {
  const GroupCut c = group_cut(G, xcd);
  return c.nfull + (c.rem ? G.spx : 0);
}

// rt_attention_fwd_grouped: the keys fall into n contiguous groups whose ends are multiples of BKV (the last is S), so a key tile lies
// in ONE group; a query row sees a tile iff the group's bit is set in its word of row_vis. By value in the kernel arguments: the group
// of a tile is found with scalar loads and compares, nothing per lane but the bit test.
constexpr int MAX_GROUPS = 32;
struct KeyGroups {
  int32_t end[MAX_GROUPS];
  int32_t n;
  const uint32_t* row_vis;   // [B][S], batch stride stride_vis_b (0: one table)
  int64_t stride_vis_b;
};
struct NoGroups {};
// rt_attention_fwd_keyed: a class id (0..31) per key, read a byte at a time: no alignment or padding is asked of the table.
struct KeyClasses {
  const uint32_t* row_vis;   // [B][S], batch stride stride_vis_b (0: one table)
  int64_t stride_vis_b;
  const uint8_t* key_class;  // [B][S], batch stride stride_class_b (0: one table)
  int64_t stride_class_b;
};
// the biased entries: their sibling's record and the bias table, fp32 [B][MAX_GROUPS] in natural-log units, one entry per key class
struct KeyBias {
  const float* key_bias;     // batch stride stride_bias_b (0: one table)
  int64_t stride_bias_b;
};
struct NoBias {};
struct KeyGroupsBiased : KeyGroups, KeyBias {};
struct KeyClassesBiased : KeyClasses, KeyBias {};
enum { DENSE_MODE = 0, GROUPED_MODE = 1, KEYED_MODE = 2, GROUPED_BIASED_MODE = 3, KEYED_BIASED_MODE = 4, KEYED_SELF_MODE = 5 };
template <int MODE> struct MaskArg { using type = NoGroups; };
template <> struct MaskArg<GROUPED_MODE> { using type = KeyGroups; };
template <> struct MaskArg<KEYED_MODE> { using type = KeyClasses; };
template <> struct MaskArg<GROUPED_BIASED_MODE> { using type = KeyGroupsBiased; };
template <> struct MaskArg<KEYED_BIASED_MODE> { using type = KeyClassesBiased; };
template <> struct MaskArg<KEYED_SELF_MODE> { using type = KeyClasses; };
// Running maximum a grouped row starts with: finite, so that a hidden score (-inf) gives exp2(-inf - M0) = 0 and not exp2(NaN), and
// so far below any score that the first visible one rescales the (all-zero) state by exp2(M0 - m) = 0.
constexpr float GROUPED_M0 = -1.0e30f;

template <int MODE>
__global__ __launch_bounds__(ATT_THREADS, 2) void attention_fwd_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, bf16_t* O,
    int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob, float scale_log2, const SplitGeom G,
    const int row_lo, const int row_hi, int* counters, char* records,
    const typename MaskArg<MODE>::type KG) {
  constexpr bool SELF = MODE == KEYED_SELF_MODE;
  constexpr bool GROUPED = MODE == GROUPED_MODE || MODE == GROUPED_BIASED_MODE, KEYED = MODE == KEYED_MODE || MODE == KEYED_BIASED_MODE || SELF;
  constexpr bool MASKED = MODE != DENSE_MODE, BIASED = MODE == GROUPED_BIASED_MODE || MODE == KEYED_BIASED_MODE;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_B];   // [slot][K|V]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hh = lane >> 5;
  const int S = G.S;
  const int ntiles = G.ntiles;

  // ---- which run of (item, key tile) pairs is this workgroup's? (scalar)
  const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3, b = (int)blockIdx.y;
  const GroupCut cut = group_cut(G, xcd);
  int run_lo, run_hi;            // in units of key tiles, relative to the first item this workgroup touches
  int item0;                     // that first item
  int jpart = -1;                // index among the `spx` splitting workgroups, -1 for a full-length workgroup
  if (slot < cut.nfull) {
    item0 = cut.start + slot;
    run_lo = 0;
    run_hi = ntiles;
  } else {
    jpart = slot - cut.nfull;
    if (cut.rem == 0 || jpart >= G.spx) return;
    const SplitRun run = split_run(G, cut, jpart);
    item0 = cut.start + cut.nfull + run.i0;
    run_lo = run.lo - run.i0 * ntiles;
    run_hi = run.hi - run.i0 * ntiles;   // may exceed ntiles: the run continues into item0 + 1
  }

  // ---- per-lane constants that do not depend on the item
  // staging: wave w stages pieces 4w..4w+3 (4 rows each) of K and of V; K and V share row/chunk offsets.
  const int srow = lane >> 4;                 // row inside a piece
  const int spc = lane & 15;                  // physical chunk written by this lane
  uint32_t soff[4];                           // BYTE offset of (row, logical chunk) from the tile's first row
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row_t = (wave * 4 + p) * 4 + srow;          // row inside the tile
    soff[p] = ((uint32_t)row_t * (uint32_t)ld + (uint32_t)((spc ^ swz(row_t)) << 3)) * 2u;
  }
  // K row read: row = 32kt + l31, chunk = 2ks + hh  ->  l31*256 + ((2ks+hh) ^ swz(l31))*16  (+ kt*8192)
  lds_cptr kp[8];
  {
    const int ksw = swz(l31);                 // swz depends on row & 15 only
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kp[ks] = (lds_cptr)smem + (l31 * 256 + (((2 * ks + hh) ^ ksw) << 4));
  }
  // V transposed read: 16-lane group g = lane>>4 (hh = g>>1, d half g&1); lane 4q+p of the group supplies row r0+q,
  // chunk c0+(p>>1), 8-byte half p&1. Rows: first block 4hh+tq, second block +8 (per k-step: + 32kt + 16s).
  const int tq = (lane >> 2) & 3, tp = lane & 3;
  const int tg1 = (lane >> 4) & 1;
  lds_cptr vp[2][4];
  {
    const int cl = tg1 * 2 + (tp >> 1);
    const int rl0 = 4 * hh + tq, rl1 = rl0 + 8;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      vp[0][dt] = (lds_cptr)smem + TILE_B + rl0 * 256 + (((dt * 4 + cl) ^ swz(rl0)) << 4) + 8 * (tp & 1);
      vp[1][dt] = (lds_cptr)smem + TILE_B + rl1 * 256 + (((dt * 4 + cl) ^ swz(rl1)) << 4) + 8 * (tp & 1);
    }
  }

  // biased: the table is in natural-log units and a raw score is multiplied by scale_log2 = scale·log2(e) inside the exp2, so an entry
  // times bias_mul = 1 / scale is a bias in raw-score units. nz: bit c set = class c's entry is not zero (scalar).
  // Only nz lives across the tile loop; the table's address and bias_mul are formed again where a bias is read (rare).
  [[maybe_unused]] uint32_t nz = 0;
  [[maybe_unused]] auto bias_at = [&](uint32_t c) -> float {      // c wave-uniform: a scalar load
    if constexpr (BIASED) return KG.key_bias[b * KG.stride_bias_b + c] * (1.4426950408889634f / scale_log2);
    return 0.f;
  };
  if constexpr (BIASED) nz = (uint32_t)__ballot(lane < MAX_GROUPS && KG.key_bias[b * KG.stride_bias_b + (lane & (MAX_GROUPS - 1))] != 0.f);
  // a tile's bias state in one scalar word: 0 = no key of the tile has a bias; MIXED_BIAS (a NaN pattern, no finite bias) = a keyed tile
  // of several classes with a bias among them; else the bits of the tile's one bias
  constexpr uint32_t MIXED_BIAS = 0x7fc00000u;
  [[maybe_unused]] auto bias_word = [&](uint32_t c) -> uint32_t { return ((nz >> c) & 1u) ? __builtin_bit_cast(uint32_t, bias_at(c)) : 0u; };

  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;

  for (int seg = 0; seg < 2; ++seg) {
    // ---- segment = the part of this workgroup's run that lies inside one item
    const int item = item0 + seg;
    const int tb = seg == 0 ? run_lo : 0;
    const int te = seg == 0 ? min(run_hi, ntiles) : run_hi - ntiles;
    if (te <= tb) break;
    const int head = item / G.nqb;
    const int q0 = (item - head * G.nqb) * BQ;
    // rt_attention_fwd_rows: an item without a query row in [row_lo, row_hi) is nobody's work. The test depends on the item alone, so
    // every workgroup that holds a piece of a split item decides alike and the item's tickets are either all drawn or none.
    if (q0 + BQ <= row_lo || q0 >= row_hi) continue;
    const bf16_t* Qb = Q + b * stride_b + head * DH;
    const bf16_t* Kb = K + b * stride_b + head * DH;
    const bf16_t* Vb = V + b * stride_b + head * DH;

    // LDS-DMA by buffer_load ... lds: 4-SGPR descriptor per operand + the lane's loop-invariant 32-bit byte offset + the tile's
    // byte offset in an SGPR — no per-tile vector address arithmetic. num_records = 2^32-1: rows are clamped here, not by the
    // range check (the host checks (S + 64) * ld * 2 < 2^31).
    const rt_srd_t rsrcK = rt_make_srd(Kb), rsrcV = rt_make_srd(Vb);
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);          // LDS byte address of the ring
    const int tile_stride_b = BKV * (int)ld * 2;
    // One branch for the whole tile, the ragged case out of line: a taken branch costs the wave an instruction-buffer refill, and the
    // common path of the tile loop should not contain any (see RT_RARE).
    auto stage = [&](int sl, int tix, bool clamp) {
      const uint32_t kb = lds0 + sl * 2 * TILE_B;
      if (RT_RARE(clamp)) {   // ragged last tile: rows past the end re-read row S-1 (masked later)
        const int kv0 = tix * BKV;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int row_t = (wave * 4 + p) * 4 + srow;
          const uint32_t off = ((uint32_t)(min(kv0 + row_t, S - 1) - kv0) * (uint32_t)ld + (uint32_t)((spc ^ swz(row_t)) << 3)) * 2u;
          rt_dma16_asm(rsrcK, kb + (wave * 4 + p) * 1024, off, (uint32_t)(tix * tile_stride_b));
          rt_dma16_asm(rsrcV, kb + TILE_B + (wave * 4 + p) * 1024, off, (uint32_t)(tix * tile_stride_b));
        }
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          rt_dma16_asm(rsrcK, kb + (wave * 4 + p) * 1024, soff[p], (uint32_t)(tix * tile_stride_b));
          rt_dma16_asm(rsrcV, kb + TILE_B + (wave * 4 + p) * 1024, soff[p], (uint32_t)(tix * tile_stride_b));
        }
      }
    };

    __syncthreads();                            // previous segment's LDS reads (tiles, ticket word) are done
    stage(0, tb, (tb + 1) * BKV > S);     // first tile in flight before the Q loads are waited for

    // ---- Q fragments (B operand of Sᵀ = K·Qᵀ): lane holds Q[q][16ks + 8hh .. +7]
    bf16x8 qf[8];
    {
      const int qrow = min(q0 + wave * 32 + l31, S - 1);
      const bf16_t* qp = Qb + (int64_t)qrow * ld + 8 * hh;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
      // The loads are waited for HERE (an opaque use), once per item: left to the first use, hipcc keeps the counted vmcnt waits
      // inside the tile loop, where they would also wait for the (uncounted, asm-issued) LDS-DMA of the next tile.
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
    }

    f32x16 o_acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_acc[i][r] = 0.f;
    float m_run = MASKED ? GROUPED_M0 : -INFINITY, l_run = 0.f;     // running max (log2 domain, may lag the true max by <= RESCALE_THR) and row sum
    // grouped: this lane's row's visibility word (the row clamped as the Q load is), and the group the run's tiles are in: tiles
    // below tile index gend_t belong to group gid (scalars; advanced at the head of a tile)
    [[maybe_unused]] uint32_t vis = 0;
    [[maybe_unused]] int gid = 0, gend_t = 0;
    if constexpr (GROUPED) {
      vis = KG.row_vis[b * KG.stride_vis_b + min(q0 + wave * 32 + l31, S - 1)];
      gend_t = (KG.end[0] + BKV - 1) / BKV;
    }
    [[maybe_unused]] uint32_t gbias = 0;      // biased grouped: the bias word of group gid (scalar; read when gid advances)
    if constexpr (GROUPED && BIASED) gbias = bias_word(0);
    // keyed: the class of key 64t + lane of the tile to come (clamped to the table: keys >= S are masked as in every mode; only the low
    // 5 bits of a byte count, whatever the table holds), loaded a tile ahead: behind tile t's DMA barrier, so that the load has the whole
    // tile to land and the next tile's barrier covers its wait
    [[maybe_unused]] const uint8_t* kcls = nullptr;
    [[maybe_unused]] uint32_t cls_next = 0;
    if constexpr (KEYED) {
      vis = KG.row_vis[b * KG.stride_vis_b + min(q0 + wave * 32 + l31, S - 1)];
      kcls = KG.key_class + b * KG.stride_class_b;
      cls_next = kcls[min(tb * BKV + lane, S - 1)] & 31u;
    }

    // ---- softmax pieces (all per lane; the row's other keys live in lane ^ 32)
    // row max of one 32-key half (this lane's 16 keys)
    auto half_max = [&](const f32x16& s) -> float {
      float ma = max3f(s[0], s[1], s[2]), mb = max3f(s[3], s[4], s[5]);
      ma = max3f(ma, s[6], s[7]);
      mb = max3f(mb, s[8], s[9]);
      ma = max3f(ma, s[10], s[11]);
      mb = max3f(mb, s[12], s[13]);
      return fmaxf(max3f(ma, s[14], s[15]), mb);
    };
    // Deferred rescale: O and l are only rescaled when some row's max grew by more than RESCALE_THR (log2 units) over the
    // max it is currently normalised with; otherwise P = exp2(s - m_run) <= 2^THR, harmless in fp32 accumulators and
    // (being a relative format) in the bf16 P operand. Returns the factor O must be multiplied with (1 = nothing to do);
    // m_run and l_run are updated here, O by the caller once every MFMA fed with old-scale numerators has been issued.
    auto decide = [&](float mx, bool& pend) -> float {
      // Both partial maxima of a row (lanes l and l+32) through one v_permlane32_swap: it exchanges the upper half of its first
      // operand with the lower half of its second, so after it each lane holds its own value in one register and its
      // partner's in the other. Inline asm: with the builtin, hipcc (ROCm 7.2) folds max(result[0], result[1]) to result[0]
      // (the swap is emitted, the v_max is not), so each half-wave saw only one of the two maxima — found by the
      // spiked-key test: a row whose largest score sat in lanes 32-63 was never rescaled. s_nop 1 = the two wait states
      // a VALU write needs before v_permlane*_swap reads it.
      unsigned xa = __builtin_bit_cast(unsigned, mx), xb = xa;
      asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(xa), "+v"(xb));
      const float mxr = fmaxf(__builtin_bit_cast(float, xa), __builtin_bit_cast(float, xb)) * scale_log2;
      float alpha = 1.f;
      pend = false;
      if (RT_RARE(__any(mxr - m_run > RESCALE_THR))) {
        asm volatile("" ::: "memory");           // keep this rare block a real branch (not if-converted)
        const float m_new = fmaxf(m_run, mxr);
        alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: exp2(-inf) = 0 on zeroed state
        m_run = m_new;
        l_run *= alpha;
        pend = true;
      }
      return alpha;
    };
    auto rescale_o = [&](float alpha) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[i][r] *= alpha;
    };
    // numerators of 8 keys (one k-step of Oᵀ += Vᵀ·Pᵀ): registers 8·s2 .. 8·s2+7 of a half
    auto numer8 = [&](const f32x16& s, int s2, bf16x8& pf) {
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[8 * s2 + j], scale_log2, -m_run));
        ps += p;
        pf[j] = (__bf16)p;
      }
      l_run += ps;
    };

// n groups of { 1 MFMA, nds LDS reads, nva vector/transcendental ops }
#define RT_WEAVE(n, nds, nva)                                          \
  _Pragma("unroll") for (int w_ = 0; w_ < (n); ++w_) {                 \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 \
    if ((nds) > 0) __builtin_amdgcn_sched_group_barrier(0x100, (nds), 0); \
    if ((nva) > 0) __builtin_amdgcn_sched_group_barrier(0x402, (nva), 0); \
  }

    auto tile = [&](auto slot_c, int t) {
      constexpr int SLOT = decltype(slot_c)::value;
      constexpr int SB = SLOT * 2 * TILE_B;
      // wave-uniform, almost always false: the tile is the ragged last one of the row (keys >= S are masked) / the tile it
      // stages is (its rows are clamped) / there is no next tile in this run
      const bool ragged = (t + 1) * BKV > S;
      auto kread = [&](int h, int ks) -> bf16x8 {
        return *(const __attribute__((address_space(3))) bf16x8*)(kp[ks] + SB + h * 8192); };
      auto vread = [&](int h, int s2, int dt) -> bf16x8 {
        const s16x4 lo = tr_read(vp[0][dt] + SB + h * 8192 + s2 * 4096);
        const s16x4 hi = tr_read(vp[1][dt] + SB + h * 8192 + s2 * 4096);
        return __builtin_shufflevector(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
      };
      auto mask_half = [&](f32x16& s, int h) {   // key of s{h}[r]: 64t + 32h + (r&3) + 8(r>>2) + 4hh
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t * BKV + 32 * h + (r & 3) + 8 * (r >> 2) + 4 * hh >= S) s[r] = -INFINITY;
      };
      // grouped: lanes whose row does not see this tile's group drop all its scores (wave-uniform branch, as for the ragged tile)
      [[maybe_unused]] bool hidden = false;
      if constexpr (GROUPED) {
        while (t >= gend_t && gid + 1 < KG.n) {
          ++gid;
          gend_t = (KG.end[gid] + BKV - 1) / BKV;
          if constexpr (BIASED) gbias = bias_word(gid);
        }
        hidden = ((vis >> gid) & 1u) == 0;
      }
      auto hide_half = [&](f32x16& s) {
        if (hidden) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = -INFINITY;
        }
      };
      [[maybe_unused]] bool any_hidden = GROUPED && __any(hidden);
      // keyed: vlo / vhi = this row's visibility of keys 0..31 / 32..63 of the tile, shifted so that bit 8(r>>2) + (r&3) is score r's
      [[maybe_unused]] uint32_t vlo = 0, vhi = 0;
      [[maybe_unused]] bool mixed = false;
      [[maybe_unused]] uint32_t cls = 0;
      [[maybe_unused]] uint32_t tbias = 0;       // biased: the tile's bias word (wave-uniform)
      if constexpr (GROUPED && BIASED) tbias = gbias;
      rt_dma_barrier();                          // tile t landed (every wave's vmcnt(0), then the barrier); the other slot is free
      if constexpr (KEYED) {
        cls = cls_next;
        cls_next = kcls[min((t + 1) * BKV + lane, S - 1)] & 31u;
        // every lane's class is below 32 and equals the class it supplies: each turn clears at least the supplying lane, 32 turns at most
        uint64_t rem = __ballot(true);           // the active lanes: the walk ends when each has met its class
        int nclass = 0;
        do {
          const uint32_t c = __builtin_amdgcn_readlane(cls, __builtin_ctzll(rem));
          const uint64_t m = __ballot(cls == c);
          rem &= ~m;
          if ((vis >> c) & 1u) {
            vlo |= (uint32_t)m;
            vhi |= (uint32_t)(m >> 32);
          }
          if constexpr (BIASED) {
            if (RT_RARE((nz >> c) & 1u)) tbias = __builtin_bit_cast(uint32_t, bias_at(c));      // the tile's, when this is its only class
          }
          ++nclass;
        } while (rem);
        mixed = nclass > 1;
        if constexpr (SELF) {
          // the wave's rows q0 + 32·wave .. +31 are keys dq .. dq + 31 of the one tile with dq = 0 or 32 (wave-uniform): there a row sees
          // its own key whatever its word says, and a row that hides the rest of a one-class tile needs the bit test per score
          const int dq = q0 + wave * 32 - t * BKV;
          if (dq == 0 || dq == 32) {
            const int self = min(q0 + wave * 32 + l31, S - 1) - t * BKV;     // clamped as the word load is: a row >= S takes row S-1's key
            if ((unsigned)self < 32u) vlo |= 1u << self;
            else if ((unsigned)self < 64u) vhi |= 1u << (self - 32);
            mixed = true;
          }
        }
        hidden = (vlo & vhi) != 0xffffffffu;     // some key of the tile is hidden from this row
        any_hidden = __any(hidden);
        vlo >>= 4 * hh;
        vhi >>= 4 * hh;
        if constexpr (BIASED) { if (RT_RARE(mixed && tbias)) tbias = MIXED_BIAS; }
      }
      // biased: every score gets the bias of its key's class, before the half's maximum is taken. One class: the scalar. Several (rare,
      // out of line): lane l loads the class and the bias of key 64t + l (clamped as the class load is: a key >= S is -inf already);
      // score r of half h is key 32h + (r&3) + 8(r>>2) + 4hh of the tile (mask_half's map) and takes the bias that the lane of that index holds.
      [[maybe_unused]] auto add_bias = [&](f32x16& s, int h) {
        if (RT_RARE(KEYED && tbias == MIXED_BIAS)) {
          asm volatile("" ::: "memory");           // keep this rare block a real branch
          float kbias = 0.f;
          if constexpr (KEYED && BIASED)
            kbias = KG.key_bias[b * KG.stride_bias_b + (kcls[min(t * BKV + lane, S - 1)] & 31u)] * (1.4426950408889634f / scale_log2);
#pragma unroll
          for (int r = 0; r < 16; ++r) {           // two scalar reads per score register (lanes 0-31 / 32-63 hold different keys), no vector temporaries
            const int k0 = 32 * h + (r & 3) + 8 * (r >> 2);
            const int b0 = __builtin_amdgcn_readlane(__builtin_bit_cast(int, kbias), k0), b1 = __builtin_amdgcn_readlane(__builtin_bit_cast(int, kbias), k0 + 4);
            s[r] += __builtin_bit_cast(float, hh ? b1 : b0);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] += __builtin_bit_cast(float, tbias);
        }
      };
      auto hide_keys = [&](f32x16& s, uint32_t vm) {   // keyed: one class -> the grouped code's whole-tile hide; several -> a bit per score
        if (RT_RARE(mixed)) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (!(vm & (1u << (8 * (r >> 2) + (r & 3))))) s[r] = -INFINITY;
        } else {
          hide_half(s);
        }
      };
      f32x16 s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
      bf16x8 kA[8], kB[8], vA[4], vB[4];         // operand fragments, read one step ahead of the MFMAs that use them
      bf16x8 p00, p01, p10, p11;                 // numerators [half][k-step]
      bool pend;
      // ---- 1: Sᵀ(h0) = K[0:32]·Qᵀ (8 MFMAs) beside the LDS-DMA issue of tile t+1 (one 1-KiB piece behind each MFMA: the asm
      //         statements are placed by hand, sched_group_barrier cannot see inside them) and the first reads of h1
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) kA[ks] = kread(0, ks);
      const bool next_ragged = (t + 2) * BKV > S;
      if (RT_RARE(t + 1 < te && next_ragged)) stage(SLOT ^ 1, t + 1, true);       // clamped rows: all eight pieces at once, out of line
      const bool weave = t + 1 < te && !next_ragged;
      {
        const uint32_t nb = lds0 + (SLOT ^ 1) * 2 * TILE_B, so = (uint32_t)((t + 1) * tile_stride_b);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kA[ks], qf[ks], s0, 0, 0, 0);
          if (RT_USUAL(weave)) rt_dma16_asm((ks & 1) ? rsrcV : rsrcK, nb + ((ks & 1) ? TILE_B : 0) + (wave * 4 + (ks >> 1)) * 1024, soff[ks >> 1], so);
          if (ks >= 4 && ks < 7) kB[ks - 4] = kread(1, ks - 4);
          RT_SB();
        }
      }
      // ---- 2: first 3 MFMAs of Sᵀ(h1) cover the retirement of Sᵀ(h0); row max of h0, decision (no numerators pending)
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kB[ks], qf[ks], s1, 0, 0, 0);
#pragma unroll
      for (int ks = 3; ks < 8; ++ks) kB[ks] = kread(1, ks);
      if (RT_RARE(ragged)) mask_half(s0, 0);
      if constexpr (GROUPED) { if (any_hidden) hide_half(s0); }
      if constexpr (KEYED) { if (any_hidden) hide_keys(s0, vlo); }
      if constexpr (BIASED) { if (tbias) add_bias(s0, 0); }
      float mx0 = half_max(s0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      RT_SB();
      {
        const float alpha = decide(mx0, pend);
        if (RT_RARE(pend)) rescale_o(alpha);
      }
      RT_SB();
      // ---- 3: rest of Sᵀ(h1) ∥ numerators of h0, k-step 0; Vᵀ fragments of (h0, k-step 0) come in
#pragma unroll
      for (int ks = 3; ks < 8; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kB[ks], qf[ks], s1, 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vA[dt] = vread(0, 0, dt);
      numer8(s0, 0, p00);
      RT_WEAVE(5, 2, 6)
      RT_PIN(p00); RT_PIN(l_run);
      RT_SB();
      // ---- 4: Oᵀ += Vᵀ(h0, k-step 0)·p00 ∥ numerators of h0 k-step 1, row max of h1
      // element j of lane-half hh of k-step (h, s2) is key 32h + 16s2 + 8(j>>2) + 4hh + (j&3)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vA[dt], p00, o_acc[dt], 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vB[dt] = vread(0, 1, dt);
      numer8(s0, 1, p01);
      if (RT_RARE(ragged)) mask_half(s1, 1);
      if constexpr (GROUPED) { if (any_hidden) hide_half(s1); }
      if constexpr (KEYED) { if (any_hidden) hide_keys(s1, vhi); }
      if constexpr (BIASED) { if (tbias) add_bias(s1, 1); }
      float mx1 = half_max(s1);
      RT_WEAVE(4, 2, 9)
      RT_PIN(p01); RT_PIN(l_run); RT_PIN(mx1);
      RT_SB();
      const float alpha1 = decide(mx1, pend);    // p01 (old scale) is still to be multiplied into O: O is rescaled after step 5
      RT_SB();
      // ---- 5: Oᵀ += Vᵀ(h0, k-step 1)·p01 ∥ numerators of h1 k-step 0 (against the new max)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vB[dt], p01, o_acc[dt], 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vA[dt] = vread(1, 0, dt);
      numer8(s1, 0, p10);
      RT_WEAVE(4, 2, 7)
      RT_PIN(p10); RT_PIN(l_run);
      RT_SB();
      if (RT_RARE(pend)) rescale_o(alpha1);
      RT_SB();
      // ---- 6: Oᵀ += Vᵀ(h1, k-step 0)·p10 ∥ numerators of h1 k-step 1
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vA[dt], p10, o_acc[dt], 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vB[dt] = vread(1, 1, dt);
      numer8(s1, 1, p11);
      RT_WEAVE(4, 2, 7)
      RT_PIN(p11); RT_PIN(l_run);
      RT_SB();
      // ---- 7: Oᵀ += Vᵀ(h1, k-step 1)·p11
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vB[dt], p11, o_acc[dt], 0, 0, 0);
    };

    // LDS slot = parity of (t - tb)
    int t = tb;
    for (; t + 1 < te; t += 2) {
      tile(S0{}, t);
      tile(S1{}, t + 1);
    }
    if (t < te) tile(S0{}, t);

    const int qrow = q0 + wave * 32 + l31;
    const bool whole = (tb == 0 && te == ntiles);
    if (!whole) {
      // ---- partial: write (Oᵀ, m, l) of this run through to memory, take a ticket, last ticket combines the item
      const int ritem = item - (cut.start + cut.nfull);            // index among the split items of this group
      char* rec = records + split_rec_index(G, b, xcd, jpart, seg) * (int64_t)REC_B + wave * REC_WAVE_B;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(rec, 0, REC_WAVE_B, 0x00020000);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 vv = {o_acc[i][4 * g + 0], o_acc[i][4 * g + 1], o_acc[i][4 * g + 2], o_acc[i][4 * g + 3]};
          const u32x4 w = __builtin_bit_cast(u32x4, vv);
          __builtin_amdgcn_raw_buffer_store_b128(w, rs, (i * 4 + g) * 1024 + lane * 16, 0, 16 /* sc1: write-through */);
        }
      {
        const float2 mlf = {m_run, l_run};
        const u32x2 ml = __builtin_bit_cast(u32x2, mlf);
        __builtin_amdgcn_raw_buffer_store_b64(ml, rs, 16384 + lane * 8, 0, 16);
      }
      int* cnt = counters + (int64_t)b * G.NI + item;
      const SplitParts parts = split_parts(G, cut, ritem);
      const bool last = split_ticket(cnt, parts.nparts, reinterpret_cast<volatile int*>(smem), tid);
      if (last) {
        auto rec_of = [&](int j) -> const char* {
          return records + split_rec_index(G, b, xcd, j, split_seg_of(G, parts, j)) * (int64_t)REC_B + wave * REC_WAVE_B;
        };
        // pass 1: common max; pass 2: weighted sum in run order
        float M = -INFINITY;   // grouped: every record's m is finite (a run that saw nothing: GROUPED_M0, l = 0, O = 0 — weight 0 or, if no run saw anything, 1)
        for (int j = parts.j_first; j <= parts.j_last; ++j) {
          const char* rj = rec_of(__builtin_amdgcn_readfirstlane(j));
          M = fmaxf(M, *reinterpret_cast<const float*>(rj + 16384 + lane * 8));
        }
        float L = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o_acc[i][r] = 0.f;
        for (int j = parts.j_first; j <= parts.j_last; ++j) {
          const char* rj = rec_of(__builtin_amdgcn_readfirstlane(j));
          const float2 ml = *reinterpret_cast<const float2*>(rj + 16384 + lane * 8);
          const float wgt = __builtin_amdgcn_exp2f(ml.x - M);
          L = __builtin_fmaf(ml.y, wgt, L);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(rj + (i * 4 + g) * 1024 + lane * 16);
#pragma unroll
              for (int e = 0; e < 4; ++e) o_acc[i][4 * g + e] = __builtin_fmaf(v[e], wgt, o_acc[i][4 * g + e]);
            }
        }
        l_run = L;
      }
      if (!last) continue;
    }

    // ---- epilogue: O[q][d] = Oᵀ / l ; lane holds q = l31, d = 32dt + (r&3) + 8(r>>2) + 4hh
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = (MASKED && !(l_tot > 0.f)) ? 0.f : 1.0f / l_tot;   // grouped: a row that sees no key gets zeros
    const bool wide = (ldo % 8 == 0) && (stride_ob % 8 == 0) && ((reinterpret_cast<uintptr_t>(O) & 15) == 0);
    if (wide) {
      rt_store_o_rows(O + b * stride_ob + (int64_t)min(qrow, S - 1) * ldo + head * DH, qrow < S, hh, o_acc, inv);
    } else if (qrow < S) {
      bf16_t* op = O + b * stride_ob + (int64_t)qrow * ldo + head * DH + 4 * hh;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          u32x2 w;
          w[0] = pack_bf16x2(o_acc[dt][4 * g + 0] * inv, o_acc[dt][4 * g + 1] * inv);
          w[1] = pack_bf16x2(o_acc[dt][4 * g + 2] * inv, o_acc[dt][4 * g + 3] * inv);
          *reinterpret_cast<u32x2*>(op + dt * 32 + 8 * g) = w;
        }
    }
  }
}

int g_slots_per_xcd = 0;   // 2 workgroups per CU, CUs / 8 per XCD group (queried once)

int slots_per_xcd() {
  if (g_slots_per_xcd == 0) {
    const char* e = getenv("RT_ATTN_SLOTS_PER_XCD");   // A/B and tests only
    g_slots_per_xcd = e ? atoi(e) : (split_cu_count() / 8) * 2;
    if (g_slots_per_xcd < 1) g_slots_per_xcd = 1;
  }
  return g_slots_per_xcd;
}

SplitGeom make_geom(int S, int H, bool want_split) { return split_geom(S, H, BQ, BKV, slots_per_xcd(), want_split); }

}  // namespace

// Workspace of the key-split tail for (B, S, H) on the current device: item counters (zero before first use; the kernel
// leaves them zero) followed by the partial records. 0 when no item of this shape would be split. The larger of the two
// kernels' needs: either may serve the call.
extern "C" int64_t rt_attention_ws_bytes(int32_t B, int32_t S, int32_t H) {
  if (B < 1 || S < 1 || H < 1) return 0;
  static const bool off = getenv("RT_ATTN_SPLIT") && getenv("RT_ATTN_SPLIT")[0] == '0';
  if (off) return 0;
  const int64_t need3 = rt_attention_v3_ws_bytes(B, S, H);
  const int64_t need = split_ws_bytes(B, make_geom(S, H, true), REC_B);
  return need > need3 ? need : need3;
}

// csrc/attention_v3.hip: the one-wave-per-SIMD kernel (64 query rows per wave); takes the launch when S % 256 == 0
extern "C" int rt_attention_variant(int32_t mode) { return rt_attention_v3_mode(mode); }

extern "C" int rt_attention_fwd_rows(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo,
                                     int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, int32_t row_lo, int32_t row_hi, void* ws,
                                     int64_t ws_bytes, void* stream);
extern "C" int rt_attention_fwd(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b,
                                int64_t ldo, int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale,
                                void* ws, int64_t ws_bytes, void* stream) {
  return rt_attention_fwd_rows(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream);
}

namespace {

int check_common(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob, int32_t B,
                 int32_t S, int32_t H, int32_t row_lo, int32_t row_hi) {
  if (!q || !k || !v || !o || B < 1 || S < 1 || H < 1 || row_lo < 0 || row_hi > S || row_lo >= row_hi) return RT_E_BADARG;
  if (!RT_ALIGNED(q, 16) || !RT_ALIGNED(k, 16) || !RT_ALIGNED(v, 16) || !RT_ALIGNED(o, 8) || ld % 8 || stride_b % 8 ||
      ldo % 4 || stride_ob % 4)
    return RT_E_ALIGN;
  if (ld < (int64_t)H * DH || ldo < (int64_t)H * DH) return RT_E_SHAPE;
  if ((int64_t)(S + BKV) * ld * 2 >= (int64_t)1 << 31) return RT_E_SHAPE;      // per-tile byte offsets are 32-bit
  if (!split_fits_32bit(make_geom(S, H, true))) return RT_E_SHAPE;
  return RT_OK;
}

// The launch of attention_fwd_kernel<MODE>: one grid, key split and workspace for every instantiation.
template <int MODE, class KG>
int launch(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob, int32_t B,
           int32_t S, int32_t H, float scale, int32_t row_lo, int32_t row_hi, void* ws, int64_t ws_bytes, void* stream, const KG& kg) {
  const int64_t need = rt_attention_ws_bytes(B, S, H);
  const bool split = ws != nullptr && need > 0;
  if (split && (ws_bytes < need || !RT_ALIGNED(ws, 256))) return RT_E_BADARG;
  const SplitGeom G = make_geom(S, H, split);
  int wmax = 0;
  for (int x = 0; x < 8; ++x) wmax = group_slots(G, x) > wmax ? group_slots(G, x) : wmax;
  const dim3 grid(8 * wmax, B);
  hipLaunchKernelGGL(attention_fwd_kernel<MODE>, grid, dim3(ATT_THREADS), 0, (hipStream_t)stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ld, stride_b, ldo, stride_ob,
                     scale * 1.4426950408889634f, G, row_lo, row_hi, split ? (int*)ws : nullptr,
                     split ? (char*)ws + split_cnt_bytes(B, S, H) : nullptr, kg);
  return rt_hip_status();
}

// The checks of rt_attention_fwd_grouped's own arguments, and its record by value.
int make_key_groups(KeyGroups& kg, int32_t S, float scale, const int32_t* group_end, int32_t n_groups, const uint32_t* row_vis,
                    int64_t stride_vis_b) {
  if (!(scale > 0.f) || !group_end || !row_vis || n_groups < 1 || n_groups > MAX_GROUPS || stride_vis_b < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(row_vis, 4)) return RT_E_ALIGN;
  int32_t prev = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int32_t e = group_end[g];
    if (e <= prev || e > S || (g + 1 < n_groups && e % BKV) || (g + 1 == n_groups && e != S)) return RT_E_BADARG;
    kg.end[g] = prev = e;
  }
  for (int g = n_groups; g < MAX_GROUPS; ++g) kg.end[g] = S;
  kg.n = n_groups;
  kg.row_vis = row_vis;
  kg.stride_vis_b = stride_vis_b;
  return RT_OK;
}

int check_key_bias(const float* key_bias, int64_t stride_bias_b) {
  if (!key_bias || stride_bias_b < 0) return RT_E_BADARG;
  return RT_ALIGNED(key_bias, 4) ? RT_OK : RT_E_ALIGN;
}

}  // namespace

// The full launch, cut exactly as rt_attention_fwd cuts it (same kernel, grid, key split and workspace), in which only the items that
// hold a query row of [row_lo, row_hi) do any work: those rows get the bits rt_attention_fwd gives them, at the cost of their items.
extern "C" int rt_attention_fwd_rows(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b,
                                     int64_t ldo, int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale,
                                     int32_t row_lo, int32_t row_hi, void* ws, int64_t ws_bytes, void* stream) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, row_lo, row_hi)) return st;
  {
    int taken = 0;
    const int st = rt_attention_v3_try(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, row_lo, row_hi, ws, ws_bytes, stream, &taken);
    if (taken || st != RT_OK) return st;
  }
  return launch<DENSE_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, row_lo, row_hi, ws, ws_bytes, stream, NoGroups{});
}

// Region-masked joint attention: always attention_fwd_kernel<true> — the grid, XCD placement, key split and workspace of the dense
// launch of (B, S, H); never attention_v3, whatever rt_attention_variant says. No tile is skipped: a hidden tile costs what a visible one does.
extern "C" int rt_attention_fwd_grouped(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b,
                                        int64_t ldo, int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale,
                                        const int32_t* group_end, int32_t n_groups, const uint32_t* row_vis, int64_t stride_vis_b,
                                        void* ws, int64_t ws_bytes, void* stream) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, 0, S)) return st;
  KeyGroups kg = {};
  if (const int st = make_key_groups(kg, S, scale, group_end, n_groups, row_vis, stride_vis_b)) return st;
  return launch<GROUPED_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream, kg);
}

// rt_attention_fwd_grouped with a bias per key group: the same checks, grid, key split and workspace, the biased instantiation.
extern "C" int rt_attention_fwd_grouped_biased(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b,
                                               int64_t ldo, int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale,
                                               const int32_t* group_end, int32_t n_groups, const uint32_t* row_vis, int64_t stride_vis_b,
                                               void* ws, int64_t ws_bytes, void* stream, const float* key_bias, int64_t stride_bias_b) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, 0, S)) return st;
  KeyGroupsBiased kg = {};
  if (const int st = make_key_groups(kg, S, scale, group_end, n_groups, row_vis, stride_vis_b)) return st;
  if (const int st = check_key_bias(key_bias, stride_bias_b)) return st;
  kg.key_bias = key_bias;
  kg.stride_bias_b = stride_bias_b;
  return launch<GROUPED_BIASED_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream, kg);
}

// Joint attention with a class id per key (region isolation of per-line prompts): the grouped launch with visibility decided per key
// instead of per 64-key tile. Same kernel source, grid, XCD placement, key split and workspace; never attention_v3.
extern "C" int rt_attention_fwd_keyed(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo,
                                      int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, const uint32_t* row_vis,
                                      int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b, void* ws, int64_t ws_bytes,
                                      void* stream) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, 0, S)) return st;
  if (!(scale > 0.f) || !row_vis || !key_class || stride_vis_b < 0 || stride_class_b < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(row_vis, 4)) return RT_E_ALIGN;
  const KeyClasses kc = {row_vis, stride_vis_b, key_class, stride_class_b};
  return launch<KEYED_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream, kc);
}

// rt_attention_fwd_keyed with the self rule (perturbed-attention guidance): row i also sees key i. The same checks, grid, key split
// and workspace, the self instantiation.
extern "C" int rt_attention_fwd_keyed_self(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo,
                                           int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, const uint32_t* row_vis,
                                           int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b, void* ws,
                                           int64_t ws_bytes, void* stream) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, 0, S)) return st;
  if (!(scale > 0.f) || !row_vis || !key_class || stride_vis_b < 0 || stride_class_b < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(row_vis, 4)) return RT_E_ALIGN;
  const KeyClasses kc = {row_vis, stride_vis_b, key_class, stride_class_b};
  return launch<KEYED_SELF_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream, kc);
}

// rt_attention_fwd_keyed with a bias per key class: the same checks, grid, key split and workspace, the biased instantiation.
extern "C" int rt_attention_fwd_keyed_biased(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo,
                                             int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, const uint32_t* row_vis,
                                             int64_t stride_vis_b, const uint8_t* key_class, int64_t stride_class_b, void* ws,
                                             int64_t ws_bytes, void* stream, const float* key_bias, int64_t stride_bias_b) {
  if (const int st = check_common(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, 0, S)) return st;
  if (!(scale > 0.f) || !row_vis || !key_class || stride_vis_b < 0 || stride_class_b < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(row_vis, 4)) return RT_E_ALIGN;
  if (const int st = check_key_bias(key_bias, stride_bias_b)) return st;
  KeyClassesBiased kc = {};
  kc.row_vis = row_vis, kc.stride_vis_b = stride_vis_b, kc.key_class = key_class, kc.stride_class_b = stride_class_b;
  kc.key_bias = key_bias, kc.stride_bias_b = stride_bias_b;
  return launch<KEYED_BIASED_MODE>(q, k, v, o, ld, stride_b, ldo, stride_ob, B, S, H, scale, 0, S, ws, ws_bytes, stream, kc);
}
