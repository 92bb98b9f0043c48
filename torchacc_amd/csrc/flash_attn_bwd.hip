// Flash-attention v2 BACKWARD for gfx950 (CDNA4 MFMA).
//
// Three kernels (recompute variant — deterministic, no atomics):
//   1. fa_bwd_preprocess: delta[b,h,sq] = rowsum(dO * O), 16-byte loads.
//   2. fa_bwd_dkv: grid over 128-key tiles (4-wave WG, wave = 32 keys);
//      K fragments live in registers, V in LDS; per 32-row Q tile (Q, dO,
//      lse, delta staged in LDS) it recomputes P from (S, stored lse),
//      computes dP, dS, and accumulates dV += P^T dO and dK += dS^T Q, using
//      the cvt_pk + permlane32_swap fragment redistribution (T12) to turn
//      the QK^T accumulator layout into mfma A-operands.
//   3. fa_bwd_dq: forward structure (8-wave WG, wave = 32 q rows); K and V
//      staged in LDS per 128-key tile; dQ += dS K accumulated in registers.
//
// LDS images. Every tile (Q, dO, V in dkv; K, V in dq) is stored ONCE, in
// the dual-use image of attn_common.h (attn_dual_off): 8-row x 32-column
// subtiles of 512 B with the 16-byte chunks of a row XORed by (row>>2)&3.
// The same copy serves the row reads (ds_read_b128, A operand of S and dP)
// and the transposed reads (ds_read_b64_tr_b16, B operand of dK, dV and dQ),
// both conflict-free; register-staged writes (V in dkv, K/V in dq) go in
// attn_dual_stage_coord order, also conflict-free. There is no transposed K
// copy.
//
// Buffer rotation. Both kernels keep TWO staging buffers and one barrier per
// tile. Iteration i computes from buffer i&1 and fills buffer (i+1)&1 with
// tile i+1:
//   dkv: direct-to-LDS loads (global_load_lds, 16 bytes for Q and dO, 4 bytes
//        for lse and delta) issued at the top of the iteration and waited
//        for (vmcnt(0)) just before the closing barrier, so they are in
//        flight over the whole compute phase and hold no registers (the
//        kernel sits at the 256-VGPR budget of two workgroups per CU; a tile
//        held in registers spills). The LDS destination of such a load is
//        wave base + lane*16, so the image is kept and the swizzle is put on
//        the per-lane source address (attn_dual_slot_coord). Rows beyond sq
//        read the clamped row sq-1 and are masked like any row beyond
//        qlimit. The compute phase consumes no ordinary global load, which
//        would make the compiler drain vmcnt early. The sweep over (head, q
//        tile) is flattened so the prefetch runs across heads.
//   dq:  per 64-key half: global loads issued before the half's MFMAs, LDS
//        write after them (16 VGPRs in flight).
// The barrier that ends iteration i does both jobs: it publishes buffer
// (i+1)&1 for iteration i+1, and it retires every wave's reads of buffer i&1
// before iteration i+1 overwrites it. The fills of iteration i need no
// barrier of their own: buffer (i+1)&1 was last read in iteration i-1, whose
// closing barrier every wave has passed. The prologue barrier publishes
// buffer 0 (and the V image in dkv).
//
// Transposed reads. In both kernels the ds_read_b64_tr_b16 of the next step
// (dkv: one (tp, a) step = 4 reads, 2 MFMAs) or of the next row of steps (dq:
// NA steps of 2 reads, 1 MFMA each) are issued before the current step's
// MFMAs; each step waits with a counted lgkmcnt for its own reads only.
//
// Two softmax bodies in dkv. Between the S/dP MFMAs and the dV/dK steps a
// wave picks, per tile and wave-uniformly, how P and dS are computed: the
// INTERIOR body when all 32 rows and 32 keys are inside the limits, the block
// lies wholly on the visible side of the causal diagonal and all 32 staged
// lse are finite (one class compare + ballot); the general body, with the
// per-element `valid` mask, otherwise. Both evaluate the same expressions,
// so the choice changes no bit. The instruction order of a tile is
// unchanged: 16 MFMAs (S, dP interleaved over t), the softmax block, 16
// MFMAs (dV, dK). Window and lens instantiations, and fa_bwd_dq, have the
// general body only (the second body costs them registers: see
// profiles/r06_attn_bwd_valu.md).
//
// P is normalized against the stored global lse and delta comes from the
// global (out, dout), so the same kernels serve per-block ring-attention
// backward unchanged.
//
// Fragment-layout cheat sheet (v_mfma_f32_32x32x16_bf16):
//   A[row][k] : lane l holds row = l&31,  k = (l>>5)*8 + j   (j = 0..7)
//   B[k][col] : lane l holds col = l&31,  k = (l>>5)*8 + j
//   D[row][col]: lane l holds col = l&31, row = CROW(r, l>>5), r = 0..15
// t12_pack_frag converts a D-layout f32 pair-block into the bf16 fragment
// whose ROW axis is D's col axis and whose k axis is D's row axis — i.e. it
// transposes the accumulator into an A/B operand.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "attn_common.h"

// s_waitcnt immediate for vmcnt(0) alone (gfx9 encoding: expcnt and lgkmcnt
// fields at their maxima). Issued as the builtin so that the compiler's own
// wait bookkeeping sees it.
#define VMCNT0 0x0F70

// ---------------------------------------------------------------------------
// 1. preprocess: delta = rowsum(dO * O)   [b,h,sq] fp32
// ---------------------------------------------------------------------------
// One 16-byte chunk of dO and of O per lane: D/8 lanes share a row and a
// wave takes 64/(D/8) rows. Lane m of a row holds the pair products
// p[4m..4m+3] (pair k = elements 2k, 2k+1); the shuffles below add them in
// the order of a 64-lane xor butterfly over k (offsets 32..1, absent pairs
// being exact zeros), so delta keeps the rounding of a pair-per-lane sum.
template <bool FP16, int D>
__global__ void fa_bwd_preprocess_kernel(const short* __restrict__ dO,
                                         const short* __restrict__ O,
                                         float* __restrict__ delta, int b,
                                         int sq, int hq) {
  constexpr int LPR = D / 8;          // lanes per row
  constexpr int RPW = WAVE / LPR;     // rows per wave
  const int lane = threadIdx.x % WAVE;
  const int m = lane % LPR;
  const long row = ((long)blockIdx.x * (blockDim.x / WAVE) +
                    (threadIdx.x / WAVE)) * RPW + lane / LPR;
  const long rows = (long)b * sq * hq;
  s16x8 d8 = {0, 0, 0, 0, 0, 0, 0, 0};
  s16x8 o8 = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < rows) {
    d8 = *reinterpret_cast<const s16x8*>(dO + row * D + m * 8);
    o8 = *reinterpret_cast<const s16x8*>(O + row * D + m * 8);
  }
  float p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    p[i] = AttnElem<FP16>::to_f32(d8[2 * i]) *
               AttnElem<FP16>::to_f32(o8[2 * i]) +
           AttnElem<FP16>::to_f32(d8[2 * i + 1]) *
               AttnElem<FP16>::to_f32(o8[2 * i + 1]);
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] += __shfl_xor(p[i], off, 64);
  }
  const float acc = (p[0] + p[2]) + (p[1] + p[3]);
  if (m == 0 && row < rows) {
    const int h = row % hq;
    const long bs = row / hq;
    const long bb = bs / sq, s = bs % sq;
    delta[(bb * hq + h) * sq + s] = acc;
  }
}

// ---------------------------------------------------------------------------
// 2. dK/dV kernel
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL, bool HAS_WINDOW, bool HAS_LENS, bool FP16>
__global__ __launch_bounds__(256, 2)
void fa_bwd_dkv_kernel(const short* __restrict__ dOut,
                       const short* __restrict__ Q,
                       const short* __restrict__ K,
                       const short* __restrict__ V,
                       const float* __restrict__ LSE,
                       const float* __restrict__ DELTA,
                       short* __restrict__ dK, short* __restrict__ dV,
                       int b_, int sq, int sk, int hq, int hk, float scale,
                       int wl, int wr, const int* __restrict__ q_lens,
                       const int* __restrict__ k_lens) {
  constexpr int NT = D / 16;
  constexpr int NA = D / 32;
  constexpr int QT = 32;            // q rows per staged tile
  constexpr int KVWG = 128;         // keys per workgroup (4 waves x 32)
  constexpr int TILE_B = QT * D * 2;        // bytes of one Q (or dO) image
  constexpr int BUF_B = 2 * TILE_B;         // one buffer = Q image + dO image
  constexpr int CPT = QT * D / 8 / 256;     // 16-byte chunks per thread

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [2 buffers][Q image, dO image], dual-use image (attn_common.h)
  char* qd_lds = smem;
  short* v_lds = reinterpret_cast<short*>(smem + 2 * BUF_B);  // [KVWG][D], same image
  float* st_lds = reinterpret_cast<float*>(v_lds + KVWG * D);
  // st_lds: [2 buffers][lse[QT], delta[QT]]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;          // 0..3
  const int col = lane & 31;
  const int hi = lane >> 5;

  const int kh = blockIdx.y % hk;
  const int b = blockIdx.y / hk;
  const int gqa = hq / hk;
  // tile<->XCD decorrelation (see fa_fwd_kernel)
  const int kv0wg = (int)((blockIdx.x + blockIdx.y) % gridDim.x) * KVWG;
  const int key_b = kv0wg + wid * 32;          // wave's key block base
  const int mykey = key_b + col;               // lane's key (K frag row)
  const int shift = sk - sq;

  int klimit = sk;
  int qlimit = sq;
  if (HAS_LENS) {
    if (k_lens != nullptr) klimit = min(klimit, k_lens[b]);
    if (q_lens != nullptr) qlimit = min(qlimit, q_lens[b]);
  }

  int q_lo = 0;
  if (CAUSAL) q_lo = max(0, kv0wg - shift);
  int q_hi = qlimit;
  if (HAS_WINDOW && wl >= 0)
    q_hi = min(q_hi, kv0wg + KVWG - 1 - shift + wl + 1);
  const int qt0 = q_lo / QT;
  const int qt1 = (max(q_hi, 0) + QT - 1) / QT;
  // the (head, q tile) sweep, heads outer, flattened so the prefetch runs
  // across the head boundary
  const int n_tiles = qt1 > qt0 ? gqa * (qt1 - qt0) : 0;

  // ---- direct-to-LDS staging of one Q/dO/lse/delta tile into buffer `buf`.
  // One wave-instruction writes 1 KiB = 64 consecutive 16-byte slots of an
  // image (wave w, pass i: slots i*256 + w*64 ..), so the image stays the
  // dual-use one and the swizzle goes on the per-lane SOURCE address
  // (attn_dual_slot_coord, the inverse of attn_dual_off): 8 rows x 128
  // contiguous bytes per instruction. Rows at or beyond sq read row sq-1:
  // in bounds, finite, and masked by qrow < qlimit like every other row
  // beyond the limit. lse (lanes 0..31) and delta (lanes 32..63) go the same
  // way, one 4-byte instruction of wave 0, so that no ordinary global load is
  // consumed while a tile is in flight (the compiler would drain vmcnt for
  // it). Nothing is held in registers.
  const int wid_s = __builtin_amdgcn_readfirstlane(wid);
  const int key_s = kv0wg + wid_s * 32;   // key_b, provably wave-uniform
  auto tile_dma = [&](int h, int q0, int buf) {
    char* dst = qd_lds + buf * BUF_B + wid_s * (WAVE * 16);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int row, ch;
      attn_dual_slot_coord<D>(tid + i * 256, row, ch);
      const int qrow = min(q0 + row, sq - 1);
      const long src = ((long)(b * sq + qrow) * hq + h) * D + ch * 8;
      attn_glds16(Q + src, dst + i * (256 * 16));
      attn_glds16(dOut + src, dst + TILE_B + i * (256 * 16));
    }
    if (wid_s == 0) {
      const int qrow = min(q0 + (lane & (QT - 1)), sq - 1);
      const long idx = ((long)b * hq + h) * sq + qrow;
      attn_glds4(lane < QT ? LSE + idx : DELTA + idx,
                 st_lds + buf * 2 * QT);
    }
  };

  // loader position: (head, q tile) of the next tile to fetch
  int ld_gh = 0, ld_qt = qt0;
  if (n_tiles > 0) tile_dma(kh * gqa, qt0 * QT, 0);

  // K fragments in registers; V staged once in LDS for the whole workgroup
  bf16x8 kfrag[NT];
  {
    const bool kv_ok = mykey < sk;
    const long base =
        ((long)b * sk + (kv_ok ? mykey : sk - 1)) * hk * D + (long)kh * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s16x8 kv8 = kv_ok
          ? *reinterpret_cast<const s16x8*>(K + base + t * 16 + hi * 8)
          : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) kfrag[t][j] = kv8[j];
    }
  }
  {
    constexpr int CHUNKS = KVWG * D / 8;
    const long vbase = ((long)b * sk * hk + kh) * D;
    for (int c = tid; c < CHUNKS; c += 256) {
      int row, ch;
      attn_dual_stage_coord<D>(c, row, ch);
      const int key = kv0wg + row;
      s16x8 vv8 = {0, 0, 0, 0, 0, 0, 0, 0};
      if (key < sk)
        vv8 = *reinterpret_cast<const s16x8*>(V + vbase +
                                              (long)key * hk * D + ch * 8);
      *reinterpret_cast<s16x8*>(reinterpret_cast<char*>(v_lds) +
                                attn_dual_off<D>(row, ch)) = vv8;
    }
  }
  // the direct-to-LDS loads of tile 0 are counted on vmcnt
  __builtin_amdgcn_s_waitcnt(VMCNT0);
  __syncthreads();   // V image and buffer 0 visible

  // per-lane constant offsets into a Q image: row reads (A operand, row =
  // col, chunk 2t+hi: even t at row_off, odd t at row_off^32, +512 per two
  // t). The two transposed-read addresses (attn_dual_tr_bases) are
  // loop-carried and hop between the two buffers, one register each: the
  // budget is 256 VGPRs with none spare.
  const unsigned row_off = attn_dual_off<D>(col, hi);
  unsigned tr0, tr1;
  attn_dual_tr_bases<D>(lane, tr0, tr1);
  tr0 += (unsigned)(size_t)qd_lds;
  tr1 += (unsigned)(size_t)qd_lds;
  // this wave's 32 keys of the V image (same row/chunk offsets as Q)
  const char* vwave =
      reinterpret_cast<const char*>(v_lds) + wid * 4 * (16 * D);

  f32x16 dkacc[NA], dvacc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    dkacc[a] = f32x16(0.f);
    dvacc[a] = f32x16(0.f);
  }

  int c_qt = qt0;
  for (int it = 0; it < n_tiles; ++it) {
    const int cur = it & 1;
    const int q0 = c_qt * QT;
    const bool has_next = it + 1 < n_tiles;   // workgroup-uniform
    // ---- issue the next tile's direct-to-LDS loads into the OTHER buffer
    // before computing this one. Every wave left that buffer's reads behind
    // at the barrier that ended the previous iteration, so no barrier is
    // needed here. The loads stay in flight over the whole compute phase
    // (which touches no global memory) and are waited for just before the
    // closing barrier. ------------------------------------------------------
    if (has_next) {
      if (++ld_qt == qt1) { ld_qt = qt0; ++ld_gh; }
      tile_dma(kh * gqa + ld_gh, ld_qt * QT, cur ^ 1);
    }

    const char* qcur = qd_lds + cur * BUF_B;
    const float* lse_lds = st_lds + cur * 2 * QT;
    const float* del_lds = lse_lds + QT;

    // per-wave skip: this wave's keys [key_b, key_b+31] have no valid q
    // in the tile (causal diagonal / window-left bound) — staging and
    // barriers are cooperative, so only the compute is guarded. The branch
    // is wave-uniform: EXEC is all ones at the transposed reads inside.
    bool wave_active = true;
    if (CAUSAL && q0 + QT - 1 < key_b - shift) wave_active = false;
    if (HAS_WINDOW && wl >= 0 && q0 > key_b + 31 - shift + wl)
      wave_active = false;

    if (wave_active) {
      // S = Q K^T and dP = dO V^T, both D[q=CROW][key=col]
      f32x16 s = f32x16(0.f);
      f32x16 dp = f32x16(0.f);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const unsigned byte =
            ((t & 1) ? (row_off ^ 32u) : row_off) + (t >> 1) * 512;
        bf16x8 qf = *reinterpret_cast<const bf16x8*>(qcur + byte);
        bf16x8 df = *reinterpret_cast<const bf16x8*>(qcur + TILE_B + byte);
        bf16x8 vf = *reinterpret_cast<const bf16x8*>(vwave + byte);
        s = AttnElem<FP16>::mfma(qf, kfrag[t], s);
        dp = AttnElem<FP16>::mfma(df, vf, dp);
      }
      // P = exp(S*scale - lse); dS = P*(dP - delta)*scale
      // (s reused as P, dp reused as dS — register budget), in two
      // instantiations. INTERIOR: every (q row, key) pair of the wave's
      // 32 x 32 block is valid, so there is no compare, no select and no
      // `valid` logic; the expressions are those of the general body, which
      // serves the edge tiles.
      auto softmax = [&](auto interior_c) {
      constexpr bool INTERIOR = decltype(interior_c)::value;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = q0 + CROW(r, hi);
        const float lse_q = lse_lds[CROW(r, hi)];
        const float del_q = del_lds[CROW(r, hi)];
        float p;
        if constexpr (INTERIOR) {
          p = __expf(s[r] * scale - lse_q);
        } else {
          bool valid =
              (qrow < qlimit) && (mykey < klimit) && isfinite(lse_q);
          if (CAUSAL) valid &= (mykey <= qrow + shift);
          if (HAS_WINDOW && wl >= 0) valid &= (mykey >= qrow + shift - wl);
          if (HAS_WINDOW && wr >= 0 && !CAUSAL)
            valid &= (mykey <= qrow + shift + wr);
          p = valid ? __expf(s[r] * scale - lse_q) : 0.f;
        }
        float ds = p * (dp[r] - del_q) * scale;
        if constexpr (INTERIOR) {
          // Keep the scalar v_sub/v_mul forms: without the selects between
          // them the SLP vectorizer would pair these into v_pk_*_f32, which
          // run slower beside MFMAs. An opaque value is no vectorizer seed.
          asm("" : "+v"(ds));
        }
        s[r] = p;
        dp[r] = ds;
      }
      };
      // wave-uniform choice of the body: all 32 rows and all 32 keys inside
      // the limits, the whole block on the visible side of the diagonal and
      // of the window, and all 32 staged lse finite (lane l tests row l&31)
      //
      // Only the instantiations without window and without lens carry the
      // second body: with it the D=64 window ones need 170 VGPRs (occupancy
      // 3 -> 2) and the D=128 causal + lens ones spill 8 bytes. The others
      // compile to what they were.
      if constexpr (!HAS_WINDOW && !HAS_LENS) {
        bool interior = (q0 + QT <= qlimit) && (key_s + 32 <= klimit);
        if (CAUSAL) interior = interior && (key_s + 31 <= q0 + shift);
        interior = interior &&
            __builtin_amdgcn_ballot_w64(isfinite(lse_lds[col])) == ~0ull;
        if (interior)
          softmax(std::true_type{});
        else
          softmax(std::false_type{});
      } else {
        softmax(std::false_type{});
      }
      // A-frags over the q k-dim; step tp covers q rows 16tp..16tp+15.
      // B-frags X[q = 16tp + hi*8 + jj][d = a*32 + col] come straight from
      // the dual-use q/do images via ds_read_b64_tr_b16 (probe:
      // csrc/tools/tr16_probe.hip; see attn_common.h). The byte address is
      //   tr0 (jj = 0..3) or tr1 (jj = 4..7)            (per-lane)
      //   + tp*32*D + a*512 (+ TILE_B for dO)           (compile-time)
      // so all 4*NA reads of a tile use two address VGPRs + offset:
      // immediates.
      //
      // The 2*NA steps (tp, a) are software-pipelined: the four reads of
      // step n+1 are issued before the two MFMAs of step n, and step n waits
      // with lgkmcnt(4), i.e. for everything but the four reads just issued
      // (LDS operations return in order; any other LDS or scalar-memory
      // operation in flight only makes the counted wait stricter). The wait
      // statement names the four destinations as in/out operands, so the
      // MFMAs depend on it. Both A fragments are packed first: s and dp are
      // dead from there on, which pays for the second set of destinations.
#define DKV_TR_DECL(n_) attn_u32x2 ql##n_, qh##n_, dl##n_, dh##n_
#define DKV_TR_ISSUE(n_, tp_, a_)                                          \
      asm volatile(                                                        \
          "ds_read_b64_tr_b16 %0, %4 offset:%c6\n\t"                     \
          "ds_read_b64_tr_b16 %1, %5 offset:%c6\n\t"                     \
          "ds_read_b64_tr_b16 %2, %4 offset:%c7\n\t"                     \
          "ds_read_b64_tr_b16 %3, %5 offset:%c7"                          \
          : "=v"(ql##n_), "=v"(qh##n_), "=v"(dl##n_), "=v"(dh##n_)         \
          : "v"(tr0), "v"(tr1),                                            \
            "i"((tp_) * 32 * D + (a_) * 512),                              \
            "i"(TILE_B + (tp_) * 32 * D + (a_) * 512))
#define DKV_TR_MFMA(n_, cnt_, a_, pb_, dsb_)                               \
      {                                                                    \
        asm volatile("s_waitcnt lgkmcnt(" #cnt_ ")"                        \
                     : "+v"(ql##n_), "+v"(qh##n_), "+v"(dl##n_),           \
                       "+v"(dh##n_));                                      \
        attn_u32x4 uq_ = {ql##n_.x, ql##n_.y, qh##n_.x, qh##n_.y};         \
        attn_u32x4 ud_ = {dl##n_.x, dl##n_.y, dh##n_.x, dh##n_.y};         \
        bf16x8 qbf = __builtin_bit_cast(bf16x8, uq_);                      \
        bf16x8 dob = __builtin_bit_cast(bf16x8, ud_);                      \
        dvacc[a_] = AttnElem<FP16>::mfma(pb_, dob, dvacc[a_]);             \
        dkacc[a_] = AttnElem<FP16>::mfma(dsb_, qbf, dkacc[a_]);            \
      }
      {
        DKV_TR_DECL(0); DKV_TR_DECL(1); DKV_TR_DECL(2); DKV_TR_DECL(3);
        DKV_TR_ISSUE(0, 0, 0);
        unsigned pfr0[4], dsfr0[4], pfr1[4], dsfr1[4];
        t12_pack_frag<AttnElem<FP16>>(s, 0, pfr0);
        t12_pack_frag<AttnElem<FP16>>(dp, 0, dsfr0);
        t12_pack_frag<AttnElem<FP16>>(s, 1, pfr1);
        t12_pack_frag<AttnElem<FP16>>(dp, 1, dsfr1);
        const bf16x8 pb0 = *reinterpret_cast<const bf16x8*>(pfr0);
        const bf16x8 dsb0 = *reinterpret_cast<const bf16x8*>(dsfr0);
        const bf16x8 pb1 = *reinterpret_cast<const bf16x8*>(pfr1);
        const bf16x8 dsb1 = *reinterpret_cast<const bf16x8*>(dsfr1);
        if constexpr (NA > 2) {
          DKV_TR_DECL(4); DKV_TR_DECL(5); DKV_TR_DECL(6); DKV_TR_DECL(7);
          DKV_TR_ISSUE(1, 0, 1); DKV_TR_MFMA(0, 4, 0, pb0, dsb0);
          DKV_TR_ISSUE(2, 0, 2); DKV_TR_MFMA(1, 4, 1, pb0, dsb0);
          DKV_TR_ISSUE(3, 0, 3); DKV_TR_MFMA(2, 4, 2, pb0, dsb0);
          DKV_TR_ISSUE(4, 1, 0); DKV_TR_MFMA(3, 4, 3, pb0, dsb0);
          DKV_TR_ISSUE(5, 1, 1); DKV_TR_MFMA(4, 4, 0, pb1, dsb1);
          DKV_TR_ISSUE(6, 1, 2); DKV_TR_MFMA(5, 4, 1, pb1, dsb1);
          DKV_TR_ISSUE(7, 1, 3); DKV_TR_MFMA(6, 4, 2, pb1, dsb1);
          DKV_TR_MFMA(7, 0, 3, pb1, dsb1);
        } else {
          DKV_TR_ISSUE(1, 0, 1); DKV_TR_MFMA(0, 4, 0, pb0, dsb0);
          DKV_TR_ISSUE(2, 1, 0); DKV_TR_MFMA(1, 4, 1, pb0, dsb0);
          DKV_TR_ISSUE(3, 1, 1); DKV_TR_MFMA(2, 4, 0, pb1, dsb1);
          DKV_TR_MFMA(3, 0, 1, pb1, dsb1);
        }
      }
#undef DKV_TR_DECL
#undef DKV_TR_ISSUE
#undef DKV_TR_MFMA
    }  // wave_active

    // one barrier per tile: it publishes buffer cur^1 (whose direct-to-LDS
    // loads every wave has waited for) and retires this iteration's reads of
    // buffer cur before the next iteration's loads overwrite it
    __builtin_amdgcn_s_waitcnt(VMCNT0);
    __syncthreads();
    if (++c_qt == qt1) c_qt = qt0;
    const unsigned hop = cur ? (unsigned)-BUF_B : (unsigned)BUF_B;
    tr0 += hop;
    tr1 += hop;
  }

  // ---- epilogue: D[key = key_b + CROW(r,hi)][d = a*32 + col] ------------
#pragma unroll
  for (int a = 0; a < NA; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = key_b + CROW(r, hi);
      const int d = a * 32 + col;
      if (key < sk) {
        const long base = ((long)b * sk + key) * hk * D + (long)kh * D;
        dK[base + d] = AttnElem<FP16>::from_f32(dkacc[a][r]);
        dV[base + d] = AttnElem<FP16>::from_f32(dvacc[a][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 3. dQ kernel (forward structure)
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL, bool HAS_WINDOW, bool HAS_LENS, bool FP16>
__global__ __launch_bounds__(512, 2)
void fa_bwd_dq_kernel(const short* __restrict__ dOut,
                      const short* __restrict__ Q,
                      const short* __restrict__ K,
                      const short* __restrict__ V,
                      const float* __restrict__ LSE,
                      const float* __restrict__ DELTA,
                      short* __restrict__ dQ, int b_, int sq, int sk, int hq,
                      int hk, float scale, int wl, int wr,
                      const int* __restrict__ q_lens,
                      const int* __restrict__ k_lens) {
  constexpr int NT = D / 16;
  constexpr int NA = D / 32;
  // 128-key staged tiles, two buffers of (K image + V image): one 8-wave WG
  // is resident anyway (VGPR-bound), so 128 KB of LDS at D=128 costs no
  // occupancy. The tile is computed, and the next one prefetched, in two
  // 64-key halves so the in-flight registers stay at 4 x 16 B per thread.
  constexpr int KVB = 128;
  constexpr int TILE_B = KVB * D * 2;       // bytes of one K (or V) image
  constexpr int BUF_B = 2 * TILE_B;
  constexpr int HALF_B = TILE_B / 2;        // 64 rows of a dual-use image
  constexpr int CPT = 64 * D / 8 / 512;     // chunks per thread per half

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [2 buffers][K image, V image], both in the dual-use image

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;
  const int hi = lane >> 5;

  const int h = blockIdx.y % hq;
  const int b = blockIdx.y / hq;
  const int kh = h / (hq / hk);
  // tile<->XCD decorrelation (see fa_fwd_kernel)
  const int q0wg = (int)((blockIdx.x + blockIdx.y) % gridDim.x) * 256;
  const int q0 = q0wg + wid * 32;
  const int qrow = q0 + col;
  const int shift = sk - sq;

  int klimit = sk;
  int qlimit = sq;
  if (HAS_LENS) {
    if (k_lens != nullptr) klimit = min(klimit, k_lens[b]);
    if (q_lens != nullptr) qlimit = min(qlimit, q_lens[b]);
  }

  int kv_hi_key = klimit;
  if (CAUSAL) kv_hi_key = min(kv_hi_key, q0wg + 255 + shift + 1);
  int kv_lo_key = 0;
  if (HAS_WINDOW && wl >= 0) kv_lo_key = max(0, q0wg + shift - wl);
  const int t0 = kv_lo_key / KVB;
  const int t1 = (max(kv_hi_key, 0) + KVB - 1) / KVB;
  const long kbase = ((long)b * sk * hk + kh) * D;

  // ---- staging of one 64-key half of a K/V tile: global-load half (into
  // registers) and LDS-write half ------------------------------------------
  s16x8 pk[CPT], pv[CPT];
  int srow[CPT];
  unsigned soff[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    int ch;
    attn_dual_stage_coord<D>(tid + i * 512, srow[i], ch);
    soff[i] = attn_dual_off<D>(srow[i], ch);
    srow[i] = srow[i] * 16 + ch;   // packed (row, ch)
  }
  auto half_load = [&](int kv0h) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int key = kv0h + (srow[i] >> 4);
      const int d0 = (srow[i] & 15) * 8;
      pk[i] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      pv[i] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (key < sk) {
        const long src = kbase + (long)key * hk * D + d0;
        pk[i] = *reinterpret_cast<const s16x8*>(K + src);
        pv[i] = *reinterpret_cast<const s16x8*>(V + src);
      }
    }
  };
  auto half_store = [&](int buf, int half) {
    char* dst = smem + buf * BUF_B + half * HALF_B;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      *reinterpret_cast<s16x8*>(dst + soff[i]) = pk[i];
      *reinterpret_cast<s16x8*>(dst + TILE_B + soff[i]) = pv[i];
    }
  };

  if (t0 < t1) half_load(t0 * KVB);

  bf16x8 qfrag[NT], dofrag[NT];
  {
    const long qbase = ((long)(b * sq + min(qrow, sq - 1)) * hq + h) * D;
    const bool qvalid = (qrow < sq);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s16x8 v8 = qvalid
          ? *reinterpret_cast<const s16x8*>(Q + qbase + t * 16 + hi * 8)
          : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 d8 = qvalid
          ? *reinterpret_cast<const s16x8*>(dOut + qbase + t * 16 + hi * 8)
          : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        qfrag[t][j] = v8[j];
        dofrag[t][j] = d8[j];
      }
    }
  }
  const bool row_ok = (qrow < qlimit);
  const float lse_q =
      row_ok ? LSE[((long)b * hq + h) * sq + qrow] : INFINITY;
  const float del_q =
      row_ok ? DELTA[((long)b * hq + h) * sq + qrow] : 0.f;

  if (t0 < t1) {
    half_store(0, 0);
    half_load(t0 * KVB + 64);
    half_store(0, 1);
  }
  __syncthreads();   // buffer 0 visible

  f32x16 dqacc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) dqacc[a] = f32x16(0.f);

  // per-lane constant offsets into a K/V image: row reads (A operand, row =
  // kb*32 + col, chunk 2t+hi) and the transposed-read bases of the
  // dQ += dS K B operand K[key = kb*32 + 16tp + 8hi + j][d = 32a + col]
  const unsigned row_off = attn_dual_off<D>(col, hi);
  unsigned tr_b0, tr_b1;
  attn_dual_tr_bases<D>(lane, tr_b0, tr_b1);
  const unsigned lds_base = (unsigned)(size_t)smem;

  for (int tile = t0; tile < t1; ++tile) {
    const int kv0 = tile * KVB;
    const int cur = (tile - t0) & 1;
    const bool has_next = tile + 1 < t1;      // workgroup-uniform

#pragma unroll 1
    for (int half = 0; half < KVB / 64; ++half) {
    const int kv0h = kv0 + half * 64;
    // ---- issue the global loads of the next tile's same half -------------
    if (has_next) half_load(kv0h + KVB);

    const char* kcur = smem + cur * BUF_B + half * HALF_B;
    const unsigned tr0 = lds_base + cur * BUF_B + half * HALF_B + tr_b0;
    const unsigned tr1 = lds_base + cur * BUF_B + half * HALF_B + tr_b1;

    // wave-uniform: EXEC is all ones at the transposed reads inside
    bool wave_active = kv0h < kv_hi_key;
    if (CAUSAL && kv0h > q0 + 31 + shift) wave_active = false;
    if (HAS_WINDOW && wl >= 0 && kv0h + 64 <= q0 + shift - wl)
      wave_active = false;

    if (wave_active) {
      // swapped S and dP^T: D[key=CROW][q=col]
      f32x16 s[2], dp[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        s[kb] = f32x16(0.f);
        dp[kb] = f32x16(0.f);
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const unsigned byte = ((t & 1) ? (row_off ^ 32u) : row_off) +
                                (t >> 1) * 512 + kb * 4 * (16 * D);
          bf16x8 kf = *reinterpret_cast<const bf16x8*>(kcur + byte);
          bf16x8 vf = *reinterpret_cast<const bf16x8*>(kcur + TILE_B + byte);
          s[kb] = AttnElem<FP16>::mfma(kf, qfrag[t], s[kb]);
          dp[kb] = AttnElem<FP16>::mfma(vf, dofrag[t], dp[kb]);
        }
      }
      // reuse dp as dS (register budget)
      const bool lane_ok = row_ok && isfinite(lse_q);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0h + kb * 32 + CROW(r, hi);
          bool valid = lane_ok && (key < klimit);
          if (CAUSAL) valid &= (key <= qrow + shift);
          if (HAS_WINDOW && wl >= 0) valid &= (key >= qrow + shift - wl);
          if (HAS_WINDOW && wr >= 0 && !CAUSAL)
            valid &= (key <= qrow + shift + wr);
          const float p = valid ? __expf(s[kb][r] * scale - lse_q) : 0.f;
          dp[kb][r] = p * (dp[kb][r] - del_q) * scale;
        }
      }
      // dQ[q][d] += dS[q][key] K[key][d]; the B operand comes from the same
      // K image by ds_read_b64_tr_b16: tr0 (j = 0..3) / tr1 (j = 4..7)
      // + (kb*4 + tp*2)*16*D + a*512 as the offset: immediate
      //
      // Software-pipelined like the dkv steps, NA reads (one row of steps,
      // (kb, tp) fixed) ahead: the reads of row r+1 are issued one per step
      // of row r, before that step's MFMA, and each step waits with a
      // counted lgkmcnt for its own pair only. The wait statement names the
      // pair as in/out operands, so the MFMA depends on it.
#define DQ_TR_DECL(n_) attn_u32x2 kl##n_, kh##n_
#define DQ_TR_ISSUE(n_, kb_, tp_, a_)                                      \
      asm volatile(                                                        \
          "ds_read_b64_tr_b16 %0, %2 offset:%c4\n\t"                     \
          "ds_read_b64_tr_b16 %1, %3 offset:%c4"                          \
          : "=v"(kl##n_), "=v"(kh##n_)                                     \
          : "v"(tr0), "v"(tr1),                                            \
            "i"(((kb_) * 4 + (tp_) * 2) * 16 * D + (a_) * 512))
#define DQ_TR_MFMA(n_, cnt_, a_, dsb_)                                     \
      {                                                                    \
        asm volatile("s_waitcnt lgkmcnt(" #cnt_ ")"                        \
                     : "+v"(kl##n_), "+v"(kh##n_));                        \
        attn_u32x4 uk_ = {kl##n_.x, kl##n_.y, kh##n_.x, kh##n_.y};         \
        bf16x8 ktb = __builtin_bit_cast(bf16x8, uk_);                      \
        dqacc[a_] = AttnElem<FP16>::mfma(dsb_, ktb, dqacc[a_]);            \
      }
#define DQ_PACK(r_, kb_, tp_)                                              \
      unsigned dsfr##r_[4];                                                \
      t12_pack_frag<AttnElem<FP16>>(dp[kb_], tp_, dsfr##r_);               \
      const bf16x8 dsb##r_ = *reinterpret_cast<const bf16x8*>(dsfr##r_)
      if constexpr (NA > 2) {
        // step n = 4*row + a, row = 2*kb + tp; NA = 4 pairs (8 reads) ahead
        DQ_TR_DECL(0); DQ_TR_DECL(1); DQ_TR_DECL(2); DQ_TR_DECL(3);
        DQ_TR_DECL(4); DQ_TR_DECL(5); DQ_TR_DECL(6); DQ_TR_DECL(7);
        DQ_TR_DECL(8); DQ_TR_DECL(9); DQ_TR_DECL(10); DQ_TR_DECL(11);
        DQ_TR_DECL(12); DQ_TR_DECL(13); DQ_TR_DECL(14); DQ_TR_DECL(15);
        DQ_TR_ISSUE(0, 0, 0, 0); DQ_TR_ISSUE(1, 0, 0, 1);
        DQ_TR_ISSUE(2, 0, 0, 2); DQ_TR_ISSUE(3, 0, 0, 3);
        DQ_PACK(0, 0, 0);
        DQ_TR_ISSUE(4, 0, 1, 0); DQ_TR_MFMA(0, 8, 0, dsb0);
        DQ_TR_ISSUE(5, 0, 1, 1); DQ_TR_MFMA(1, 8, 1, dsb0);
        DQ_TR_ISSUE(6, 0, 1, 2); DQ_TR_MFMA(2, 8, 2, dsb0);
        DQ_TR_ISSUE(7, 0, 1, 3); DQ_TR_MFMA(3, 8, 3, dsb0);
        DQ_PACK(1, 0, 1);
        DQ_TR_ISSUE(8, 1, 0, 0); DQ_TR_MFMA(4, 8, 0, dsb1);
        DQ_TR_ISSUE(9, 1, 0, 1); DQ_TR_MFMA(5, 8, 1, dsb1);
        DQ_TR_ISSUE(10, 1, 0, 2); DQ_TR_MFMA(6, 8, 2, dsb1);
        DQ_TR_ISSUE(11, 1, 0, 3); DQ_TR_MFMA(7, 8, 3, dsb1);
        DQ_PACK(2, 1, 0);
        DQ_TR_ISSUE(12, 1, 1, 0); DQ_TR_MFMA(8, 8, 0, dsb2);
        DQ_TR_ISSUE(13, 1, 1, 1); DQ_TR_MFMA(9, 8, 1, dsb2);
        DQ_TR_ISSUE(14, 1, 1, 2); DQ_TR_MFMA(10, 8, 2, dsb2);
        DQ_TR_ISSUE(15, 1, 1, 3); DQ_TR_MFMA(11, 8, 3, dsb2);
        DQ_PACK(3, 1, 1);
        DQ_TR_MFMA(12, 6, 0, dsb3);
        DQ_TR_MFMA(13, 4, 1, dsb3);
        DQ_TR_MFMA(14, 2, 2, dsb3);
        DQ_TR_MFMA(15, 0, 3, dsb3);
      } else {
        // step n = 2*row + a; NA = 2 pairs (4 reads) ahead
        DQ_TR_DECL(0); DQ_TR_DECL(1); DQ_TR_DECL(2); DQ_TR_DECL(3);
        DQ_TR_DECL(4); DQ_TR_DECL(5); DQ_TR_DECL(6); DQ_TR_DECL(7);
        DQ_TR_ISSUE(0, 0, 0, 0); DQ_TR_ISSUE(1, 0, 0, 1);
        DQ_PACK(0, 0, 0);
        DQ_TR_ISSUE(2, 0, 1, 0); DQ_TR_MFMA(0, 4, 0, dsb0);
        DQ_TR_ISSUE(3, 0, 1, 1); DQ_TR_MFMA(1, 4, 1, dsb0);
        DQ_PACK(1, 0, 1);
        DQ_TR_ISSUE(4, 1, 0, 0); DQ_TR_MFMA(2, 4, 0, dsb1);
        DQ_TR_ISSUE(5, 1, 0, 1); DQ_TR_MFMA(3, 4, 1, dsb1);
        DQ_PACK(2, 1, 0);
        DQ_TR_ISSUE(6, 1, 1, 0); DQ_TR_MFMA(4, 4, 0, dsb2);
        DQ_TR_ISSUE(7, 1, 1, 1); DQ_TR_MFMA(5, 4, 1, dsb2);
        DQ_PACK(3, 1, 1);
        DQ_TR_MFMA(6, 2, 0, dsb3);
        DQ_TR_MFMA(7, 0, 1, dsb3);
      }
#undef DQ_PACK
#undef DQ_TR_DECL
#undef DQ_TR_ISSUE
#undef DQ_TR_MFMA
    }
    // ---- write the prefetched half to the OTHER buffer: all waves left it
    // at the barrier that ended the previous tile --------------------------
    if (has_next) half_store(cur ^ 1, half);
    }  // half
    // one barrier per tile: publishes buffer cur^1 and retires this tile's
    // reads of buffer cur before the next tile's writes to it
    __syncthreads();
  }

  // epilogue: D[q = q0 + CROW(r,hi)][d = a*32 + col]
#pragma unroll
  for (int a = 0; a < NA; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q_r = q0 + CROW(r, hi);
      const int d = a * 32 + col;
      if (q_r < sq) {
        const long obase = ((long)(b * sq + q_r) * hq + h) * D;
        dQ[obase + d] = (q_r < qlimit)
            ? AttnElem<FP16>::from_f32(dqacc[a][r]) : (short)0;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

template <int D, bool FP16>
static void launch_fa_bwd(const torch::Tensor& dout, const torch::Tensor& q,
                          const torch::Tensor& k, const torch::Tensor& v,
                          const torch::Tensor& lse,
                          const torch::Tensor& delta, torch::Tensor& dq,
                          torch::Tensor& dk, torch::Tensor& dv, float scale,
                          bool causal, int wl, int wr, const int* qlp,
                          const int* klp, hipStream_t stream) {
  const int b = q.size(0), sq = q.size(1), hq = q.size(2);
  const int sk = k.size(1), hk = k.size(2);
  const bool has_window = (wl >= 0 || wr >= 0);
  const bool has_lens = qlp != nullptr || klp != nullptr;

#define ARGS_DKV                                                             \
  (const short*)dout.data_ptr(), (const short*)q.data_ptr(),                 \
      (const short*)k.data_ptr(), (const short*)v.data_ptr(),                \
      lse.data_ptr<float>(), delta.data_ptr<float>(),                        \
      (short*)dk.data_ptr(), (short*)dv.data_ptr(), b, sq, sk, hq, hk,       \
      scale, wl, wr, qlp, klp
#define ARGS_DQ                                                              \
  (const short*)dout.data_ptr(), (const short*)q.data_ptr(),                 \
      (const short*)k.data_ptr(), (const short*)v.data_ptr(),                \
      lse.data_ptr<float>(), delta.data_ptr<float>(),                        \
      (short*)dq.data_ptr(), b, sq, sk, hq, hk, scale, wl, wr, qlp, klp

  dim3 gkv((sk + 127) / 128, b * hk), bkv(256);
  // 2 x (Q + dO image) + V image + 2 x (lse + delta)
  const int lds_kv = (4 * 32 * D + 128 * D) * 2 + 4 * 32 * 4;
  dim3 gq((sq + 255) / 256, b * hq), bq(512);
  const int lds_q = 4 * 128 * D * 2;   // 2 x (K image + V image)

#define DISPATCH(C, W, L)                                                    \
  do {                                                                       \
    hipLaunchKernelGGL((fa_bwd_dkv_kernel<D, C, W, L, FP16>), gkv, bkv,     \
                       lds_kv, stream, ARGS_DKV);                            \
    hipLaunchKernelGGL((fa_bwd_dq_kernel<D, C, W, L, FP16>), gq, bq, lds_q,  \
                       stream, ARGS_DQ);                                     \
  } while (0)

  if (causal) {
    if (has_window) { if (has_lens) DISPATCH(true, true, true); else DISPATCH(true, true, false); }
    else { if (has_lens) DISPATCH(true, false, true); else DISPATCH(true, false, false); }
  } else {
    if (has_window) { if (has_lens) DISPATCH(false, true, true); else DISPATCH(false, true, false); }
    else { if (has_lens) DISPATCH(false, false, true); else DISPATCH(false, false, false); }
  }
#undef DISPATCH
#undef ARGS_DKV
#undef ARGS_DQ
}

std::vector<torch::Tensor> fa_backward_extra(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, double softmax_scale, bool causal,
    long wl, long wr, torch::Tensor q_lens, torch::Tensor k_lens,
    torch::Tensor alibi_slopes, double p_drop, long rng_seed);

std::vector<torch::Tensor> fa_backward(torch::Tensor dout, torch::Tensor q,
                                       torch::Tensor k, torch::Tensor v,
                                       torch::Tensor out, torch::Tensor lse,
                                       double softmax_scale, bool causal,
                                       long wl, long wr, torch::Tensor q_lens,
                                       torch::Tensor k_lens,
                                       torch::Tensor alibi_slopes,
                                       double p_drop, long rng_seed) {
  if (alibi_slopes.numel() > 0 || p_drop > 0.0) {
    return fa_backward_extra(dout, q, k, v, out, lse, softmax_scale, causal,
                             wl, wr, q_lens, k_lens, alibi_slopes, p_drop,
                             rng_seed);
  }
  TORCH_CHECK(q.is_cuda() && (q.scalar_type() == torch::kBFloat16 ||
                              q.scalar_type() == torch::kHalf),
              "fa_backward: bf16/fp16 only");
  const bool fp16 = q.scalar_type() == torch::kHalf;
  TORCH_CHECK(dout.is_contiguous() && q.is_contiguous() &&
              k.is_contiguous() && v.is_contiguous());
  const int b = q.size(0), sq = q.size(1), hq = q.size(2), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128);
  auto stream = at::hip::getCurrentHIPStream();
  auto lse_c = lse.contiguous();
  auto delta = torch::empty_like(lse_c);
  {
    const long rows = (long)b * sq * hq;
    // 4 waves per block, 64 / (D/8) rows per wave
    const long rpb = 4 * (WAVE / (D / 8));
    const long grid = (rows + rpb - 1) / rpb;
#define PRE_LAUNCH(F, DD)                                                    \
    hipLaunchKernelGGL((fa_bwd_preprocess_kernel<F, DD>),                    \
                       dim3((unsigned)grid), dim3(256), 0, stream,           \
                       (const short*)dout.data_ptr(),                        \
                       (const short*)out.data_ptr(),                         \
                       delta.data_ptr<float>(), b, sq, hq)
    if (D == 128) {
      if (fp16) PRE_LAUNCH(true, 128); else PRE_LAUNCH(false, 128);
    } else {
      if (fp16) PRE_LAUNCH(true, 64); else PRE_LAUNCH(false, 64);
    }
#undef PRE_LAUNCH
  }
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto ql = q_lens.numel() ? q_lens.to(q.device(), torch::kInt32) : q_lens;
  auto kl = k_lens.numel() ? k_lens.to(q.device(), torch::kInt32) : k_lens;
  const int* qlp = ql.numel() ? ql.data_ptr<int>() : nullptr;
  const int* klp = kl.numel() ? kl.data_ptr<int>() : nullptr;
  if (D == 128) {
    if (fp16)
      launch_fa_bwd<128, true>(dout, q, k, v, lse_c, delta, dq, dk, dv,
                               (float)softmax_scale, causal, (int)wl,
                               (int)wr, qlp, klp, stream);
    else
      launch_fa_bwd<128, false>(dout, q, k, v, lse_c, delta, dq, dk, dv,
                                (float)softmax_scale, causal, (int)wl,
                                (int)wr, qlp, klp, stream);
  } else {
    if (fp16)
      launch_fa_bwd<64, true>(dout, q, k, v, lse_c, delta, dq, dk, dv,
                              (float)softmax_scale, causal, (int)wl,
                              (int)wr, qlp, klp, stream);
    else
      launch_fa_bwd<64, false>(dout, q, k, v, lse_c, delta, dq, dk, dv,
                               (float)softmax_scale, causal, (int)wl,
                               (int)wr, qlp, klp, stream);
  }
  HIP_CHECK_LAST();
  return {dq, dk, dv};
}
