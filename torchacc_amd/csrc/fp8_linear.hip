// Weight-only fp8 (e4m3) linear layers (W8A16):
//   y[M,N] = (x[M,K] @ dequant(W8[N,K])^T) * scale[N] (+ bias[N])
// W8 e4m3 codes, row-major; one fp32 scale per output channel, which
// multiplies the fp32 accumulator once, in the epilogue. A decode step is
// bound by reading the projection weights once; e4m3 halves those bytes
// against the 16-bit paths in gemm.hip. Operand order, batch invariance and
// tail rules are in wq_gemm_common.h, whose host front end (operand checks,
// split rule, allocate / launch / combine), MFMA wrappers, x-image layout and
// stage barrier this file uses; its kernels are its own (folded onto the
// shared frame and epilogue they ran 1-7 % slower,
// profiles/r21_wq_gemm_refactor.md).
//
// Skinny weight stream (v_mfma_f32_16x16x32: lane l holds weight row l&15,
// k-slots 8*(l>>4)..+7): a lane reads 16 contiguous codes of its row per
// 16-byte load; the four lane groups of a row cover 64 contiguous bytes, and a
// step issues the two loads of a 128-byte line back to back: 128 codes per
// row and step. The 16 codes feed two MFMA K-steps (codes 0..7, then 8..15).
// The reduction order inside K is free, so the x fragment simply follows the
// same permutation: lane (j, g) reads x[j][k0 + 16g + 8s .. +7] for K-step s,
// 32 contiguous bytes.
//
// e4m3 -> 16 bit is exact (3 mantissa bits): v_cvt_pk_f32_fp8, then
// v_cvt_pk_bf16_f32 (bf16) or v_cvt_pkrtz (fp16).
//
// Three ways to fill the device:
//   fp8_linear         4 waves on 32 channels; where N/32 workgroups are too
//                      few, K is also cut across S workgroups that write fp32
//                      partials, summed by a second launch (the split-KV
//                      combine pattern). Any M, in 64-row blocks.
//   fp8_linear_wide,   ONE launch for every (N, K), M <= 64: at batch 1 a
//   fp8_swiglu_linear  layer's projections are bound by launch count, not
//                      bytes (profiles/r17_fp8_one_launch.md), so K is cut
//                      only across the 4 or 8 waves of a workgroup on 16 or 32
//                      channels (opt-in, one_launch=True).
//   fp8_gemm           M > 64 (prefill, mixed serving steps), further down.
#include <vector>

#include "wq_gemm_common.h"

// packed fp32 VALU forms are kept out of this file's device code
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

constexpr int FP8L_WAVES = 4;     // waves per workgroup, all on the same tiles
constexpr int FP8L_NT = 2;        // 16-channel tiles per wave
constexpr int FP8L_BN = 16 * FP8L_NT;
constexpr int FP8L_STEP = 128;    // codes per wave step: one 128-byte line/row
constexpr int FP8L_MAX_SPLITS = 16;
// workgroups per CU the K split aims for; 2 x 4 waves with a whole step of
// loads in flight each (profiles/r15_fp8_linear.md)
constexpr int FP8L_WG_PER_CU = 2;

template <bool FP16>
struct Fp8lElem;

template <>
struct Fp8lElem<false> {
  // two e4m3 codes as fp32 -> bf16 pair in one dword. v_cvt_pk_bf16_f32 is
  // exact here (3 mantissa bits). Integer forms on the bit-cast elements
  // (shift/mask, __builtin_amdgcn_perm) were compiled to read element 0 of
  // the convert's result pair twice, so the float-domain convert is used.
  static DEVINLINE unsigned pack(f32x2 f) {
    return __builtin_bit_cast(unsigned,
                              __builtin_convertvector(f, wq_bf16x2));
  }
};

template <>
struct Fp8lElem<true> {
  static DEVINLINE unsigned pack(f32x2 f) {
    return AttnElem<true>::cvt_pk(f[0], f[1]);
  }
};

// 8 e4m3 codes (two dwords) -> one 16-bit x8 MFMA A fragment
template <bool FP16>
DEVINLINE attn_u32x4 fp8l_cvt8(unsigned c0, unsigned c1) {
  attn_u32x4 a;
  a[0] = Fp8lElem<FP16>::pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)c0, false));
  a[1] = Fp8lElem<FP16>::pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)c0, true));
  a[2] = Fp8lElem<FP16>::pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)c1, false));
  a[3] = Fp8lElem<FP16>::pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)c1, true));
  return a;
}

// Scale, bias, convert and store channels n..n+3 (n % 4 == 0) of row m.
template <bool FP16>
DEVINLINE void fp8l_finish4(f32x4 v, long m, int n, int N,
                            const float* __restrict__ scale,
                            const short* __restrict__ bias,
                            short* __restrict__ y) {
  if ((N & 3) == 0) {  // then n + 3 < N and the row start is 8-byte aligned
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + n);
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = v[r] * sc[r];
    if (bias != nullptr) {
      const s16x4 bv = *reinterpret_cast<const s16x4*>(bias + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] += AttnElem<FP16>::to_f32(bv[r]);
    }
    s16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = AttnElem<FP16>::from_f32(o[r]);
    *reinterpret_cast<s16x4*>(y + m * N + n) = ov;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (n + r < N) {
        float o = v[r] * scale[n + r];
        if (bias != nullptr) o += AttnElem<FP16>::to_f32(bias[n + r]);
        y[m * N + n + r] = AttnElem<FP16>::from_f32(o);
      }
    }
  }
}

// One 128-code step of a wave: for each half (64 codes) every lane loads its
// 16 codes of both tiles and its 16 activations of every column block, then
// 2 K-steps x NT x MT MFMAs. TAIL is the one ragged step at the end of K
// (K % 128 != 0): 16-code granules at or past K contribute zeros. NT is
// deduced from the row pointers (2 everywhere but the one-tile wide kernel).
template <bool FP16, int MT, bool TAIL, int NT>
DEVINLINE void fp8l_step(const unsigned char* const (&wrow)[NT],
                         const short* const (&xrow)[MT], int kl, int K,
                         f32x4 (&acc)[NT][MT]) {
  attn_u32x4 wv[2][NT];
  attn_u32x4 xv[2][MT][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = kl + h * 64;          // this lane's 16 codes: [k, k + 16)
    const bool live = !TAIL || k < K;
    const int kc = live ? k : 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      wv[h][nt] = *reinterpret_cast<const attn_u32x4*>(wrow[nt] + kc);
      if (TAIL && !live) wv[h][nt] = attn_u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        xv[h][mt][s] =
            *reinterpret_cast<const attn_u32x4*>(xrow[mt] + kc + 8 * s);
        if (TAIL && !live) xv[h][mt][s] = attn_u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const attn_u32x4 a =
            fp8l_cvt8<FP16>(wv[h][nt][2 * s], wv[h][nt][2 * s + 1]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[nt][mt] = wq_mfma16<FP16>(a, xv[h][mt][s], acc[nt][mt]);
      }
    }
  }
}

// grid = (ceil(N/32), S, ceil(M/64)); block = 256.
// S == 1: writes y. S > 1: writes raw fp32 sums to part[S][M][N].
template <bool FP16, int MT>
__global__ __launch_bounds__(FP8L_WAVES * WAVE)
void fp8_linear_kernel(const short* __restrict__ x,
                       const unsigned char* __restrict__ w,
                       const float* __restrict__ scale,
                       const short* __restrict__ bias,
                       short* __restrict__ y, float* __restrict__ part,
                       int M, int N, int K) {
  __shared__ f32x4 red[FP8L_WAVES][FP8L_NT * MT][WAVE];
  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid % WAVE;
  const int j = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * FP8L_BN;
  const int split = blockIdx.y, S = gridDim.y;
  const int mb = blockIdx.z * 64;

  // contiguous, balanced runs of steps over the S * 4 wave slots
  const int T = (K + FP8L_STEP - 1) / FP8L_STEP, Tfull = K / FP8L_STEP;
  const int slots = S * FP8L_WAVES, slot = split * FP8L_WAVES + wave;
  const int t0 = (int)((long)slot * T / slots);
  const int t1 = (int)((long)(slot + 1) * T / slots);

  // rows past the end are clamped: loaded, multiplied, never stored
  const unsigned char* wrow[FP8L_NT];
#pragma unroll
  for (int nt = 0; nt < FP8L_NT; ++nt)
    wrow[nt] = w + (long)min(n0 + nt * 16 + j, N - 1) * K;
  const short* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] = x + (long)min(mb + mt * 16 + j, M - 1) * K;

  f32x4 acc[FP8L_NT][MT];
#pragma unroll
  for (int nt = 0; nt < FP8L_NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tm = min(t1, Tfull);
#pragma unroll 2
  for (int t = t0; t < tm; ++t)
    fp8l_step<FP16, MT, false>(wrow, xrow, t * FP8L_STEP + g * 16, K, acc);
  if (t1 > Tfull)  // only the last slot, only when K % 128 != 0
    fp8l_step<FP16, MT, true>(wrow, xrow, Tfull * FP8L_STEP + g * 16, K, acc);

  // the four waves' sums, added in wave order
#pragma unroll
  for (int i = 0; i < FP8L_NT * MT; ++i) red[wave][i][lane] = acc[i / MT][i % MT];
  __syncthreads();
  for (int idx = tid; idx < FP8L_NT * MT * WAVE; idx += FP8L_WAVES * WAVE) {
    const int i = idx / WAVE, l = idx % WAVE;
    f32x4 v = red[0][i][l];
#pragma unroll
    for (int wv = 1; wv < FP8L_WAVES; ++wv) v += red[wv][i][l];
    const int m = mb + (i % MT) * 16 + (l & 15);
    const int n = n0 + (i / MT) * 16 + 4 * (l >> 4);
    if (m >= M || n >= N) continue;
    if (S == 1) {
      fp8l_finish4<FP16>(v, m, n, N, scale, bias, y);
    } else {
      float* p = part + ((long)split * M + m) * N + n;
      if ((N & 3) == 0) {
        *reinterpret_cast<f32x4*>(p) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) p[r] = v[r];
      }
    }
  }
}

// y = (sum over splits, in split order) * scale + bias; a thread per four
// channels of one row.
template <bool FP16>
__global__ __launch_bounds__(256)
void fp8_linear_combine_kernel(const float* __restrict__ part,
                               const float* __restrict__ scale,
                               const short* __restrict__ bias,
                               short* __restrict__ y, int M, int N, int S) {
  const int n4 = (N + 3) / 4;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)M * n4) return;
  const long m = idx / n4;
  const int n = (int)(idx % n4) * 4;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const float* p = part + ((long)s * M + m) * N + n;
    if ((N & 3) == 0) {
      v += *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) v[r] += p[r];
    }
  }
  fp8l_finish4<FP16>(v, m, n, N, scale, bias, y);
}

// ---------------------------------------------------------------------------
// fp8_wide: the skinny GEMM in ONE launch for every (N, K). At batch 1 a
// layer's projections are bound by launch count, not bytes
// (profiles/r17_fp8_one_launch.md), so K is never cut across workgroups: no
// partials, no combine launch, no allocation besides y. The device is filled
// from the other side instead: a workgroup is W in {4, 8} waves on only 16 or
// 32 channels, each wave on its own contiguous, balanced run of 128-code
// steps (fp8_linear_kernel's slot arithmetic with S = 1), and the W
// accumulators are summed through LDS in wave order. W and NT are compile-time
// instances picked from (N, K, CU count) alone, so no K boundary moves with
// the batch; a row's bits are the same for every MT.
//
// Two epilogues on that body:
//   PLAIN   y = acc * scale (+ bias); NT in {1, 2} tiles of one weight.
//   SWIGLU  the wave's two tiles are tile i of the GATE weight and tile i of
//           the UP weight (two pointers, two scale vectors, nothing
//           interleaved): one x fragment feeds both, a workgroup owns 16
//           channels of y = silu(g * sg (+ bg)) * (u * su (+ bu)). The two
//           pre-activations stay fp32 in registers / LDS: they are never
//           rounded to 16 bit and never reach memory.
//
// LDS: red[W][NT * MT][64] f32x4, at most 8 * 8 * 1 KiB = 64 KiB (W = 8,
// NT = 2, MT = 4); after one barrier thread (i, l) sums slot (i, l) of waves
// 0..W-1 in that order and runs the epilogue for its 4 channels of one row.
// Tails as in fp8_linear_kernel: channels >= N read a clamped row and are
// predicated at the store, rows >= M read row M-1 and are never stored, the
// one ragged step zero-fills 16-code granules at or past K. M <= 64.

// silu(g) * u for channels n..n+3 of row m; fp8l_finish4's store rule.
template <bool FP16>
DEVINLINE void fp8w_finish4_swiglu(f32x4 vg, f32x4 vu, long m, int n, int N,
                                   const float* __restrict__ sg,
                                   const float* __restrict__ su,
                                   const short* __restrict__ bg,
                                   const short* __restrict__ bu,
                                   short* __restrict__ y) {
  const bool vec = (N & 3) == 0;  // then n + 3 < N, 8-byte aligned row start
  s16x4 ov;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = vec ? n + r : min(n + r, N - 1);
    float g = vg[r] * sg[c], u = vu[r] * su[c];
    if (bg != nullptr) g += AttnElem<FP16>::to_f32(bg[c]);
    if (bu != nullptr) u += AttnElem<FP16>::to_f32(bu[c]);
    // exp overflows to +inf for g < -88: the quotient is then -0, silu's limit
    ov[r] = AttnElem<FP16>::from_f32(g / (1.f + __expf(-g)) * u);
  }
  if (vec) {
    *reinterpret_cast<s16x4*>(y + m * N + n) = ov;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < N) y[m * N + n + r] = ov[r];
  }
}

// grid = ceil(N / BN), BN = 16 (SWIGLU, or NT == 1) or 32; block = W * 64.
// PLAIN reads (w0, s0, b0) only.
template <bool FP16, int MT, int W, int NT, bool SWIGLU>
__global__ __launch_bounds__(W * WAVE)
void fp8_wide_kernel(const short* __restrict__ x,
                     const unsigned char* __restrict__ w0,
                     const unsigned char* __restrict__ w1,
                     const float* __restrict__ s0,
                     const float* __restrict__ s1,
                     const short* __restrict__ b0,
                     const short* __restrict__ b1,
                     short* __restrict__ y, int M, int N, int K) {
  static_assert(!SWIGLU || NT == 2, "SWIGLU: one gate tile, one up tile");
  static_assert(W * NT * MT * WAVE * sizeof(f32x4) <= 64 * 1024, "LDS");
  constexpr int BN = SWIGLU ? 16 : 16 * NT;
  __shared__ f32x4 red[W][NT * MT][WAVE];
  const int tid = threadIdx.x, lane = tid % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int j = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * BN;

  // contiguous, balanced runs of steps over the W waves
  const int T = (K + FP8L_STEP - 1) / FP8L_STEP, Tfull = K / FP8L_STEP;
  const int t0 = (int)((long)wave * T / W);
  const int t1 = (int)((long)(wave + 1) * T / W);

  const unsigned char* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (SWIGLU)
      wrow[nt] = (nt == 0 ? w0 : w1) + (long)min(n0 + j, N - 1) * K;
    else
      wrow[nt] = w0 + (long)min(n0 + nt * 16 + j, N - 1) * K;
  }
  const short* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] = x + (long)min(mt * 16 + j, M - 1) * K;

  f32x4 acc[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tm = min(t1, Tfull);
#pragma unroll 2
  for (int t = t0; t < tm; ++t)
    fp8l_step<FP16, MT, false>(wrow, xrow, t * FP8L_STEP + g * 16, K, acc);
  if (t1 > Tfull)  // only the last wave, only when K % 128 != 0
    fp8l_step<FP16, MT, true>(wrow, xrow, Tfull * FP8L_STEP + g * 16, K, acc);

#pragma unroll
  for (int i = 0; i < NT * MT; ++i) red[wave][i][lane] = acc[i / MT][i % MT];
  __syncthreads();
  // SWIGLU: one item per (column block, lane) takes the gate and the up sum
  constexpr int ITEMS = (SWIGLU ? 1 : NT) * MT * WAVE;
  for (int idx = tid; idx < ITEMS; idx += W * WAVE) {
    const int i = idx / WAVE, l = idx % WAVE;
    const int m = (i % MT) * 16 + (l & 15);
    const int n = n0 + (i / MT) * 16 + 4 * (l >> 4);
    if (m >= M || n >= N) continue;
    f32x4 v = red[0][i][l];
#pragma unroll
    for (int wv = 1; wv < W; ++wv) v += red[wv][i][l];
    if constexpr (SWIGLU) {
      f32x4 u = red[0][MT + i][l];
#pragma unroll
      for (int wv = 1; wv < W; ++wv) u += red[wv][MT + i][l];
      fp8w_finish4_swiglu<FP16>(v, u, m, n, N, s0, s1, b0, b1, y);
    } else {
      fp8l_finish4<FP16>(v, m, n, N, s0, b0, y);
    }
  }
}

// ---------------------------------------------------------------------------
// fp8_gemm: the same formula for M > 64 (prefill, mixed serving steps), as a
// tiled GEMM that reads every code once per row tile and converts it once.
//
// A workgroup of 4 waves computes 128 x rows by 128 channels over BK = 64
// steps; the waves sit 2 (channels) x 2 (rows), each on 64 x 64 as 2 x 2 tiles
// of v_mfma_f32_32x32x16_{bf16,f16}. As in the skinny kernel the WEIGHTS are
// the A operand, so the result is y^T: lane l owns x row l&31 of a tile and,
// per group of four accumulator registers q, the four consecutive channels
// 8q + 4(l>>5)..+3: the epilogue is fp8l_finish4.
//
// LDS: two stages of (x image, weight image), both [128 rows][64 x 16 bit]
// row-major with 128-byte rows whose eight 16-byte chunks are XORed with
// (row>>1)&7, 16 KiB each, 64 KiB in all (two workgroups per CU). A lane's A
// or B fragment of K-step kk is chunk 2kk + (l>>5) of row l&31: one
// ds_read_b128, and 16 consecutive lanes (rows 16n..16n+15, one chunk) touch
// the 16 distinct 16-byte slots of the 256-byte bank line.
//   x goes global -> LDS directly (attn_glds16); a wave instruction fills 64
//   consecutive slots (8 rows), and the swizzle goes on the source address.
//   Rows >= M read row M-1 and are never stored.
//   Weights: a thread loads 2 x 16 codes of stage t+1 before the MFMAs of
//   stage t, converts them after those MFMAs (fp8l_cvt8, exact) and writes
//   them as 16-bit chunks with ds_write_b128: every code is converted once
//   per workgroup. Channels >= N read row N-1 and are predicated at the store.
//   One barrier per stage. The ragged step (K % 64 != 0) is always the last
//   one: it stages x through registers so that 16-code granules at or past K
//   are zero in both operands.
//
// Filling the device: where the tiles are fewer than the CUs, K is cut over
// S workgroups (grid.z) that write fp32 partials [S][M][N], summed in split
// order by fp8_linear_combine_kernel. No atomics: results are bitwise
// repeatable and depend on (M, N, K, CU count) only. S depends on M, so unlike
// the skinny kernel this path does NOT promise that a row's bits are
// independent of the batch it sits in.
constexpr int FP8G_TILE_B = WQG_X_B;               // one 16-bit image
constexpr int FP8G_STAGE_B = 2 * FP8G_TILE_B;      // x image, weight image
static_assert(WQG_BM == WQG_BA, "both images share wqg_xoff");

// grid = (ceil(N/128), ceil(M/128), S); block = 256.
// S == 1: writes y. S > 1: writes raw fp32 sums to part[S][M][N].
template <bool FP16>
__global__ __launch_bounds__(256, 2)
void fp8_gemm_kernel(const short* __restrict__ x,
                     const unsigned char* __restrict__ w,
                     const float* __restrict__ scale,
                     const short* __restrict__ bias,
                     short* __restrict__ y, float* __restrict__ part,
                     int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char lds[2 * FP8G_STAGE_B];
  const int tid = threadIdx.x, lane = tid % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int wn = wave & 1, wm = wave >> 1;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n0 = blockIdx.x * WQG_BA, m0 = blockIdx.y * WQG_BM;
  const int split = blockIdx.z, S = gridDim.z;

  // contiguous, balanced runs of BK steps over the splits; the host keeps
  // S <= T, so every split owns at least one step
  const int T = (K + WQG_BK - 1) / WQG_BK, Tfull = K / WQG_BK;
  const int t0 = (int)((long)split * T / S);
  const int t1 = (int)((long)(split + 1) * T / S);

  // x staging: pass i fills slots i*256 + tid of the image, slot s = row
  // s>>3, stored chunk s&7, which holds logical chunk (s&7) ^ ((row>>1)&7);
  // the row's bits 1..3 are tid's bits 4..6 in every pass
  const int xc = (tid & 7) ^ ((tid >> 4) & 7);
  const short* xsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    xsrc[i] = x + (long)min(m0 + i * 32 + (tid >> 3), M - 1) * K + xc * 8;
  // weight staging: pass i, row i*64 + tid>>2, codes 16*(tid&3)..+15 of the
  // step, i.e. 16-bit chunks 2*(tid&3) and the next one
  const int wq = tid & 3;
  const unsigned char* wsrc[2];
  unsigned wdst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = i * 64 + (tid >> 2);
    wsrc[i] = w + (long)min(n0 + row, N - 1) * K + wq * 16;
    wdst[i] = FP8G_TILE_B + wqg_xoff(row, 2 * wq);
  }

  // issue the loads of step t: x into buffer `buf`, the codes into wv
  auto stage_load = [&](int t, int buf, attn_u32x4 (&wv)[2]) {
    const int k0 = t * WQG_BK;
    const bool tail = t >= Tfull;
    char* xi = lds + buf * FP8G_STAGE_B;
    if (!tail) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        attn_glds16(xsrc[i] + k0, xi + (i * 256 + wave * WAVE) * 16);
    } else {
      const bool live = k0 + xc * 8 < K;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        attn_u32x4 v = attn_u32x4{0u, 0u, 0u, 0u};
        if (live) v = *reinterpret_cast<const attn_u32x4*>(xsrc[i] + k0);
        *reinterpret_cast<attn_u32x4*>(xi + (i * 256 + tid) * 16) = v;
      }
    }
    const bool wlive = !tail || k0 + wq * 16 < K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      wv[i] = attn_u32x4{0u, 0u, 0u, 0u};
      if (wlive) wv[i] = *reinterpret_cast<const attn_u32x4*>(wsrc[i] + k0);
    }
  };
  // convert the 32 codes and write them into buffer `buf`
  auto stage_commit = [&](int buf, const attn_u32x4 (&wv)[2]) {
    char* base = lds + buf * FP8G_STAGE_B;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<attn_u32x4*>(base + wdst[i]) =
          fp8l_cvt8<FP16>(wv[i][0], wv[i][1]);
      *reinterpret_cast<attn_u32x4*>(base + (wdst[i] ^ 16u)) =
          fp8l_cvt8<FP16>(wv[i][2], wv[i][3]);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  attn_u32x4 wv[2];
  stage_load(t0, 0, wv);
  stage_commit(0, wv);
  wqg_publish<0>();

  // fragment reads: row 32*tile + l31 of the wave's half, chunk 2kk + hi
  const unsigned sw = (unsigned)((l31 >> 1) & 7);
  const unsigned xrow_off = (unsigned)((wm * 64 + l31) * 128);
  const unsigned wrow_off = (unsigned)(FP8G_TILE_B + (wn * 64 + l31) * 128);

  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    const bool more = t + 1 < t1;
    // buffer cur^1 was last read before the barrier that ended step t-1
    if (more) stage_load(t + 1, cur ^ 1, wv);
    const char* base = lds + cur * FP8G_STAGE_B;
#pragma unroll
    for (int kk = 0; kk < WQG_BK / 16; ++kk) {
      const unsigned ch = (((unsigned)(2 * kk + hi)) ^ sw) << 4;
      attn_u32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const attn_u32x4*>(
            base + wrow_off + i * (32 * 128) + ch);
        b[i] = *reinterpret_cast<const attn_u32x4*>(
            base + xrow_off + i * (32 * 128) + ch);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = wq_mfma32<FP16>(a[i], b[j], acc[i][j]);
    }
    if (more) stage_commit(cur ^ 1, wv);
    // publishes buffer cur^1 and retires this step's reads of buffer cur
    wqg_publish<0>();
  }

  // lane: x row m of tile j; registers 4q..4q+3 of tile i: channels n..n+3
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm * 64 + j * 32 + l31;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 64 + i * 32 + 8 * q + 4 * hi;
        if (n >= N) continue;
        const f32x4 v = f32x4{acc[i][j][4 * q], acc[i][j][4 * q + 1],
                              acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        if (S == 1) {
          fp8l_finish4<FP16>(v, m, n, N, scale, bias, y);
        } else {
          float* p = part + ((long)split * M + m) * N + n;
          if ((N & 3) == 0) {
            *reinterpret_cast<f32x4*>(p) = v;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (n + r < N) p[r] = v[r];
          }
        }
      }
    }
  }
}

}  // namespace

#pragma clang attribute pop

namespace {

// the per-format part of wq_operands: w8 [N,K] e4m3, scale [N] fp32
struct Fp8Host {
  static constexpr long K_MULT = 16;
  static void check(const char* op, long K, const torch::Tensor& w8,
                    const torch::Tensor& scale) {
    TORCH_CHECK(scale.dim() == 1 &&
                    w8.scalar_type() == torch::kFloat8_e4m3fn &&
                    scale.scalar_type() == torch::kFloat,
                op, ": w8 [N,K] float8_e4m3fn, scale [N] fp32");
    TORCH_CHECK(w8.size(1) == K && scale.size(0) == w8.size(0),
                op, ": shape mismatch");
    TORCH_CHECK((uintptr_t)scale.data_ptr() % 16 == 0,
                op, ": scale must be 16-byte aligned");
  }
};

// Launch a skinny kernel: fp8_linear_kernel (split: S splits, any M) or the
// (W, NT) instance of fp8_wide_kernel (M <= 64), PLAIN or SWIGLU by the
// operands.
torch::Tensor fp8_skinny(const torch::Tensor& x, const WqOperands& o, long W,
                         long NT, bool split, long S) {
  auto stream = at::hip::getCurrentHIPStream();
  const long bn = o.swiglu ? 16 : 16 * NT;
  const dim3 grid((unsigned)((o.N + bn - 1) / bn), (unsigned)S,
                  (unsigned)(split ? (o.M + 63) / 64 : 1));
  const dim3 block((unsigned)(W * WAVE));
  const int mt = wq_skinny_mt(o.M);
#define FP8W_LAUNCH(MTV, WV, NTV, SW)                                         \
  hipLaunchKernelGGL((fp8_wide_kernel<kFP16, MTV, WV, NTV, SW>), grid, block, \
                     0, stream, o.x, o.w[0], o.w[1], (const float*)o.s[0],    \
                     (const float*)o.s[1], o.b[0], o.b[1], y, (int)o.M,       \
                     (int)o.N, (int)o.K)
#define FP8W_INSTANCE(MTV)                                  \
  do {                                                      \
    if (split) {                                            \
      hipLaunchKernelGGL((fp8_linear_kernel<kFP16, MTV>), grid, block, 0,    \
                         stream, o.x, o.w[0], (const float*)o.s[0], o.b[0],  \
                         y, part, (int)o.M, (int)o.N, (int)o.K);             \
    } else if (o.swiglu) {                                  \
      if (W == 4) FP8W_LAUNCH(MTV, 4, 2, true);             \
      else FP8W_LAUNCH(MTV, 8, 2, true);                    \
    } else if (NT == 1) {                                   \
      if (W == 4) FP8W_LAUNCH(MTV, 4, 1, false);            \
      else FP8W_LAUNCH(MTV, 8, 1, false);                   \
    } else {                                                \
      if (W == 4) FP8W_LAUNCH(MTV, 4, 2, false);            \
      else FP8W_LAUNCH(MTV, 8, 2, false);                   \
    }                                                       \
  } while (0)
  return wq_run(
      x, o, S,
      [&](short* y, float* part) {
        FP16_SWITCH(o.fp16, {
          if (mt == 1) FP8W_INSTANCE(1);
          else if (mt == 2) FP8W_INSTANCE(2);
          else FP8W_INSTANCE(4);
        });
      },
      [&](float* part, short* y, dim3 cgrid) {
        FP16_SWITCH(o.fp16, {
          hipLaunchKernelGGL((fp8_linear_combine_kernel<kFP16>), cgrid,
                             dim3(256), 0, stream, part, (const float*)o.s[0],
                             o.b[0], y, (int)o.M, (int)o.N, (int)S);
        });
      });
#undef FP8W_INSTANCE
#undef FP8W_LAUNCH
}

}  // namespace

// Number of K splits across workgroups for an [N, K] weight on a device with
// num_cus compute units. A function of (N, K, num_cus) only: the batch size
// must not move a K boundary (batch invariance). Every wave slot keeps at
// least one whole step.
long fp8_linear_num_splits(long n, long k, long num_cus) {
  const long wgs = (n + FP8L_BN - 1) / FP8L_BN;
  const long steps = (k + FP8L_STEP - 1) / FP8L_STEP;
  const long want = (FP8L_WG_PER_CU * num_cus + wgs - 1) / wgs;
  const long cap = std::min<long>(FP8L_MAX_SPLITS, steps / FP8L_WAVES);
  return std::max<long>(1, std::min(want, cap));
}

// y = (x @ dequant(w8)^T) * scale (+ bias), any M >= 1. num_splits: 0 =
// chosen from (N, K) and the CU count, otherwise forced (benchmarks, tests).
torch::Tensor fp8_linear(torch::Tensor x, torch::Tensor w8,
                         torch::Tensor scale,
                         c10::optional<torch::Tensor> bias,
                         long num_splits) {
  const char* op = "fp8_linear";
  const auto o = wq_operands<Fp8Host>(op, x, w8, scale, bias, nullptr, nullptr,
                                      c10::nullopt);
  wq_check_skinny_size(op, o, true);
  long S = num_splits;
  if (S <= 0) {
    S = fp8_linear_num_splits(
        o.N, o.K, at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  }
  TORCH_CHECK(S <= FP8L_MAX_SPLITS, op, ": num_splits above ",
              FP8L_MAX_SPLITS);
  S = std::max<long>(1, std::min(S, (o.K + FP8L_STEP - 1) / FP8L_STEP));
  return fp8_skinny(x, o, FP8L_WAVES, FP8L_NT, true, S);
}

// Number of K splits of fp8_gemm for an [M, K] x [N, K]^T problem on a device
// with num_cus compute units (wqg_splits on 128 x 128 tiles).
long fp8_gemm_num_splits(long m, long n, long k, long num_cus) {
  return wqg_splits(m, n, k, num_cus, WQG_BA);
}

// y = (x @ dequant(w8)^T) * scale (+ bias) for any M >= 1, on the tiled
// kernel. num_splits: 0 = chosen from (M, N, K) and the CU count, otherwise
// forced (benchmarks, tests).
torch::Tensor fp8_gemm(torch::Tensor x, torch::Tensor w8, torch::Tensor scale,
                       c10::optional<torch::Tensor> bias, long num_splits) {
  const char* op = "fp8_gemm";
  const auto o = wq_operands<Fp8Host>(op, x, w8, scale, bias, nullptr, nullptr,
                                      c10::nullopt);
  const long S = wqg_check_splits(op, o, WQG_BA, num_splits);
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)((o.N + WQG_BA - 1) / WQG_BA),
                  (unsigned)((o.M + WQG_BM - 1) / WQG_BM), (unsigned)S);
  return wq_run(
      x, o, S,
      [&](short* y, float* part) {
        FP16_SWITCH(o.fp16, {
          hipLaunchKernelGGL((fp8_gemm_kernel<kFP16>), grid, dim3(256), 0,
                             stream, o.x, o.w[0], (const float*)o.s[0],
                             o.b[0], y, part, (int)o.M, (int)o.N, (int)o.K);
        });
      },
      [&](float* part, short* y, dim3 cgrid) {
        FP16_SWITCH(o.fp16, {
          hipLaunchKernelGGL((fp8_linear_combine_kernel<kFP16>), cgrid,
                             dim3(256), 0, stream, part, (const float*)o.s[0],
                             o.b[0], y, (int)o.M, (int)o.N, (int)S);
        });
      });
}

// The (W, NT) instance of the one-launch kernel for an [N, K] weight (SWIGLU:
// N = I, a gate/up pair) on a device with num_cus compute units. A function
// of (N, K, num_cus) only, never of M. Set by the sweep in
// profiles/r17_fp8_one_launch.md: PLAIN takes 4 waves on two tiles (which
// share one x fragment) once every CU gets a workgroup that way, and below
// that 8 waves on one tile; 8 x 2 was never the fastest. SWIGLU (always two
// tiles, 16 channels) takes 4 waves where that gives FP8W_WAVES_PER_CU waves
// per CU, otherwise 8. W = 8 needs 8 steps in K, so that every wave keeps a
// whole one.
constexpr long FP8W_WAVES_PER_CU = 4 * FP8L_WG_PER_CU;

std::vector<long> fp8_wide_instance(long n, long k, long num_cus,
                                    bool swiglu) {
  const long steps = (k + FP8L_STEP - 1) / FP8L_STEP;
  const long wg16 = (n + 15) / 16, wg32 = (n + 31) / 32;
  const long w8 = steps >= 8 ? 8 : 4;
  if (swiglu) return {wg16 * 4 >= FP8W_WAVES_PER_CU * num_cus ? 4 : w8, 2};
  if (wg32 >= num_cus) return {4, 2};
  return {w8, 1};
}

namespace {

// The one-launch front end: PLAIN when w1 is absent, SWIGLU otherwise.
torch::Tensor fp8_wide(const char* op, const torch::Tensor& x,
                       const torch::Tensor& w0, const torch::Tensor& s0,
                       const c10::optional<torch::Tensor>& b0,
                       const torch::Tensor* w1, const torch::Tensor* s1,
                       const c10::optional<torch::Tensor>& b1, long waves,
                       long tiles) {
  const auto o = wq_operands<Fp8Host>(op, x, w0, s0, b0, w1, s1, b1);
  wq_check_skinny_size(op, o, false);
  const auto inst = fp8_wide_instance(
      o.N, o.K, at::cuda::getCurrentDeviceProperties()->multiProcessorCount,
      o.swiglu);
  const long W = waves > 0 ? waves : inst[0];
  const long NT = o.swiglu ? 2 : (tiles > 0 ? tiles : inst[1]);
  TORCH_CHECK((W == 4 || W == 8) && (NT == 1 || NT == 2),
              op, ": instances are waves in {4, 8}, tiles in {1, 2}");
  return fp8_skinny(x, o, W, NT, false, 1);
}

}  // namespace

// fp8_linear's formula for M <= 64 in one launch whatever (N, K). waves /
// tiles: 0 = fp8_wide_instance's choice, otherwise forced (benchmarks, tests).
torch::Tensor fp8_linear_wide(torch::Tensor x, torch::Tensor w8,
                              torch::Tensor scale,
                              c10::optional<torch::Tensor> bias, long waves,
                              long tiles) {
  return fp8_wide("fp8_linear_wide", x, w8, scale, bias, nullptr, nullptr,
                  c10::nullopt, waves, tiles);
}

// y[M,I] = silu((x @ dq(wg8)^T) * sg (+ bias_gate))
//          * ((x @ dq(wu8)^T) * su (+ bias_up)), M <= 64, one launch.
torch::Tensor fp8_swiglu_linear(torch::Tensor x, torch::Tensor wg8,
                                torch::Tensor sg, torch::Tensor wu8,
                                torch::Tensor su,
                                c10::optional<torch::Tensor> bias_gate,
                                c10::optional<torch::Tensor> bias_up,
                                long waves) {
  return fp8_wide("fp8_swiglu_linear", x, wg8, sg, bias_gate, &wu8, &su,
                  bias_up, waves, 0);
}
