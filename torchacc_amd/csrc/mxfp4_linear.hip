// Weight-only MXFP4 linear layers (W4A16):
//   y[M,N] = x[M,K] @ dequant(W4[N,K])^T (+ bias[N])
// The weight is in the OCP microscaling format: e2m1 elements
// (+-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), two per byte (element 2i in bits 0..3 of
// byte i, 2i+1 in bits 4..7), codes [N, K/2] row-major, and one e8m0 scale
// byte per 32 elements along K, scales [N, K/32]: group g of row n is
// multiplied by 2^(scales[n,g] - 127). A quarter of the 16-bit bytes and half
// of the e4m3 ones that fp8_linear.hip streams. Operand order, kernel frames,
// batch invariance and tail rules are in wq_gemm_common.h; this file holds the
// format.
//
// Skinny weight stream (v_mfma_f32_16x16x32: lane l holds channel l&15,
// k-slots 8*(l>>4)..+7): a lane's 16-byte load is 32 codes of its row, which
// is exactly one scale group. The four lane groups of a row cover 64
// contiguous bytes, and a wave step issues the two loads of a 128-byte line
// back to back: 256 codes per row and step. Dword s of the load feeds MFMA
// K-step s (4 per load) through v_cvt_scalef32_pk_{bf16,f16}_fp4, one
// instruction per byte (two elements) with the group's scale applied: 16
// converts per load. The product element * 2^e is exact in the 16-bit type
// (see the range note below), so the conversion rounds nothing. The reduction
// order inside K is free, so the x fragment follows the same permutation: lane
// (j, g) reads x[j][k0 + 32g + 8s .. +7] for K-step s, 64 contiguous bytes per
// load.
//
// Group scales: the 8 scale bytes of a row's step are contiguous
// (scales[row][8t .. 8t+7]); a lane fetches them with one 8-byte load (rows
// start at any byte when K/32 is no multiple of 8, so the load is declared
// unaligned) and selects byte 4h + g for half h. The f32 scale is
// bitcast(max(e, 1) << 23): e = 0 would be 2^-127, an fp32 subnormal, and is
// CLAMPED to 2^-126. The quantiser never produces byte 0, and 255 (NaN) is
// rejected there.
//
// Exactness range: element * 2^e is a bf16 value for every scale byte 1..252
// (exponents -126..125; results below 2^-126 are bf16 subnormals). In fp16 it
// holds for exponents -14..12 (bytes 113..139) only; the fp16 contract is
// limited to that range.
//
// mxfp4_linear / mxfp4_swiglu_linear: one launch for every (N, K), M <= 64; K
// is cut only across the W in {4, 8} waves of a workgroup. Against the fp8
// kernel the weight bytes per MFMA halve while the x bytes stay, so a wave
// owns NT in {1, 2, 4} channel tiles per x fragment (an A fragment costs 4
// VGPRs per 32 codes). The x fragments of one half (MT x 4 x 16 bytes) are
// loaded per half, not per step, which keeps MT = 4 at 64 VGPRs of x. Built
// instances (W, NT): (4,1) (8,1) (4,2) (8,2) (4,4); (8,4) would need 128 KiB
// of reduction LDS at MT = 4 and is left out. The ragged step (K % 256 != 0,
// whole 32-code groups) reads its scale bytes one by one, predicated.
//
// mxfp4_dequantize writes the [N, K] 16-bit weight with the same convert
// (16-byte loads and stores); it serves checkpoint export. The tiled
// mxfp4_gemm kernel (second half of this file) serves M > 64.
#include <vector>

#include "wq_gemm_common.h"

// packed fp32 VALU forms are kept out of this file's device code
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

constexpr int MX4_STEP = 256;        // codes per wave step: one 128-byte line/row
constexpr int MX4_GROUP = 32;        // codes per scale byte

// the 8 scale bytes of a row's step; rows start at any byte
typedef unsigned mx4_u32x2_u __attribute__((ext_vector_type(2), aligned(1)));

// f32 2^(e - 127) from an e8m0 byte; e = 0 (an fp32 subnormal) clamps to 2^-126
DEVINLINE float mx4_scale(unsigned e) {
  return __builtin_bit_cast(float, max(e, 1u) << 23);
}

// 8 e2m1 codes (one dword) times the group scale -> one 16-bit x8 A fragment;
// byte i holds elements 2i (low nibble) and 2i+1
template <bool FP16>
DEVINLINE attn_u32x4 mx4_cvt8(unsigned c, float sc) {
  attn_u32x4 a;
  if constexpr (FP16) {
    a[0] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0));
    a[1] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1));
    a[2] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2));
    a[3] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3));
  } else {
    a[0] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0));
    a[1] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1));
    a[2] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2));
    a[3] = __builtin_bit_cast(
        unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3));
  }
  return a;
}

// One 256-code step t of a wave. Lane (j, g), half h: codes
// [256t + 128h + 32g, +32) of its row of every tile, i.e. 16 bytes at
// 128t + 64h + 16g, and scale byte 8t + 4h + g. Both halves' codes and the
// step's scale bytes are requested first; per half the lane then loads its 32
// activations of every column block and runs 4 K-steps x NT x MT MFMAs.
// TAIL is the one ragged step at the end of K (K % 256 != 0): groups at or
// past K contribute zeros (codes and activations both zeroed).
template <bool FP16, int MT, bool TAIL, int NT>
DEVINLINE void mx4_step(const unsigned char* const (&wrow)[NT],
                        const unsigned char* const (&srow)[NT],
                        const short* const (&xrow)[MT], int t, int g, int K,
                        f32x4 (&acc)[NT][MT]) {
  attn_u32x4 wv[2][NT];
  float sc[2][NT];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = t * MX4_STEP + h * 128 + g * MX4_GROUP;
    const bool live = !TAIL || k < K;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      wv[h][nt] = attn_u32x4{0u, 0u, 0u, 0u};
      if (live)
        wv[h][nt] = *reinterpret_cast<const attn_u32x4*>(wrow[nt] + (k >> 1));
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if constexpr (TAIL) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int gi = t * 8 + h * 4 + g;
        sc[h][nt] = mx4_scale(gi * MX4_GROUP < K ? srow[nt][gi] : 127u);
      }
    } else {
      const mx4_u32x2_u sv =
          *reinterpret_cast<const mx4_u32x2_u*>(srow[nt] + t * 8);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        sc[h][nt] = mx4_scale((sv[h] >> (8 * g)) & 0xFFu);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = t * MX4_STEP + h * 128 + g * MX4_GROUP;
    const bool live = !TAIL || k < K;
    attn_u32x4 xv[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        xv[mt][s] = attn_u32x4{0u, 0u, 0u, 0u};
        if (live)
          xv[mt][s] =
              *reinterpret_cast<const attn_u32x4*>(xrow[mt] + k + 8 * s);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const attn_u32x4 a = mx4_cvt8<FP16>(wv[h][nt][s], sc[h][nt]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[nt][mt] = wq_mfma16<FP16>(a, xv[mt][s], acc[nt][mt]);
      }
    }
  }
}

// wq_skinny_kernel's format: a code and a scale-row pointer per tile
struct Mx4Fmt {
  static constexpr int STEP = MX4_STEP;
  template <int NT>
  struct Rows {
    const unsigned char* w[NT];
    const unsigned char* s[NT];
    DEVINLINE void set(int nt, const unsigned char* wp,
                       const unsigned char* sp, long row, int K) {
      w[nt] = wp + row * (K / 2);
      s[nt] = sp + row * (K / MX4_GROUP);
    }
  };
  template <bool FP16, int MT, bool TAIL, int NT>
  static DEVINLINE void step(const Rows<NT>& rows,
                             const short* const (&xrow)[MT], int t, int g,
                             int K, f32x4 (&acc)[NT][MT]) {
    mx4_step<FP16, MT, TAIL>(rows.w, rows.s, xrow, t, g, K, acc);
  }
};

// A thread converts one scale group: 16 bytes of codes in, 64 bytes out.
template <bool FP16>
__global__ __launch_bounds__(256)
void mxfp4_dequantize_kernel(const unsigned char* __restrict__ codes,
                             const unsigned char* __restrict__ scales,
                             short* __restrict__ out, long groups) {
  const long gi = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= groups) return;
  const attn_u32x4 c = *reinterpret_cast<const attn_u32x4*>(codes + gi * 16);
  const float sc = mx4_scale(scales[gi]);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    *reinterpret_cast<attn_u32x4*>(out + gi * MX4_GROUP + 8 * s) =
        mx4_cvt8<FP16>(c[s], sc);
}

// ---------------------------------------------------------------------------
// mxfp4_gemm: the tiled kernel of wq_gemm_common.h with the codes kept PACKED
// in LDS and converted after the fragment read. BK = 64 codes is two scale
// groups per stage.
//
// LDS, per stage 20 KiB, MX4G_STAGES = 3 of them (60 KiB, two workgroups per
// CU); both images are filled global -> LDS directly (attn_glds16, five per
// thread and stage), with the swizzles on the source address:
//   x      the shared image. The fragment of K-step s is chunk 4*hi + s of
//          row l&31 (hi = l>>5): the reduction order inside a stage follows
//          the weight side, as in the skinny kernel.
//   codes  [128 rows][32 bytes]: 256 slots of 16 bytes, one per thread; a
//          slot is 32 codes, one scale group. Group `half` of row r sits in
//          slot 2r + (half ^ ((r>>3)&1)). A lane's A fragment for the WHOLE
//          stage is one ds_read_b128 of slot (row l&31, half hi); its 16-lane
//          groups are rows 16n..16n+15 of one half, and the XOR sends rows
//          8..15 to the other slot parity: 16 distinct slots of the 256-byte
//          bank line (unswizzled, 2r + hi has 8 distinct values mod 16, a
//          2-way conflict). Dword s of the slot feeds K-step s through
//          mx4_cvt8 (exact): 2 reads and 32 converts per lane under 16 MFMAs;
//          a code is converted once per wave, twice per workgroup.
//   scales a lane needs scales[row][2t + hi] of its two channel tiles: two
//          byte loads per stage, issued a stage ahead into registers (rows
//          start at any byte). No LDS image: the bytes are per lane already,
//          and an image would add a sixth direct load whose 128 live bytes
//          use an eighth of a wave instruction.
// Pipeline: the direct loads of step t+2 are issued after the barrier of step
// t, which also retires every read of the buffer they overwrite (step t-1's).
// Loads complete in order, so waiting until at most the MX4G_LOADS loads of
// step t+1 are outstanding (vmcnt) publishes step t; one barrier per stage.
//
// SWIGLU: two code and two scale pointers, nothing re-laid. A workgroup's 128
// A rows are 64 gate channels and the same 64 up channels; a wave's tile
// i = 0 is gate and i = 1 up for the SAME 32 channels, so
// silu(g (+ bg)) * (u (+ bu)) is formed in-lane in fp32, g and u never reach
// memory and x is staged once for both. grid.x = ceil(I / 64).
//
// The ragged step (K % 64 == 32): both code slots of a row are filled from
// its group 0 (no load leaves the tensor), and lanes of half 1 zero their
// fragment and read scale 1.
// -DMX4G_STAGES=2 builds the two-stage variant timed in
// profiles/r20_mxfp4_gemm.md
#ifndef MX4G_STAGES
#define MX4G_STAGES 3
#endif
constexpr int MX4G_W_B = WQG_BA * WQG_BK / 2;      // packed code image
constexpr int MX4G_STAGE_B = WQG_X_B + MX4G_W_B;
constexpr int MX4G_LOADS = 5;     // direct loads per thread and full stage
static_assert(MX4G_STAGES == 2 || MX4G_STAGES == 3, "two or three stages");
static_assert(MX4G_STAGES * MX4G_STAGE_B <= 64 * 1024, "LDS");

// byte offset of scale group `half` (0..1) of row `row` in the code image
DEVINLINE constexpr unsigned mx4g_woff(int row, int half) {
  return (unsigned)((2 * row + (half ^ ((row >> 3) & 1))) << 4);
}

// grid = (ceil(N / BN), ceil(M / 128), S), BN = 128 (PLAIN) or 64 (SWIGLU);
// block = 256. PLAIN reads (w0, s0, b0) only. S == 1: writes y. S > 1: writes
// raw fp32 sums to part[S][M][N] (SWIGLU: part[S][2][M][N], gate then up).
template <bool FP16, bool SWIGLU>
__global__ __launch_bounds__(256, 2)
void mxfp4_gemm_kernel(const short* __restrict__ x,
                       const unsigned char* __restrict__ w0,
                       const unsigned char* __restrict__ w1,
                       const unsigned char* __restrict__ s0,
                       const unsigned char* __restrict__ s1,
                       const short* __restrict__ b0,
                       const short* __restrict__ b1,
                       short* __restrict__ y, float* __restrict__ part,
                       int M, int N, int K) {
  constexpr int NS = MX4G_STAGES;
  constexpr int BN = SWIGLU ? WQG_BA / 2 : WQG_BA;
  __shared__ __attribute__((aligned(16))) char lds[NS * MX4G_STAGE_B];
  const int tid = threadIdx.x, lane = tid % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int wn = wave & 1, wm = wave >> 1;
  const int l31 = lane & 31, hi = lane >> 5;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * WQG_BM;
  const int split = blockIdx.z, S = gridDim.z;
  const int G = K / MX4_GROUP;    // scale bytes per row

  // contiguous, balanced runs of BK steps over the splits; the host keeps
  // S <= max(1, K / BK), so every split owns at least one step
  const int T = (K + WQG_BK - 1) / WQG_BK, Tfull = K / WQG_BK;
  const int t0 = (int)((long)split * T / S);
  const int t1 = (int)((long)(split + 1) * T / S);
  // steps below tq have a full successor NS - 2 steps on
  const int tq = min(t1, Tfull) - (NS - 2);

  // A row r of the workgroup: PLAIN channel n0 + r of w0. SWIGLU: wave half
  // r>>6, tile (r>>5)&1 = gate / up, channel n0 + 32 * (r>>6) + (r&31).
  auto a_chan = [&](int r) {
    return min(SWIGLU ? n0 + (r >> 6) * 32 + (r & 31) : n0 + r, N - 1);
  };

  // x staging: pass i fills slots i*256 + tid of the image, slot s = row
  // s>>3, stored chunk s&7, which holds logical chunk (s&7) ^ ((row>>1)&7);
  // the row's bits 1..3 are tid's bits 4..6 in every pass
  const int xc = (tid & 7) ^ ((tid >> 4) & 7);
  const short* xsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    xsrc[i] = x + (long)min(m0 + i * 32 + (tid >> 3), M - 1) * K + xc * 8;
  // code staging: thread tid fills slot tid = 2 * row + stored parity, which
  // holds group parity ^ ((row>>3)&1); the row's bit 3 is tid's bit 4
  const int wr = tid >> 1;
  const int wh = (tid & 1) ^ ((tid >> 4) & 1);
  const unsigned char* wsrc =
      (SWIGLU && ((wr >> 5) & 1) ? w1 : w0) + (long)a_chan(wr) * (K / 2);
  // scale rows of the lane's two channel tiles
  const unsigned char* srow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    srow[i] = (SWIGLU && i ? s1 : s0) +
              (long)a_chan(wn * 64 + i * 32 + l31) * G;

  // the lane's scale bytes of step t; groups at or past K read as 1.0
  auto load_scales = [&](int t, unsigned (&e)[2]) {
    const int gi = 2 * t + hi;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      e[i] = 127u;
      if (gi < G) e[i] = srow[i][gi];
    }
  };
  // issue the loads of step t into buffer `buf`
  auto stage_load = [&](int t, int buf) {
    const int k0 = t * WQG_BK;
    char* xi = lds + buf * MX4G_STAGE_B;
    char* wi = xi + WQG_X_B + wave * WAVE * 16;
    if (t < Tfull) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        attn_glds16(xsrc[i] + k0, xi + (i * 256 + wave * WAVE) * 16);
      attn_glds16(wsrc + (k0 >> 1) + wh * 16, wi);
    } else {
      const bool live = k0 + xc * 8 < K;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        attn_u32x4 v = attn_u32x4{0u, 0u, 0u, 0u};
        if (live) v = *reinterpret_cast<const attn_u32x4*>(xsrc[i] + k0);
        *reinterpret_cast<attn_u32x4*>(xi + (i * 256 + tid) * 16) = v;
      }
      // group 1 lies past the row: both slots take group 0
      attn_glds16(wsrc + (k0 >> 1), wi);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // en: the scale bytes of the next step, requested at the top of a step and
  // converted at its end; sc: the current step's scales
  unsigned en[2];
  load_scales(t0, en);
  float sc[2] = {mx4_scale(en[0]), mx4_scale(en[1])};
#pragma unroll
  for (int d = 0; d < NS - 1; ++d)
    if (t0 + d < t1) stage_load(t0 + d, d);

  // fragment reads: x row 32j + l31 of the wave's half, chunk 4hi + s; code
  // slot (row 32i + l31 of the wave's half, group hi)
  const unsigned sw = (unsigned)((l31 >> 1) & 7);
  const unsigned xrow_off = (unsigned)((wm * 64 + l31) * 128);
  const unsigned wslot_off =
      (unsigned)WQG_X_B + mx4g_woff(wn * 64 + l31, hi);

  int cur = 0;
  for (int t = t0; t < t1; ++t) {
    // publishes step t; retires the reads of step t-1's buffer
    if (NS > 2 && t < tq) wqg_publish<(NS - 2) * MX4G_LOADS>();
    else wqg_publish<0>();
    if (t + 1 < t1) load_scales(t + 1, en);
    if (t + NS - 1 < t1) {
      const int nb = cur + NS - 1;
      stage_load(t + NS - 1, nb >= NS ? nb - NS : nb);
    }
    const char* base = lds + cur * MX4G_STAGE_B;
    attn_u32x4 wf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      wf[i] = *reinterpret_cast<const attn_u32x4*>(
          base + wslot_off + i * (32 * 32));
      if (2 * t + hi >= G) wf[i] = attn_u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const unsigned ch = (((unsigned)(4 * hi + s)) ^ sw) << 4;
      attn_u32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = mx4_cvt8<FP16>(wf[i][s], sc[i]);
        b[i] = *reinterpret_cast<const attn_u32x4*>(
            base + xrow_off + i * (32 * 128) + ch);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = wq_mfma32<FP16>(a[i], b[j], acc[i][j]);
    }
    sc[0] = mx4_scale(en[0]);
    sc[1] = mx4_scale(en[1]);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }

  // lane: x row m of tile j; registers 4q..4q+3 of tile i: channels n..n+3.
  // SWIGLU: tile 0 is gate and tile 1 up of the same channels.
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm * 64 + j * 32 + l31;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < (SWIGLU ? 1 : 2); ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * (BN / 2) + i * 32 + 8 * q + 4 * hi;
        if (n >= N) continue;
        f32x4 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ti = SWIGLU ? h : i;
          v[h] = f32x4{acc[ti][j][4 * q], acc[ti][j][4 * q + 1],
                       acc[ti][j][4 * q + 2], acc[ti][j][4 * q + 3]};
        }
        if (S == 1) {
          wq_finish4<FP16, SWIGLU>(v[0], v[1], m, n, N, b0, b1, y);
          continue;
        }
#pragma unroll
        for (int h = 0; h < (SWIGLU ? 2 : 1); ++h) {
          float* p = part +
                     (((long)split * (SWIGLU ? 2 : 1) + h) * M + m) * N + n;
          if ((N & 3) == 0) {
            *reinterpret_cast<f32x4*>(p) = v[h];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (n + r < N) p[r] = v[h][r];
          }
        }
      }
    }
  }
}

}  // namespace

#pragma clang attribute pop

// The (W, NT) instance for an [N, K] weight (SWIGLU: N = I, a gate/up pair,
// NT counts gate and up tiles together) on a device with num_cus compute
// units. A function of (N, K, num_cus) only, never of M. PLAIN takes the
// widest tile count that still gives every CU a workgroup, since one x
// fragment then feeds the most weight bytes; below that, one channel tile on 8
// waves (which needs 8 steps in K, so that every wave keeps a whole one).
// SWIGLU takes four tiles only from two workgroups per CU on: at 1.3 per CU
// (I = 11008 on 256 CUs) the second, partial round of workgroups cost more at
// M <= 16 than the shared x fragment saved (profiles/r19_mxfp4_linear.md).
std::vector<long> mxfp4_linear_instance(long n, long k, long num_cus,
                                        bool swiglu) {
  const long steps = (k + MX4_STEP - 1) / MX4_STEP;
  const long w8 = steps >= 8 ? 8 : 4;
  const long wg16 = (n + 15) / 16, wg32 = (n + 31) / 32, wg64 = (n + 63) / 64;
  if (swiglu) {
    if (wg32 >= 2 * num_cus) return {4, 4};
    return {wg16 >= 2 * num_cus ? 4 : w8, 2};
  }
  if (wg64 >= num_cus) return {4, 4};
  if (wg32 >= num_cus) return {4, 2};
  return {w8, 1};
}

namespace {

// the per-format part of wq_operands: codes [N,K/2] and scales [N,K/32] uint8
struct Mx4Host {
  static constexpr long K_MULT = MX4_GROUP;
  static void check(const char* op, long K, const torch::Tensor& codes,
                    const torch::Tensor& scales) {
    TORCH_CHECK(scales.dim() == 2 && codes.scalar_type() == torch::kByte &&
                    scales.scalar_type() == torch::kByte,
                op, ": codes [N,K/2] uint8, scales [N,K/32] uint8");
    TORCH_CHECK(codes.size(1) * 2 == K && scales.size(1) * MX4_GROUP == K &&
                    scales.size(0) == codes.size(0),
                op, ": shape mismatch");
  }
};

// The one-launch front end: PLAIN when c1 is absent, SWIGLU otherwise.
torch::Tensor mx4_launch(const char* op, const torch::Tensor& x,
                         const torch::Tensor& c0, const torch::Tensor& s0,
                         const c10::optional<torch::Tensor>& b0,
                         const torch::Tensor* c1, const torch::Tensor* s1,
                         const c10::optional<torch::Tensor>& b1, long waves,
                         long tiles) {
  const auto o = wq_operands<Mx4Host>(op, x, c0, s0, b0, c1, s1, b1);
  wq_check_skinny_size(op, o, false);
  const auto inst = mxfp4_linear_instance(
      o.N, o.K, at::cuda::getCurrentDeviceProperties()->multiProcessorCount,
      o.swiglu);
  const long W = waves > 0 ? waves : inst[0];
  const long NT = tiles > 0 ? tiles : inst[1];
  TORCH_CHECK((W == 4 || W == 8) && (NT == 1 || NT == 2 || NT == 4) &&
                  !(W == 8 && NT == 4) && !(o.swiglu && NT == 1),
              op, ": instances are (waves, tiles) in (4,1) (8,1) (4,2) (8,2) "
                  "(4,4); SWIGLU counts gate and up tiles, so 2 or 4");

  auto stream = at::hip::getCurrentHIPStream();
  const long bn = o.swiglu ? 8 * NT : 16 * NT;
  const dim3 grid((unsigned)((o.N + bn - 1) / bn)), block((unsigned)(W * WAVE));
  const int mt = wq_skinny_mt(o.M);
#define MX4_LAUNCH(MTV, WV, NTV, SW)                                          \
  hipLaunchKernelGGL(                                                         \
      (wq_skinny_kernel<Mx4Fmt, kFP16, MTV, WV, NTV, SW>), grid, block, 0,    \
      stream, o.x, o.w[0], o.w[1], (const unsigned char*)o.s[0],              \
      (const unsigned char*)o.s[1], o.b[0], o.b[1], y, (int)o.M, (int)o.N,    \
      (int)o.K)
#define MX4_INSTANCE(MTV)                                   \
  do {                                                      \
    if (o.swiglu) {                                         \
      if (NT == 4) MX4_LAUNCH(MTV, 4, 4, true);             \
      else if (W == 4) MX4_LAUNCH(MTV, 4, 2, true);         \
      else MX4_LAUNCH(MTV, 8, 2, true);                     \
    } else if (NT == 4) {                                   \
      MX4_LAUNCH(MTV, 4, 4, false);                         \
    } else if (NT == 2) {                                   \
      if (W == 4) MX4_LAUNCH(MTV, 4, 2, false);             \
      else MX4_LAUNCH(MTV, 8, 2, false);                    \
    } else {                                                \
      if (W == 4) MX4_LAUNCH(MTV, 4, 1, false);             \
      else MX4_LAUNCH(MTV, 8, 1, false);                    \
    }                                                       \
  } while (0)
  return wq_run(
      x, o, 1,
      [&](short* y, float*) {
        FP16_SWITCH(o.fp16, {
          if (mt == 1) MX4_INSTANCE(1);
          else if (mt == 2) MX4_INSTANCE(2);
          else MX4_INSTANCE(4);
        });
      },
      [](float*, short*, dim3) {});
#undef MX4_INSTANCE
#undef MX4_LAUNCH
}

// The tiled front end: PLAIN when c1 is absent, SWIGLU otherwise.
torch::Tensor mx4g_launch(const char* op, const torch::Tensor& x,
                          const torch::Tensor& c0, const torch::Tensor& s0,
                          const c10::optional<torch::Tensor>& b0,
                          const torch::Tensor* c1, const torch::Tensor* s1,
                          const c10::optional<torch::Tensor>& b1,
                          long num_splits) {
  const auto o = wq_operands<Mx4Host>(op, x, c0, s0, b0, c1, s1, b1);
  const long bn = o.swiglu ? WQG_BA / 2 : WQG_BA;
  const long S = wqg_check_splits(op, o, bn, num_splits);
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)((o.N + bn - 1) / bn),
                  (unsigned)((o.M + WQG_BM - 1) / WQG_BM), (unsigned)S);
#define MX4G_LAUNCH(SW)                                                       \
  hipLaunchKernelGGL((mxfp4_gemm_kernel<kFP16, SW>), grid, dim3(256), 0,      \
                     stream, o.x, o.w[0], o.w[1],                             \
                     (const unsigned char*)o.s[0],                            \
                     (const unsigned char*)o.s[1], o.b[0], o.b[1], y, part,   \
                     (int)o.M, (int)o.N, (int)o.K)
#define MX4G_COMBINE(SW)                                                      \
  hipLaunchKernelGGL((wq_combine_kernel<kFP16, SW>), cgrid, dim3(256), 0,     \
                     stream, part, o.b[0], o.b[1], y, (int)o.M, (int)o.N,     \
                     (int)S)
  return wq_run(
      x, o, S,
      [&](short* y, float* part) {
        FP16_SWITCH(o.fp16, {
          if (o.swiglu) MX4G_LAUNCH(true);
          else MX4G_LAUNCH(false);
        });
      },
      [&](float* part, short* y, dim3 cgrid) {
        FP16_SWITCH(o.fp16, {
          if (o.swiglu) MX4G_COMBINE(true);
          else MX4G_COMBINE(false);
        });
      });
#undef MX4G_COMBINE
#undef MX4G_LAUNCH
}

}  // namespace

// y = x @ dequant(codes, scales)^T (+ bias), 1 <= M <= 64, one launch.
// waves / tiles: 0 = mxfp4_linear_instance's choice, otherwise forced
// (benchmarks, tests).
torch::Tensor mxfp4_linear(torch::Tensor x, torch::Tensor codes,
                           torch::Tensor scales,
                           c10::optional<torch::Tensor> bias, long waves,
                           long tiles) {
  return mx4_launch("mxfp4_linear", x, codes, scales, bias, nullptr, nullptr,
                    c10::nullopt, waves, tiles);
}

// y[M,I] = silu(x @ dq(gate)^T (+ bias_gate)) * (x @ dq(up)^T (+ bias_up)),
// M <= 64, one launch. tiles counts gate and up tiles of a wave: 2 or 4.
torch::Tensor mxfp4_swiglu_linear(torch::Tensor x, torch::Tensor gate_codes,
                                  torch::Tensor gate_scales,
                                  torch::Tensor up_codes,
                                  torch::Tensor up_scales,
                                  c10::optional<torch::Tensor> bias_gate,
                                  c10::optional<torch::Tensor> bias_up,
                                  long waves, long tiles) {
  return mx4_launch("mxfp4_swiglu_linear", x, gate_codes, gate_scales,
                    bias_gate, &up_codes, &up_scales, bias_up, waves, tiles);
}

// [N, K] weight in bf16 or fp16 from codes [N, K/2] and scales [N, K/32].
torch::Tensor mxfp4_dequantize(torch::Tensor codes, torch::Tensor scales,
                               torch::ScalarType dtype) {
  const bool fp16 = dtype == torch::kHalf;
  TORCH_CHECK(fp16 || dtype == torch::kBFloat16,
              "mxfp4_dequantize: dtype must be bf16 or fp16");
  TORCH_CHECK(codes.is_cuda() && scales.is_cuda() &&
                  codes.device() == scales.device(),
              "mxfp4_dequantize: GPU tensors on one device required");
  TORCH_CHECK(codes.dim() == 2 && scales.dim() == 2 &&
                  codes.scalar_type() == torch::kByte &&
                  scales.scalar_type() == torch::kByte &&
                  codes.is_contiguous() && scales.is_contiguous(),
              "mxfp4_dequantize: codes [N,K/2], scales [N,K/32], contiguous "
              "uint8");
  const long N = codes.size(0), K = codes.size(1) * 2;
  TORCH_CHECK(N >= 1 && K >= MX4_GROUP && K % MX4_GROUP == 0 &&
                  scales.size(0) == N && scales.size(1) * MX4_GROUP == K,
              "mxfp4_dequantize: K must be a positive multiple of 32 and the "
              "shapes must match");
  TORCH_CHECK((uintptr_t)codes.data_ptr() % 16 == 0,
              "mxfp4_dequantize: codes must be 16-byte aligned");
  auto out = torch::empty({N, K}, codes.options().dtype(dtype));
  const long groups = N * (K / MX4_GROUP);
  TORCH_CHECK((groups + 255) / 256 < (1L << 31),
              "mxfp4_dequantize: problem too large");
  auto stream = at::hip::getCurrentHIPStream();
  FP16_SWITCH(fp16, {
    hipLaunchKernelGGL((mxfp4_dequantize_kernel<kFP16>),
                       dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                       stream, (const unsigned char*)codes.data_ptr(),
                       (const unsigned char*)scales.data_ptr(),
                       (short*)out.data_ptr(), groups);
  });
  HIP_CHECK_LAST();
  return out;
}

// Number of K splits of mxfp4_gemm for an [M, K] x [N, K]^T problem on a
// device with num_cus compute units (wqg_splits on 128 x 128 tiles;
// mxfp4_swiglu_gemm applies it to its 128 x 64 tiles).
long mxfp4_gemm_num_splits(long m, long n, long k, long num_cus) {
  return wqg_splits(m, n, k, num_cus, WQG_BA);
}

// y = x @ dequant(codes, scales)^T (+ bias) for any M >= 1, on the tiled
// kernel. num_splits: 0 = chosen from (M, N, K) and the CU count, otherwise
// forced (benchmarks, tests). Bitwise repeatable; NOT batch-invariant, since
// the split depends on M.
torch::Tensor mxfp4_gemm(torch::Tensor x, torch::Tensor codes,
                         torch::Tensor scales,
                         c10::optional<torch::Tensor> bias, long num_splits) {
  return mx4g_launch("mxfp4_gemm", x, codes, scales, bias, nullptr, nullptr,
                     c10::nullopt, num_splits);
}

// y[M,I] = silu(x @ dq(gate)^T (+ bias_gate)) * (x @ dq(up)^T (+ bias_up)) for
// any M >= 1, one launch of the tiled kernel (plus the combine when K is
// split). Bitwise repeatable; NOT batch-invariant.
torch::Tensor mxfp4_swiglu_gemm(torch::Tensor x, torch::Tensor gate_codes,
                                torch::Tensor gate_scales,
                                torch::Tensor up_codes,
                                torch::Tensor up_scales,
                                c10::optional<torch::Tensor> bias_gate,
                                c10::optional<torch::Tensor> bias_up,
                                long num_splits) {
  return mx4g_launch("mxfp4_swiglu_gemm", x, gate_codes, gate_scales,
                     bias_gate, &up_codes, &up_scales, bias_up, num_splits);
}
