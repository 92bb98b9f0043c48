// What the weight-only quantised GEMMs (fp8_linear.hip: W8A16 e4m3,
// mxfp4_linear.hip: W4A16 MXFP4) share. Each file adds its format: how codes
// and scales are laid out, loaded and converted.
//
// Operands: x [M,K] and y [M,N] bf16 or fp16, fp32 accumulation; the weight
// [N,K] row-major in its format. The WEIGHTS are the MFMA A operand and the
// activation rows the B operand, so the result is y^T: a lane owns one x row
// and four consecutive channels, an 8-byte store along N (wq_finish4).
//
// Skinny kernel (M <= 64 rows per workgroup, wq_skinny_kernel): W waves on
// the same NT 16-channel tiles, each wave on its own contiguous, balanced run
// of K steps; the W accumulators are summed through LDS in wave order. W, NT,
// the split count and every K boundary come from (N, K, CU count) alone,
// never from M, and an output row depends on its own B column only: a row's
// bits depend neither on the batch it sits in nor on its position.
// Activations are read straight from global memory (they are L2-resident, and
// no two waves of a workgroup read the same x bytes).
//
// Tiled kernels (M > 64, one per format): 128 x rows by 128 A rows over
// BK = 64, 4 waves as 2 x 2, each on 2 x 2 tiles of the 32x32x16 MFMA. The x
// image's layout and the stage barrier are here; written as shared helpers the
// x staging and the epilogue loop moved both kernels' register allocation
// (profiles/r21_wq_gemm_refactor.md), so each kernel spells them out. K may
// be cut over S workgroups that write fp32 partials [S][M][N] (SWIGLU
// [S][2][M][N]), summed in split order by a combine kernel (wq_combine_kernel
// here for MXFP4). No atomics anywhere: results are bitwise repeatable. The
// tiled split depends on M, so only the skinny kernel is batch-invariant.
//
// Tails, everywhere: channels >= N read row N-1 and are predicated at the
// store; N % 4 != 0 takes scalar stores; rows >= M read row M-1 and are never
// stored; the one ragged K step is the last and contributes zeros past K.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "common.h"
#include "attn_common.h"

// packed fp32 VALU forms are kept out of this path's device code
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

typedef __bf16 wq_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wq_bf16x2 __attribute__((ext_vector_type(2)));

template <bool FP16>
DEVINLINE f32x4 wq_mfma16(attn_u32x4 a, attn_u32x4 b, f32x4 c) {
  if constexpr (FP16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        __builtin_bit_cast(attn_f16x8, a), __builtin_bit_cast(attn_f16x8, b),
        c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        __builtin_bit_cast(wq_bf16x8, a), __builtin_bit_cast(wq_bf16x8, b),
        c, 0, 0, 0);
  }
}

template <bool FP16>
DEVINLINE f32x16 wq_mfma32(attn_u32x4 a, attn_u32x4 b, f32x16 c) {
  if constexpr (FP16) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(
        __builtin_bit_cast(attn_f16x8, a), __builtin_bit_cast(attn_f16x8, b),
        c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(wq_bf16x8, a), __builtin_bit_cast(wq_bf16x8, b),
        c, 0, 0, 0);
  }
}

// Bias, convert and store channels n..n+3 (n % 4 == 0) of row m. SWIGLU:
// silu(v (+ b0)) * (u (+ b1)) in fp32.
template <bool FP16, bool SWIGLU>
DEVINLINE void wq_finish4(f32x4 v, f32x4 u, long m, int n, int N,
                          const short* __restrict__ b0,
                          const short* __restrict__ b1,
                          short* __restrict__ y) {
  const bool vec = (N & 3) == 0;  // then n + 3 < N, 8-byte aligned row start
  s16x4 ov;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = vec ? n + r : min(n + r, N - 1);
    float o = v[r];
    if (b0 != nullptr) o += AttnElem<FP16>::to_f32(b0[c]);
    if constexpr (SWIGLU) {
      float up = u[r];
      if (b1 != nullptr) up += AttnElem<FP16>::to_f32(b1[c]);
      // exp overflows to +inf for o < -88: the quotient is then -0, silu's
      // limit
      o = o / (1.f + __expf(-o)) * up;
    }
    ov[r] = AttnElem<FP16>::from_f32(o);
  }
  if (vec) {
    *reinterpret_cast<s16x4*>(y + m * N + n) = ov;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < N) y[m * N + n + r] = ov[r];
  }
}

// y = epilogue(sum over splits, in split order); a thread per four channels
// of one row. part is [S][M][N], SWIGLU [S][2][M][N] (gate, then up).
template <bool FP16, bool SWIGLU>
__global__ __launch_bounds__(256)
void wq_combine_kernel(const float* __restrict__ part,
                       const short* __restrict__ b0,
                       const short* __restrict__ b1,
                       short* __restrict__ y, int M, int N, int S) {
  constexpr int P = SWIGLU ? 2 : 1;
  const int n4 = (N + 3) / 4;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)M * n4) return;
  const long m = idx / n4;
  const int n = (int)(idx % n4) * 4;
  f32x4 v[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int h = 0; h < P; ++h) {
      const float* p = part + (((long)s * P + h) * M + m) * N + n;
      if ((N & 3) == 0) {
        v[h] += *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) v[h][r] += p[r];
      }
    }
  }
  wq_finish4<FP16, SWIGLU>(v[0], v[1], m, n, N, b0, b1, y);
}

// ---------------------------------------------------------------------------
// The skinny kernel. Fmt supplies: STEP (codes per wave step, one 128-byte
// line per row), Rows<NT> (per-tile row state) with set(nt, w, s, row, K), and
// step<FP16, MT, TAIL>(rows, xrow, t, g, K, acc).
//
// PLAIN: the wave's NT tiles are consecutive tiles of w0. SWIGLU: NT/2 tiles
// of the GATE weight w0 and the same NT/2 tiles of the UP weight w1 (two
// pointers, two scale pointers, nothing re-laid); one x fragment feeds both,
// and the two pre-activations stay fp32 in registers / LDS.
//
// grid.x = ceil(N / BN), BN = 16 * NT (PLAIN) or 8 * NT (SWIGLU); block =
// W * 64. LDS: red[W][NT * MT][64] f32x4, at most 64 KiB; after one barrier
// thread (i, l) sums slot (i, l) of waves 0..W-1 in that order and runs the
// epilogue for its 4 channels of one row.
template <class Fmt, bool FP16, int MT, int W, int NT, bool SWIGLU>
__global__ __launch_bounds__(W * WAVE)
void wq_skinny_kernel(const short* __restrict__ x,
                      const unsigned char* __restrict__ w0,
                      const unsigned char* __restrict__ w1,
                      const unsigned char* __restrict__ s0,
                      const unsigned char* __restrict__ s1,
                      const short* __restrict__ b0,
                      const short* __restrict__ b1,
                      short* __restrict__ y, int M, int N, int K) {
  static_assert(!SWIGLU || NT % 2 == 0, "SWIGLU: as many gate as up tiles");
  static_assert(W * NT * MT * WAVE * sizeof(f32x4) <= 64 * 1024, "LDS");
  constexpr int CT = SWIGLU ? NT / 2 : NT;   // channel tiles per workgroup
  constexpr int BN = 16 * CT;
  constexpr int STEP = Fmt::STEP;
  __shared__ f32x4 red[W][NT * MT][WAVE];
  const int tid = threadIdx.x, lane = tid % WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int j = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * BN;

  // contiguous, balanced runs of steps over the W waves
  const int T = (K + STEP - 1) / STEP, Tfull = K / STEP;
  const int t0 = (int)((long)wave * T / W);
  const int t1 = (int)((long)(wave + 1) * T / W);

  // tiles 0..CT-1 are w0's; SWIGLU: tiles CT..NT-1 are the same channels of w1
  typename Fmt::template Rows<NT> rows;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    rows.set(nt, nt < CT ? w0 : w1, nt < CT ? s0 : s1,
             (long)min(n0 + (nt % CT) * 16 + j, N - 1), K);
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
  for (int t = t0; t < tm; ++t)
    Fmt::template step<FP16, MT, false>(rows, xrow, t, g, K, acc);
  if (t1 > Tfull)  // only the last wave, only when K % STEP != 0
    Fmt::template step<FP16, MT, true>(rows, xrow, Tfull, g, K, acc);

#pragma unroll
  for (int i = 0; i < NT * MT; ++i) red[wave][i][lane] = acc[i / MT][i % MT];
  __syncthreads();
  // item (channel tile ct, column block mt, lane l) sums slot ct * MT + mt of
  // waves 0..W-1 in that order; SWIGLU also the up slot (CT + ct) * MT + mt
  constexpr int ITEMS = CT * MT * WAVE;
  for (int idx = tid; idx < ITEMS; idx += W * WAVE) {
    const int i = idx / WAVE, l = idx % WAVE;
    const int m = (i % MT) * 16 + (l & 15);
    const int n = n0 + (i / MT) * 16 + 4 * (l >> 4);
    if (m >= M || n >= N) continue;
    f32x4 v = red[0][i][l];
#pragma unroll
    for (int wv = 1; wv < W; ++wv) v += red[wv][i][l];
    f32x4 u = v;
    if constexpr (SWIGLU) {
      u = red[0][CT * MT + i][l];
#pragma unroll
      for (int wv = 1; wv < W; ++wv) u += red[wv][CT * MT + i][l];
    }
    wq_finish4<FP16, SWIGLU>(v, u, m, n, N, b0, b1, y);
  }
}

// ---------------------------------------------------------------------------
// Tiled kernels: the x side, the barrier and the epilogue loop.
constexpr int WQG_BM = 128;       // x rows per workgroup
constexpr int WQG_BA = 128;       // weight (A) rows per workgroup
constexpr int WQG_BK = 64;
constexpr int WQG_X_B = WQG_BM * WQG_BK * 2;    // the x image
constexpr int WQG_MAX_SPLITS = 16;
// BK steps a split keeps at least when S is chosen automatically: prologue,
// epilogue and the partials' traffic are paid per split
constexpr int WQG_MIN_STEPS = 4;

// The x image is [128 rows][64 x 16 bit] with 128-byte rows whose eight
// 16-byte chunks are XORed with (row>>1)&7: 16 consecutive lanes reading one
// logical chunk of rows 16n..16n+15 touch the 16 distinct 16-byte slots of the
// 256-byte bank line. Byte offset of chunk ch (0..7) of row `row`:
DEVINLINE constexpr unsigned wqg_xoff(int row, int ch) {
  return (unsigned)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4));
}

// Wait until at most `PENDING` of this wave's loads are outstanding (vmcnt;
// 0x0F70 waits for nothing else), then a workgroup barrier with its LDS
// fences written out: __syncthreads() is a call here, once per BK step.
template <int PENDING>
DEVINLINE void wqg_publish() {
  static_assert(PENDING >= 0 && PENDING < 16, "vmcnt's low field");
  __builtin_amdgcn_s_waitcnt(0x0F70 | PENDING);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace

#pragma clang attribute pop

// ---------------------------------------------------------------------------
// Host side.
namespace {

// K splits of a tiled kernel for row tiles of 128 and channel tiles of bn on
// a device with num_cus compute units: 1 once the tiles cover the CUs,
// otherwise as many as bring the workgroup count up to the CU count, while
// every split keeps at least WQG_MIN_STEPS whole BK steps (one, where K has
// fewer than that).
inline long wqg_splits(long m, long n, long k, long num_cus, long bn) {
  const long tiles = ((m + WQG_BM - 1) / WQG_BM) * ((n + bn - 1) / bn);
  const long steps = k / WQG_BK;   // whole steps
  const long want = num_cus / tiles;
  const long cap = std::min<long>(WQG_MAX_SPLITS, steps / WQG_MIN_STEPS);
  return std::max<long>(1, std::min(want, cap));
}

// The checked operands of one call: PLAIN when w1 is absent, SWIGLU otherwise.
struct WqOperands {
  bool fp16, swiglu;
  long M, N, K;
  const short* x;
  const unsigned char* w[2];
  const void* s[2];
  const short* b[2];
};

// One check for every op of the path. HostFmt supplies K_MULT and
// check(op, K, w, s): the types and shapes of a weight's code and scale
// tensors against K, and the scale's alignment where the kernels need it.
template <class HostFmt>
WqOperands wq_operands(const char* op, const torch::Tensor& x,
                       const torch::Tensor& w0, const torch::Tensor& s0,
                       const c10::optional<torch::Tensor>& b0,
                       const torch::Tensor* w1, const torch::Tensor* s1,
                       const c10::optional<torch::Tensor>& b1) {
  WqOperands o{};
  o.swiglu = w1 != nullptr;
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  (uintptr_t)x.data_ptr() % 16 == 0,
              op, ": x must be a contiguous, aligned [M,K] GPU tensor");
  o.fp16 = x.scalar_type() == torch::kHalf;
  TORCH_CHECK(o.fp16 || x.scalar_type() == torch::kBFloat16,
              op, ": x must be bf16 or fp16");
  o.M = x.size(0);
  o.K = x.size(1);
  TORCH_CHECK(o.M >= 1 && o.K >= HostFmt::K_MULT && o.K % HostFmt::K_MULT == 0,
              op, ": K must be a positive multiple of ", HostFmt::K_MULT);
  o.x = (const short*)x.data_ptr();
  const torch::Tensor* w[2] = {&w0, w1};
  const torch::Tensor* s[2] = {&s0, s1};
  const c10::optional<torch::Tensor>* b[2] = {&b0, &b1};
  for (int i = 0; i < (o.swiglu ? 2 : 1); ++i) {
    TORCH_CHECK(w[i]->is_cuda() && s[i]->is_cuda() &&
                    w[i]->device() == x.device() &&
                    s[i]->device() == x.device(),
                op, ": weights and scales on x's GPU required");
    TORCH_CHECK(w[i]->dim() == 2 && w[i]->is_contiguous() &&
                    s[i]->is_contiguous() &&
                    (uintptr_t)w[i]->data_ptr() % 16 == 0,
                op, ": weights [N,...] and scales contiguous, weights "
                    "16-byte aligned");
    HostFmt::check(op, o.K, *w[i], *s[i]);
    if (i == 0) o.N = w0.size(0);
    TORCH_CHECK(o.N >= 1, op, ": the weight has no rows");
    TORCH_CHECK(w[i]->size(0) == o.N, op, ": gate/up shape mismatch");
    o.w[i] = (const unsigned char*)w[i]->data_ptr();
    o.s[i] = s[i]->data_ptr();
    if (b[i]->has_value()) {
      const torch::Tensor& bt = **b[i];
      TORCH_CHECK(bt.is_cuda() && bt.device() == x.device() &&
                      bt.scalar_type() == x.scalar_type() && bt.dim() == 1 &&
                      bt.size(0) == o.N && bt.is_contiguous() &&
                      (uintptr_t)bt.data_ptr() % 8 == 0,
                  op, ": bias must be [N], contiguous, aligned, x's dtype");
      o.b[i] = (const short*)bt.data_ptr();
    }
  }
  return o;
}

// skinny ops: the kernels index rows and channels of one 64-row block in int
inline void wq_check_skinny_size(const char* op, const WqOperands& o,
                                 bool any_m) {
  TORCH_CHECK(any_m || o.M <= 64, op, ": 1 <= M <= 64");
  TORCH_CHECK((o.M + 63) / 64 <= 65535, op, ": too many 64-row blocks");
  TORCH_CHECK(o.M * o.K < (1L << 31) && 64 * o.K < (1L << 31) &&
                  (o.M + 64) * o.N < (1L << 31) && 128 * o.N < (1L << 31),
              op, ": problem too large");
}

// Tiled ops: the forced or chosen split count, capped so that every split
// keeps at least one whole BK step, after the size checks of the tiled grid.
inline long wqg_check_splits(const char* op, const WqOperands& o, long bn,
                             long num_splits) {
  TORCH_CHECK(o.M * o.K < (1L << 31) && (o.M + WQG_BM) * o.N < (1L << 31) &&
                  (o.M + WQG_BM - 1) / WQG_BM <= 65535,
              op, ": problem too large");
  long S = num_splits;
  if (S <= 0) {
    S = wqg_splits(
        o.M, o.N, o.K,
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount, bn);
  }
  TORCH_CHECK(S <= WQG_MAX_SPLITS, op, ": num_splits above ", WQG_MAX_SPLITS);
  return std::max<long>(1, std::min(S, o.K / WQG_BK));
}

// Allocate y (and the partials when S > 1), run `launch(y, part)` and, when
// S > 1, `combine(part, y, grid)`: the tail of every front end.
template <class Launch, class Combine>
torch::Tensor wq_run(const torch::Tensor& x, const WqOperands& o, long S,
                     Launch&& launch, Combine&& combine) {
  auto y = torch::empty({o.M, o.N}, x.options());
  torch::Tensor part;
  float* part_p = nullptr;
  if (S > 1) {
    part = torch::empty({S * (o.swiglu ? 2 : 1), o.M, o.N},
                        x.options().dtype(torch::kFloat));
    part_p = part.data_ptr<float>();
  }
  launch((short*)y.data_ptr(), part_p);
  HIP_CHECK_LAST();
  if (S > 1) {
    const long groups = o.M * ((o.N + 3) / 4);
    combine(part_p, (short*)y.data_ptr(),
            dim3((unsigned)((groups + 255) / 256)));
    HIP_CHECK_LAST();
  }
  return y;
}

// column blocks of 16 rows a skinny workgroup carries for M rows (<= 64)
inline int wq_skinny_mt(long m) { return m > 32 ? 4 : (m > 16 ? 2 : 1); }

}  // namespace
