// Multi-query attention over a KV cache (chunked prefill, speculative
// verification, mixed prefill/decode batches), forward only, gfx950.
//
// q [b, sq, hq, d] holds the LAST n_i <= sq tokens of sequence i, whose keys
// the caller has already written into the cache; L_i = k_lens[i] counts them.
// Query row j < n_i sits at position p = L_i - n_i + j and sees the keys
// [lo, p], lo = max(0, p - wl) with a left window, else 0. Rows with j >= n_i
// or p < 0 give a zero output row and lse = -inf. Both length tensors are
// read on the device.
//
// The body is fa_fwd_kernel's ladder (flash_attn_fwd.hip): swapped QK^T so a
// lane owns one score row, K row-major and V transposed in LDS with the same
// swizzles, 64-key tiles, register-staged stage_load / stage_write, double
// buffer, P rounded to 16 bits and redistributed with permlane32_swap. What
// differs:
//   - GQA packing. A workgroup serves one (sequence, kv head, row tile); the
//     MFMA row index runs over (query position, head within the group),
//     m = j * rep + r. Every K/V tile is therefore read once per kv head and
//     sq = 4..16 at rep = 4..8 already fills 32-row MFMA tiles. The lane's row
//     gives j = m / rep for the mask and h = kh * rep + m % rep for the Q
//     load and the O / LSE store.
//   - Row tile = 4 waves x 32 rows = 128 packed rows (256 threads). There is
//     no split over the keys, so the row tiles are the only parallelism
//     inside one (sequence, kv head): 128 rows give twice the workgroups of
//     fa_fwd's 256, and the staging registers of a 64-key tile (8 x 16 bytes
//     per thread at d = 128) still fit without scratch.
//   - Per-sequence alignment: shift = L - n is workgroup-uniform, read from
//     device memory. The tile range runs from the lowest lo to the highest p
//     of the workgroup's rows.
//   - Loads never touch an invisible slot. A staging row whose key lies
//     outside [kv_lo, kv_hi) (the union of the visible ranges of the
//     workgroup's rows, kv_hi <= L) re-reads the nearest key inside the range
//     (branch-free load) and is replaced by zero before it is written to LDS.
//     Slots at or past L, and slots below the window of the tile's first row,
//     are never read; what they hold (NaN included) cannot matter.
//   - PAGED: key -> table[i, key >> log2(page_size)], clamped into
//     [0, num_pages - 1], slot key & (page_size - 1). The entries of a tile
//     are fetched one tile before its K/V loads are issued. Only entries of
//     keys in [kv_lo, kv_hi) are read, so those of logical pages at or past
//     ceil(L / page_size) are never dereferenced. The tiles, the masks and
//     all arithmetic are the contiguous kernel's: the result is bitwise the
//     contiguous one on the gathered cache.
//   - FP8: the caches hold OCP e4m3fn codes; a thread stages 8 bytes per
//     chunk and converts them at stage_write (e4m3 is exact in bf16 and in
//     fp16). The Q fragments stay 16-bit MFMA operands, so k_scale[kh] is
//     folded into the factor that scales the scores; v_scale[kh] multiplies
//     the normalised row once in the epilogue. Both are read from device
//     memory.
// Plain vector stores only, no atomics, one fixed reduction order: the result
// is deterministic.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "common.h"
#include "attn_common.h"
#include "kvcache_common.h"

namespace {

constexpr int MQ_WAVES = 4;
constexpr int MQ_THREADS = MQ_WAVES * 64;
constexpr int MQ_ROWS = MQ_WAVES * 32;   // packed rows per workgroup
constexpr int MQ_KVB = 64;               // keys per tile

typedef float mq_f32x16 __attribute__((ext_vector_type(16)));

// two fp32 values that are exactly representable in the 16-bit type, packed
// (lo in the low half): bf16 keeps the upper 16 bits, fp16 converts
template <bool FP16>
DEVINLINE unsigned mq_pack_exact(float lo, float hi) {
  if constexpr (FP16) {
    return AttnElem<true>::cvt_pk(lo, hi);
  } else {
    return (__builtin_bit_cast(unsigned, lo) >> 16) |
           (__builtin_bit_cast(unsigned, hi) & 0xffff0000u);
  }
}

// 8 e4m3 codes -> 8 16-bit elements (exact)
template <bool FP16>
DEVINLINE s16x8 mq_cvt8_fp8(const u32x2& r) {
  float f[8];
  kvc_cvt8_fp8(r, f);
  s16x8 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned w = mq_pack_exact<FP16>(f[2 * i], f[2 * i + 1]);
    out[2 * i + 0] = (short)(w & 0xffffu);
    out[2 * i + 1] = (short)(w >> 16);
  }
  return out;
}

// In HIP the second launch-bounds argument is waves per SIMD: 2 gives a
// 256-VGPR budget (the 64 KB of LDS at d = 128 admit 2 workgroups per CU).
template <int D, bool FP16, bool PAGED, bool FP8>
__global__ __launch_bounds__(MQ_THREADS, 2)
void fa_kvcache_mq_kernel(const short* __restrict__ Q,
                          const void* __restrict__ Kp,
                          const void* __restrict__ Vp,
                          const int* __restrict__ k_lens,
                          const int* __restrict__ q_lens,
                          short* __restrict__ O, float* __restrict__ LSE,
                          int sq, int cap, int hq, int hk,
                          // contiguous: batch / sequence strides; PAGED:
                          // page / slot strides (elements of the cache)
                          long k_sb, long k_ss, long v_sb, long v_ss,
                          float scale, int wl,
                          const int* __restrict__ block_table,
                          int page_shift, int num_pages,
                          const float* __restrict__ k_scale,
                          const float* __restrict__ v_scale) {
  using ET = AttnElem<FP16>;
  using KE = typename std::conditional<FP8, unsigned char, short>::type;
  using KV8 = typename std::conditional<FP8, u32x2, s16x8>::type;
  constexpr int NT = D / 16;   // QK^T k-steps (d slices of 16)
  constexpr int NA = D / 32;   // PV output accs (d blocks of 32)
  constexpr int KVB = MQ_KVB;
  constexpr int KROW_BYTES = D * 2;
  constexpr int CPR = D / 8;                    // 8-element chunks per row
  constexpr int PER_THR = KVB * CPR / MQ_THREADS;
  constexpr int ROWS_PER_PASS = MQ_THREADS / CPR;

  // LDS: K [64][D] + V^T [D][64], double buffered
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* k_lds = reinterpret_cast<short*>(smem);                // 2*64*D
  short* vt_lds = reinterpret_cast<short*>(smem) + 2 * KVB * D; // 2*D*64

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;         // packed row within the wave / d col
  const int hi = lane >> 5;          // lane half

  const int rep = hq / hk;
  const int M = sq * rep;            // packed rows of one (sequence, kv head)
  const int kh = blockIdx.y;
  const int b = blockIdx.z;
  const int m0wg = blockIdx.x * MQ_ROWS;
  const int m0 = m0wg + wid * 32;    // this wave's first packed row
  const int mrow = m0 + col;         // this lane's packed row

  // ---- per-sequence alignment, from device memory ------------------------
  const int L = min(max(k_lens[b], 0), cap);
  int n = sq;
  if (q_lens != nullptr) n = min(max(q_lens[b], 0), sq);
  const int shift = L - n;

  const int jr = mrow / rep;                   // query position of the row
  const int h = kh * rep + (mrow - jr * rep);  // q head of the row
  const bool in_range = mrow < M;
  // position of the row; -1 for rows that see nothing (no key is <= -1)
  const int prow = (in_range && jr < n) ? max(shift + jr, -1) : -1;
  const int lorow = (wl >= 0) ? max(0, prow - wl) : 0;

  // ---- workgroup key range: union of the rows' visible ranges ------------
  const int jf_wg = m0wg / rep;
  const int jl_wg = min(n - 1, min(M - 1, m0wg + MQ_ROWS - 1) / rep);
  const int kv_hi = min(L, max(0, shift + jl_wg + 1));           // exclusive
  const int kv_lo = (wl >= 0) ? max(0, max(shift + jf_wg, 0) - wl) : 0;
  const int t0 = kv_lo / KVB;
  const int t1 = (kv_hi + KVB - 1) / KVB;                        // exclusive
  const int ntiles = (jf_wg < n && kv_hi > kv_lo) ? t1 - t0 : 0;

  // ---- this wave's rows ---------------------------------------------------
  const int jf_w = m0 / rep;
  const int jl_w = min(n - 1, min(M - 1, m0 + 31) / rep);
  const int phi_w = shift + jl_w;              // highest position
  const int plo_w = max(shift + jf_w, 0);      // lowest valid position
  const bool wave_any = (m0 < M) && (jf_w < n) && (phi_w >= 0);
  const bool wave_all = (m0 + 31 < M) && ((m0 + 31) / rep < n) &&
                        (shift + jf_w >= 0);

  // ---- Q fragments --------------------------------------------------------
  // B-frag for swapped QK^T: lane holds Q[row][t*16 + hi*8 + j], j=0..7
  bf16x8 qfrag[NT];
  {
    const long qbase = in_range ? ((long)(b * (long)sq + jr) * hq + h) * D : 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s16x8 v = in_range
          ? *reinterpret_cast<const s16x8*>(Q + qbase + t * 16 + hi * 8)
          : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) qfrag[t][j] = v[j];
    }
  }
  // fp8: the scores are those of the scaled keys
  float sc = scale;
  if constexpr (FP8) sc *= k_scale[kh];

  // ---- staging ------------------------------------------------------------
  const int srow = tid / CPR;                  // row of chunk i: srow + i*RPP
  const int d0 = (tid % CPR) * 8;
  const KE* kp = reinterpret_cast<const KE*>(Kp) +
                 (PAGED ? 0L : (long)b * k_sb) + (long)kh * D + d0;
  const KE* vp = reinterpret_cast<const KE*>(Vp) +
                 (PAGED ? 0L : (long)b * v_sb) + (long)kh * D + d0;
  const int* bt =
      PAGED ? block_table + (long)b * (cap >> page_shift) : nullptr;
  KV8 kreg[PER_THR], vreg[PER_THR];
  int pg[PER_THR];   // PAGED: clamped pages of the tile loaded next

  // the key a staging row reads: its own, or the nearest one in range
  auto src_key = [&](int tile, int i) {
    const int key = (t0 + tile) * KVB + srow + i * ROWS_PER_PASS;
    return min(max(key, kv_lo), kv_hi - 1);
  };

  auto load_pages = [&](int tile) {
#pragma unroll
    for (int i = 0; i < PER_THR; ++i)
      pg[i] = min(max(bt[src_key(tile, i) >> page_shift], 0), num_pages - 1);
  };

  auto stage_load = [&](int tile) {
#pragma unroll
    for (int i = 0; i < PER_THR; ++i) {
      const int key = src_key(tile, i);
      long ko, vo;
      if constexpr (PAGED) {
        const int in_page = key & ((1 << page_shift) - 1);
        ko = (long)pg[i] * k_sb + (long)in_page * k_ss;
        vo = (long)pg[i] * v_sb + (long)in_page * v_ss;
      } else {
        ko = (long)key * k_ss;
        vo = (long)key * v_ss;
      }
      kreg[i] = *reinterpret_cast<const KV8*>(kp + ko);
      vreg[i] = *reinterpret_cast<const KV8*>(vp + vo);
    }
  };

  auto stage_write = [&](int tile, int buf) {
    short* kdst = k_lds + buf * KVB * D;
    short* vdst = vt_lds + buf * KVB * D;
    const int kv0 = (t0 + tile) * KVB;
#pragma unroll
    for (int i = 0; i < PER_THR; ++i) {
      const int row = srow + i * ROWS_PER_PASS;
      const int key = kv0 + row;
      const bool live = (key >= kv_lo) && (key < kv_hi);
      s16x8 kk, vv;
      if constexpr (FP8) {
        kk = mq_cvt8_fp8<FP16>(kreg[i]);
        vv = mq_cvt8_fp8<FP16>(vreg[i]);
      } else {
        kk = kreg[i];
        vv = vreg[i];
      }
      if (!live) {
        kk = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        vv = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      // K: row-major with (row&7)<<4 byte-XOR swizzle
      {
        unsigned byte = row * KROW_BYTES + d0 * 2;
        byte ^= (unsigned)((row & 7) << 4);
        *reinterpret_cast<s16x8*>(
            reinterpret_cast<char*>(kdst) + byte) = kk;
      }
      // V^T: [D][64] with (d&7)<<4 swizzle, scalar scatter. d0 is a multiple
      // of 8, so the 8 elements of a chunk share the XOR term and differ by
      // a constant 128 bytes: one address per chunk, the rest are immediates
      {
        const unsigned base = (unsigned)d0 * (KVB * 2) +
                              ((unsigned)(row * 2) ^
                               (unsigned)(((d0 >> 3) & 7) << 4));
        char* vrow = reinterpret_cast<char*>(vdst) + base;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<short*>(vrow + j * (KVB * 2)) = vv[j];
      }
    }
  };

  // ---- online softmax state ----------------------------------------------
  float m_run = -INFINITY;
  float l_run = 0.f;
  mq_f32x16 oacc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) oacc[a] = mq_f32x16(0.f);

  if (ntiles > 0) {
    if constexpr (PAGED) load_pages(0);
    stage_load(0);
    if constexpr (PAGED) { if (ntiles > 1) load_pages(1); }
    stage_write(0, 0);
    if (ntiles > 1) {
      stage_load(1);   // in flight under tile 0's compute
      if constexpr (PAGED) { if (ntiles > 2) load_pages(2); }
    }
  }
  __syncthreads();

  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const int kv0 = (t0 + tile) * KVB;
    // wave-level skip: tile entirely outside this wave's causal/window span
    bool wave_active = wave_any && (kv0 <= phi_w);
    if (wl >= 0 && kv0 + KVB <= plo_w - wl) wave_active = false;

    if (wave_active) {
      const short* kbuf = k_lds + buf * KVB * D;
      const short* vbuf = vt_lds + buf * KVB * D;
      // ---- QK^T: 2 key sub-blocks x NT d-steps --------------------------
      mq_f32x16 p[2];
      p[0] = mq_f32x16(0.f);
      p[1] = mq_f32x16(0.f);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          // A-frag: K[key = kb*32 + col][d = t*16 + hi*8 + j]
          const int row = kb * 32 + col;
          unsigned byte = (unsigned)row * KROW_BYTES + (t * 16 + hi * 8) * 2;
          byte ^= (unsigned)((row & 7) << 4);
          bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const char*>(kbuf) + byte);
          p[kb] = ET::mfma(kf, qfrag[t], p[kb]);
        }
      }
      // ---- mask + scale --------------------------------------------------
      // "full" = no per-element masking for ANY row of this wave: every row
      // is valid, the tile ends at or below the smallest position and, with
      // a window, starts at or above the largest row's lower bound
      const bool tile_full = wave_all && (kv0 + KVB - 1 <= shift + jf_w) &&
                             (wl < 0 || kv0 >= phi_w - wl);
      float pmax = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s = p[kb][r] * sc;
          if (!tile_full) {
            const int key = kv0 + kb * 32 + CROW(r, hi);
            const bool valid = (key >= lorow) && (key <= prow);
            s = valid ? s : -INFINITY;
          }
          p[kb][r] = s;
          pmax = fmaxf(pmax, s);
        }
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));
      // ---- online rescale ------------------------------------------------
      const float m_new = fmaxf(m_run, pmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha =
          (m_run == -INFINITY) ? 0.f : __expf(m_run - m_use);
      m_run = m_new;
      float lsum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float e = __expf(p[kb][r] - m_use);  // -inf -> 0
          p[kb][r] = e;
          lsum += e;
        }
      }
      lsum += __shfl_xor(lsum, 32, 64);
      l_run = l_run * alpha + lsum;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[a][r] *= alpha;
      }
      // ---- P -> 16-bit B-fragments (cvt_pk + permlane32_swap) ------------
      // step (kb, tp): B-frag covering keys [kv0+kb*32+16*tp, +16)
      unsigned pb[4][4];  // [step][u32 slot]
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int tp = 0; tp < 2; ++tp)
          t12_pack_frag<ET>(p[kb], tp, pb[kb * 2 + tp]);
      }
      // ---- PV: OUT^T[d][row] += V^T x P ----------------------------------
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          // A-frag: V^T[d = a*32 + col][key = st*16 + hi*8 + j]
          const int d = a * 32 + col;
          unsigned byte = (unsigned)d * (KVB * 2) + (st * 16 + hi * 8) * 2;
          byte ^= (unsigned)(((d >> 3) & 7) << 4);
          bf16x8 vf = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const char*>(vbuf) + byte);
          bf16x8 pf = *reinterpret_cast<const bf16x8*>(&pb[st][0]);
          oacc[a] = ET::mfma(vf, pf, oacc[a]);
        }
      }
    }

    if (tile + 1 < ntiles) {
      // write tile+1 (loaded one iteration ago) into the other buffer --
      // safe: buf^1 was last read during tile-1, behind a barrier
      stage_write(tile + 1, buf ^ 1);
      if (tile + 2 < ntiles) {
        stage_load(tile + 2);
        if constexpr (PAGED) { if (tile + 3 < ntiles) load_pages(tile + 3); }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: every row m < M is written -------------------------------
  if (in_range) {
    float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
    if constexpr (FP8) inv_l *= v_scale[kh];   // once per normalised row
    short* op = O + ((long)(b * (long)sq + jr) * hq + h) * D;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // registers 4g..4g+3 are d = a*32 + 8g + 4hi + 0..3: one 8-byte store
        s16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          w[e] = ET::from_f32(oacc[a][4 * g + e] * inv_l);
        *reinterpret_cast<s16x4*>(op + a * 32 + CROW(4 * g, hi)) = w;
      }
    }
    if (hi == 0) {
      LSE[((long)b * hq + h) * sq + jr] =
          (l_run > 0.f) ? m_run + __logf(l_run) : -INFINITY;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

template <int D, bool FP16, bool PAGED, bool FP8>
void mq_launch(const torch::Tensor& q, const torch::Tensor& k,
               const torch::Tensor& v, const int* klp, const int* qlp,
               torch::Tensor& o, torch::Tensor& lse, int cap, float scale,
               int wl, const int* bt, int page_shift, const float* k_scale,
               const float* v_scale, hipStream_t stream) {
  const int b = q.size(0), sq = q.size(1), hq = q.size(2);
  const int hk = k.size(2);
  const int rows = sq * (hq / hk);
  dim3 grid((rows + MQ_ROWS - 1) / MQ_ROWS, hk, b);
  const int lds = 4 * MQ_KVB * D * 2;  // K + V^T, double buffered
  hipLaunchKernelGGL((fa_kvcache_mq_kernel<D, FP16, PAGED, FP8>), grid,
                     dim3(MQ_THREADS), lds, stream,
                     (const short*)q.data_ptr(), (const void*)k.data_ptr(),
                     (const void*)v.data_ptr(), klp, qlp,
                     (short*)o.data_ptr(), lse.data_ptr<float>(), sq, cap,
                     hq, hk, (long)k.stride(0), (long)k.stride(1),
                     (long)v.stride(0), (long)v.stride(1), scale, wl, bt,
                     page_shift, PAGED ? (int)k.size(0) : 0, k_scale,
                     v_scale);
}

constexpr const char* MQ_OP = "fa_kvcache_mq";

// Shape-only checks, no host sync.
template <bool PAGED, bool FP8>
std::vector<torch::Tensor> mq_run(const torch::Tensor& q,
                                  const torch::Tensor& k_cache,
                                  const torch::Tensor& v_cache,
                                  const torch::Tensor& k_lens,
                                  const torch::Tensor& q_lens,
                                  const torch::Tensor& block_table,
                                  const torch::Tensor& k_scale,
                                  const torch::Tensor& v_scale,
                                  double softmax_scale, long wl) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.is_contiguous(),
              "fa_kvcache_mq: q must be a contiguous GPU [b, sq, hq, d]");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 ||
                  q.scalar_type() == torch::kHalf,
              "fa_kvcache_mq: bf16/fp16 only");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0);
  kvc_check_cache(MQ_OP, k_cache, q, "k_cache", FP8);
  kvc_check_cache(MQ_OP, v_cache, q, "v_cache", FP8);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "fa_kvcache_mq: k_cache and v_cache shapes differ");
  const long b = q.size(0), sq = q.size(1), hq = q.size(2), D = q.size(3);
  const long hk = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128,
              "fa_kvcache_mq: head_dim must be 64 or 128");
  TORCH_CHECK(hk > 0 && hq % hk == 0, "fa_kvcache_mq: needs h_k | h_q");
  TORCH_CHECK(b >= 1 && b <= 65535 && hk <= 65535 && sq >= 1 &&
                  sq * (hq / hk) <= (1L << 30),
              "fa_kvcache_mq: batch / heads / rows out of range");
  const int* klp = kvc_check_lens(MQ_OP, k_lens, q, "k_lens");
  const int* qlp = nullptr;
  if (kvc_present(q_lens)) qlp = kvc_check_lens(MQ_OP, q_lens, q, "q_lens");
  const KvcGeometry geo = kvc_check_geometry(MQ_OP, q, k_cache, block_table);
  const float *ks = nullptr, *vs = nullptr;
  if constexpr (FP8) {
    ks = kvc_check_scale(MQ_OP, k_scale, k_cache, "k_scale");
    vs = kvc_check_scale(MQ_OP, v_scale, v_cache, "v_scale");
  }
  wl = std::min<long>(wl, 1L << 30);  // anything larger is "no window"

  auto o = torch::empty_like(q);
  auto lse = torch::empty({b, hq, sq}, q.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
#define MQ_LAUNCH(DD)                                                        \
  FP16_SWITCH(q.scalar_type() == torch::kHalf,                               \
              mq_launch<DD, kFP16, PAGED, FP8>(                              \
                  q, k_cache, v_cache, klp, qlp, o, lse, (int)geo.cap,       \
                  (float)softmax_scale, (int)wl, geo.table, geo.page_shift,  \
                  ks, vs, stream))
  if (D == 128) MQ_LAUNCH(128); else MQ_LAUNCH(64);
#undef MQ_LAUNCH
  HIP_CHECK_LAST();
  return {o, lse};
}

}  // namespace

// q_lens, block_table, k_scale and v_scale are optional: an undefined or
// empty 1-d tensor means absent. With a table the caches are page pools
// [num_pages, page_size, hk, d]. With scales (fp32 [hk] on the device, both
// or neither) they hold float8_e4m3fn codes: score = softmax_scale *
// k_scale[kh] * (q . K8), out = v_scale[kh] * sum p V8.
std::vector<torch::Tensor> fa_kvcache_mq(
    torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor k_lens, torch::Tensor q_lens, torch::Tensor block_table,
    torch::Tensor k_scale, torch::Tensor v_scale, double softmax_scale,
    long wl) {
  const bool fp8 = kvc_present(k_scale);
  TORCH_CHECK(fp8 == kvc_present(v_scale),
              "fa_kvcache_mq: k_scale and v_scale come together");
  auto run = kvc_present(block_table)
                 ? (fp8 ? mq_run<true, true> : mq_run<true, false>)
                 : (fp8 ? mq_run<false, true> : mq_run<false, false>);
  return run(q, k_cache, v_cache, k_lens, q_lens, block_table, k_scale,
             v_scale, softmax_scale, wl);
}
