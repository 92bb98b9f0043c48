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
//   - Row tile = 4 waves x 32 rows = 128 packed rows (256 threads). Without
//     SPLIT (below) the row tiles are the only parallelism
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
//   - SPLIT (compile-time): split-KV, the decode kernel's cut applied per
//     workgroup. The grid's x dimension carries (row tile, split); a workgroup
//     computes its own tile range [t0, t1) as above, then takes tps =
//     ceil(ntiles / num_splits) tiles starting at t0 + split * tps. The key
//     range that loads clamp into, and that stage_write zeroes outside of,
//     is the intersection of the split's tiles with [kv_lo, kv_hi), so the
//     guarantees about invisible slots and table entries hold per split. The
//     epilogue writes fp32 partials (normalised row, v_scale applied, and the
//     split's lse; -inf for every row the split holds no visible key of, whose
//     row of o_part stays unwritten), and fa_kvcache_mq_combine_kernel forms
//     the fixed-order log-sum-exp weighted sum per (b, j, h) row. The
//     workspace is never initialised: the combine reads an o_part row only
//     behind a finite lse. SPLIT = false is the kernel without any of this;
//     it receives an empty MqSplit and reads none of it.
// Plain vector stores only, no atomics, one fixed reduction order: the result
// is deterministic for a given num_splits.
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

// Split-KV arguments. Empty without SPLIT, so those instances receive no
// workspace pointers (as DecScales<FP8> in flash_attn_decode.hip).
//   o_part   [b, sq, hq, num_splits, d]  fp32, normalised rows
//   lse_part [b, sq, hq, num_splits]     fp32
// Both are indexed by the row of O, (b * sq + j) * hq + h: the combine reads
// the num_splits lse values and rows of one output row back to back.
template <bool SPLIT>
struct MqSplit {};

template <>
struct MqSplit<true> {
  float* o_part;
  float* lse_part;
  int num_splits;
};

// In HIP the second launch-bounds argument is waves per SIMD: 2 gives a
// 256-VGPR budget (the 64 KB of LDS at d = 128 admit 2 workgroups per CU).
template <int D, bool FP16, bool PAGED, bool FP8, bool SPLIT>
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
                          const float* __restrict__ v_scale,
                          MqSplit<SPLIT> sp) {
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
  // SPLIT: blockIdx.x = row tile * num_splits + split
  int m0wg_x = blockIdx.x * MQ_ROWS;
  int split = 0;
  if constexpr (SPLIT) {
    const int row_tile = blockIdx.x / sp.num_splits;
    split = blockIdx.x - row_tile * sp.num_splits;
    m0wg_x = row_tile * MQ_ROWS;
  }
  const int m0wg = m0wg_x;
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
  int kv_hi = min(L, max(0, shift + jl_wg + 1));                 // exclusive
  int kv_lo = (wl >= 0) ? max(0, max(shift + jf_wg, 0) - wl) : 0;
  int t0 = kv_lo / KVB;
  const int t1 = (kv_hi + KVB - 1) / KVB;                        // exclusive
  int ntiles = (jf_wg < n && kv_hi > kv_lo) ? t1 - t0 : 0;
  if constexpr (SPLIT) {
    // this split's tiles [tb, te) of the workgroup's own range, and the key
    // range narrowed to them. With ntiles > 0 afterwards, t0 <= tb < te <= t1
    // gives max(kv_lo, tb * KVB) < min(kv_hi, te * KVB): the clamp of src_key
    // stays inside the split and inside [kv_lo, kv_hi).
    const int tps = (ntiles + sp.num_splits - 1) / sp.num_splits;
    const int tb = t0 + split * tps;
    const int te = min(t0 + ntiles, tb + tps);
    ntiles = max(te - tb, 0);
    t0 = tb;
    kv_lo = max(kv_lo, tb * KVB);
    kv_hi = min(kv_hi, te * KVB);
  }

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
  if constexpr (SPLIT) {
    // fp32 partials. Every row gets its lse (-inf: the split is empty for the
    // workgroup, the wave or the row); only rows with a visible key in this
    // split write their normalised row, with 16-byte stores.
    if (in_range) {
      const long prow_idx =
          (((long)(b * (long)sq + jr) * hq + h) * sp.num_splits + split);
      if (l_run > 0.f) {
        float inv_l = 1.f / l_run;
        if constexpr (FP8) inv_l *= v_scale[kh];   // once per normalised row
        float* op = sp.o_part + prow_idx * D;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            // registers 4g..4g+3 are d = a*32 + 8g + 4hi + 0..3
            f32x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = oacc[a][4 * g + e] * inv_l;
            *reinterpret_cast<f32x4*>(op + a * 32 + CROW(4 * g, hi)) = w;
          }
        }
      }
      if (hi == 0) {
        sp.lse_part[prow_idx] =
            (l_run > 0.f) ? m_run + __logf(l_run) : -INFINITY;
      }
    }
  } else if (in_range) {
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

// Split-KV combine: one fixed-order log-sum-exp weighted sum of the
// normalised partials per output row (b, j, h). D / 4 adjacent lanes serve a
// row, 4 head-dim elements each (16-byte loads, one 8-byte store); a 256-thread
// workgroup serves 1024 / D rows. A split whose lse is -inf is skipped without
// reading its (possibly never written) partial row.
constexpr int MQ_COMBINE_THREADS = 256;

template <int D, bool FP16>
__global__ __launch_bounds__(MQ_COMBINE_THREADS)
void fa_kvcache_mq_combine_kernel(const float* __restrict__ o_part,
                                  const float* __restrict__ lse_part,
                                  short* __restrict__ O,
                                  float* __restrict__ LSE, long rows, int sq,
                                  int hq, int num_splits) {
  using ET = AttnElem<FP16>;
  constexpr int LPR = D / 4;                     // lanes per row
  constexpr int RPB = MQ_COMBINE_THREADS / LPR;  // rows per workgroup
  const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
  if (row >= rows) return;
  const int d = (threadIdx.x % LPR) * 4;
  const float* lp = lse_part + row * num_splits;
  float mx = -INFINITY;
  for (int s = 0; s < num_splits; ++s) mx = fmaxf(mx, lp[s]);
  float wsum = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  if (mx != -INFINITY) {  // otherwise -inf - -inf
    for (int s = 0; s < num_splits; ++s) {
      const float ls = lp[s];
      if (ls != -INFINITY) {
        const float w = __expf(ls - mx);
        wsum += w;
        const f32x4 p = *reinterpret_cast<const f32x4*>(
            o_part + (row * num_splits + s) * D + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += w * p[e];
      }
    }
  }
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  s16x4 w;
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = ET::from_f32(o[e] * inv);
  *reinterpret_cast<s16x4*>(O + row * D + d) = w;
  if (d == 0) {
    // row = (b * sq + j) * hq + h -> LSE[b, h, j]
    const long bj = row / hq;
    const int h = (int)(row - bj * hq);
    const long bb = bj / sq;
    const int j = (int)(bj - bb * sq);
    LSE[(bb * hq + h) * sq + j] =
        wsum > 0.f ? mx + __logf(wsum) : -INFINITY;
  }
}

// Host-side split choice, from shapes and the CU count alone (no device data,
// no sync, safe under graph capture; the tiles are cut on the device). Aim
// for ~2 workgroups per CU over b * hk * row_tiles. A split must be able to
// own MQ_MIN_KEYS_PER_SPLIT slots of the cache: one that owns fewer than 8
// tiles reads at most 8 x 32 KB of K/V at d = 128 while it may write 64 KB of
// partials, so the floor is at least 512 whatever the timing says, and the
// choice is 1 for every cap < 2 * floor. MQ_MAX_SPLITS bounds the automatic
// choice (workspace, combine loop); MQ_SPLIT_LIMIT bounds a forced count.
// Values and the rows that decided them: profiles/r11_kvcache_chunk_split.md.
constexpr long MQ_MIN_KEYS_PER_SPLIT = 512;
constexpr long MQ_MAX_SPLITS = 32;
constexpr long MQ_SPLIT_LIMIT = 128;

long mq_choose_num_splits(long b, long hk, long packed_rows, long cap,
                          long num_cus) {
  const long row_tiles = (packed_rows + MQ_ROWS - 1) / MQ_ROWS;
  const long base = std::max<long>(b * hk * row_tiles, 1);
  long s = (2 * num_cus) / base;
  s = std::min(s, cap / MQ_MIN_KEYS_PER_SPLIT);
  s = std::min(s, MQ_MAX_SPLITS);
  return std::max<long>(s, 1);
}

// ns == 1: the unsplit instance writes O / LSE, sp_o / sp_lse are unused.
// ns > 1: the split instance writes the partials, then the combine.
template <int D, bool FP16, bool PAGED, bool FP8>
void mq_launch(const torch::Tensor& q, const torch::Tensor& k,
               const torch::Tensor& v, const int* klp, const int* qlp,
               torch::Tensor& o, torch::Tensor& lse, int cap, float scale,
               int wl, const int* bt, int page_shift, const float* k_scale,
               const float* v_scale, int ns, float* o_part, float* lse_part,
               hipStream_t stream) {
  const int b = q.size(0), sq = q.size(1), hq = q.size(2);
  const int hk = k.size(2);
  const int rows = sq * (hq / hk);
  const int row_tiles = (rows + MQ_ROWS - 1) / MQ_ROWS;
  const int lds = 4 * MQ_KVB * D * 2;  // K + V^T, double buffered
#define MQ_KERNEL_ARGS                                                       \
  (const short*)q.data_ptr(), (const void*)k.data_ptr(),                     \
      (const void*)v.data_ptr(), klp, qlp, (short*)o.data_ptr(),             \
      lse.data_ptr<float>(), sq, cap, hq, hk, (long)k.stride(0),             \
      (long)k.stride(1), (long)v.stride(0), (long)v.stride(1), scale, wl,    \
      bt, page_shift, PAGED ? (int)k.size(0) : 0, k_scale, v_scale
  if (ns == 1) {
    hipLaunchKernelGGL((fa_kvcache_mq_kernel<D, FP16, PAGED, FP8, false>),
                       dim3(row_tiles, hk, b), dim3(MQ_THREADS), lds, stream,
                       MQ_KERNEL_ARGS, MqSplit<false>{});
    return;
  }
  hipLaunchKernelGGL((fa_kvcache_mq_kernel<D, FP16, PAGED, FP8, true>),
                     dim3(row_tiles * ns, hk, b), dim3(MQ_THREADS), lds,
                     stream, MQ_KERNEL_ARGS,
                     MqSplit<true>{o_part, lse_part, ns});
#undef MQ_KERNEL_ARGS
  constexpr int RPB = MQ_COMBINE_THREADS / (D / 4);
  const long out_rows = (long)b * sq * hq;
  hipLaunchKernelGGL((fa_kvcache_mq_combine_kernel<D, FP16>),
                     dim3((unsigned)((out_rows + RPB - 1) / RPB)),
                     dim3(MQ_COMBINE_THREADS), 0, stream, o_part, lse_part,
                     (short*)o.data_ptr(), lse.data_ptr<float>(), out_rows,
                     sq, hq, ns);
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
                                  double softmax_scale, long wl,
                                  long num_splits) {
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

  TORCH_CHECK(num_splits >= 0 && num_splits <= MQ_SPLIT_LIMIT,
              "fa_kvcache_mq: num_splits must be in [0, ", MQ_SPLIT_LIMIT,
              "] (0: chosen from the shapes, 1: no split), got ", num_splits);
  const long packed_rows = sq * (hq / hk);
  long ns = num_splits;
  if (ns == 0)
    ns = mq_choose_num_splits(
        b, hk, packed_rows, geo.cap,
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  if (ns > 1) {
    // grid x carries (row tile, split); the combine serves >= 8 rows per
    // workgroup. Both stay below 2^24 workgroups of 256 threads.
    const long row_tiles = (packed_rows + MQ_ROWS - 1) / MQ_ROWS;
    TORCH_CHECK(row_tiles * ns <= (1L << 23) && b * sq * hq <= (1L << 26),
                "fa_kvcache_mq: too many rows for num_splits = ", ns,
                "; use num_splits = 1");
  }

  auto o = torch::empty_like(q);
  auto lse = torch::empty({b, hq, sq}, q.options().dtype(torch::kFloat32));
  torch::Tensor o_part, lse_part;  // no memset: see the kernels
  float *opp = nullptr, *lpp = nullptr;
  if (ns > 1) {
    o_part = torch::empty({b, sq, hq, ns, D}, lse.options());
    lse_part = torch::empty({b, sq, hq, ns}, lse.options());
    opp = o_part.data_ptr<float>();
    lpp = lse_part.data_ptr<float>();
  }
  auto stream = at::hip::getCurrentHIPStream();
#define MQ_LAUNCH(DD)                                                        \
  FP16_SWITCH(q.scalar_type() == torch::kHalf,                               \
              mq_launch<DD, kFP16, PAGED, FP8>(                              \
                  q, k_cache, v_cache, klp, qlp, o, lse, (int)geo.cap,       \
                  (float)softmax_scale, (int)wl, geo.table, geo.page_shift,  \
                  ks, vs, (int)ns, opp, lpp, stream))
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
// k_scale[kh] * (q . K8), out = v_scale[kh] * sum p V8. num_splits: 0 lets
// the host choose the number of key splits from the shapes, 1 runs the
// unsplit kernel, 2..MQ_SPLIT_LIMIT (128) forces that count.
std::vector<torch::Tensor> fa_kvcache_mq(
    torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor k_lens, torch::Tensor q_lens, torch::Tensor block_table,
    torch::Tensor k_scale, torch::Tensor v_scale, double softmax_scale,
    long wl, long num_splits) {
  const bool fp8 = kvc_present(k_scale);
  TORCH_CHECK(fp8 == kvc_present(v_scale),
              "fa_kvcache_mq: k_scale and v_scale come together");
  auto run = kvc_present(block_table)
                 ? (fp8 ? mq_run<true, true> : mq_run<true, false>)
                 : (fp8 ? mq_run<false, true> : mq_run<false, false>);
  return run(q, k_cache, v_cache, k_lens, q_lens, block_table, k_scale,
             v_scale, softmax_scale, wl, num_splits);
}

// The automatic choice as a pure function of the shapes (tests, benchmarks).
long fa_kvcache_mq_num_splits(long b, long hk, long packed_rows, long cap,
                              long num_cus) {
  TORCH_CHECK(b >= 1 && hk >= 1 && packed_rows >= 1 && cap >= 1 &&
                  num_cus >= 1,
              "fa_kvcache_mq_num_splits: every argument must be >= 1");
  return mq_choose_num_splits(b, hk, packed_rows, cap, num_cus);
}

// {MQ_MIN_KEYS_PER_SPLIT, MQ_MAX_SPLITS, MQ_SPLIT_LIMIT}
std::vector<long> fa_kvcache_mq_split_constants() {
  return {MQ_MIN_KEYS_PER_SPLIT, MQ_MAX_SPLITS, MQ_SPLIT_LIMIT};
}
