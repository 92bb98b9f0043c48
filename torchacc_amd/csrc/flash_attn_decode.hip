// Split-KV single-query (decode) attention over an in-place KV cache, gfx950.
//
// Decode attention is a memory-bound stream of the KV cache against at most
// a handful of query rows per kv head, so it gets its own kernel instead of
// the 256-row MFMA tile of flash_attn_fwd.hip:
//   - one workgroup serves ALL q heads of one kv head (groups of <= 8 rows),
//     so K and V are read once per kv head, not once per q head;
//   - the key axis is cut into num_splits chunks, computed ON THE DEVICE from
//     k_lens[b] and the window, so one short sequence in a large preallocated
//     cache still spreads over its workgroups;
//   - the cache is read where it lies: batch and sequence strides are kernel
//     arguments, only [heads][d] must be dense;
//   - two plain launches (split, then combine). No atomics, no flags, no
//     in-launch hand-off; fixed summation order, so results are bitwise
//     reproducible for a given num_splits. With num_splits == 1 the split
//     kernel writes the final output and the combine launch is skipped.
//
// Inner loop: pure fp32 VALU rather than a padded-MFMA tile. K and V
// go straight from global memory to VGPRs with 16-byte loads (operand is
// streamed once and shared by no other wave, so an LDS round trip would be
// pure overhead). D/8 adjacent lanes own one key: each lane holds 8 head-dim
// elements of K and of V, the q.k dot product is finished across those lanes
// with DPP adds, and every key group keeps its own online-softmax state
// (m, l, acc) that is merged once at the end (wave shuffles, then LDS across
// the 4 waves). Why VALU and not MFMA: with R <= 8 query rows the arithmetic
// intensity is <= 8 flop per KV byte, i.e. <= ~50 TFLOP/s at the ~6.3 TB/s
// the HBM sustains, a third of the 157 TFLOP/s fp32 vector peak; a 32-wide
// MFMA tile would spend >= 3/4 of its columns on padding and needs V
// transposed through LDS. R = 8 is the tight case (the per-key softmax and
// conversion instructions come on top of the FMAs); R <= 4 is memory-bound.
//
// Masking: keys outside [lo, klen) are never loaded (their registers are
// zero) and their scores are -inf, so whatever lies in unwritten cache slots
// cannot reach the result, not even as 0 * NaN.
//
// Paged variant (PAGED = true): K and V are page pools [num_pages,
// page_size, hk, d] and block_table[b][key >> shift] names the physical page
// of a logical key. Only the address computation differs: slot, dofs, the
// tile loop, the split chunks and every arithmetic step are the contiguous
// kernel's, so the result is bitwise the contiguous kernel's on the gathered
// cache at the same num_splits. The table entries of a tile are fetched one
// tile before its K/V loads are issued (two tiles before they are used), so
// no table read sits in front of a K/V prefetch inside the loop; only
// entries of keys < end are read (never those of logical pages past the
// live length), and each is clamped into [0, num_pages - 1] before use.
//
// fp8 variant (fa_decode_split_fp8_kernel): K and V hold OCP e4m3fn codes
// (one byte per element) with one fp32 scale per kv head each; q, the output
// and all arithmetic stay as they are. The lane mapping is unchanged: D/8
// lanes per key, 8 elements per lane, so a lane's load is 8 bytes instead of 16 and
// slot, dofs, the tile loop, the split chunks and the merge order are those
// of the 16-bit kernel. k_scale[kh] is folded into the q pre-scale and
// v_scale[kh] multiplies the normalised row once in the epilogue, so the
// inner loop gains only the fp8 -> fp32 conversions (v_cvt_pk_f32_fp8, two
// elements each). Both scales are read from device memory by the kernel.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "attn_common.h"

namespace {

constexpr int DEC_THREADS = 256;  // 4 waves
// Keys per tile. 64, except 32 for the largest instance (8 rows x 128 dims):
// 64 q + 64 accumulator registers leave room for 2 keys per lane in flight,
// not 4, without scratch spills.
constexpr int dec_tile_keys(int d, int r) { return (d * r > 512) ? 32 : 64; }
constexpr int DEC_MAX_ROWS = 8;   // q heads served by one workgroup
// host split choice (choose_num_splits)
constexpr int DEC_MIN_KEYS_PER_SPLIT = 256;
constexpr int DEC_MAX_SPLITS = 64;

// DPP lane exchanges inside a 16-lane row. After the two quad steps every
// lane of a quad holds the same partial sum, so the mirrors (i -> 7-i,
// i -> 15-i) serve as xor 4 / xor 8.
template <int CTRL>
DEVINLINE float dec_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                         0xf, 0xf, false));
}

// sum over the LPK (8 or 16) adjacent lanes that share a key
template <int LPK>
DEVINLINE float dec_group_sum(float v) {
  v += dec_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dec_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dec_dpp<0x141>(v);  // row_half_mirror
  if (LPK == 16) v += dec_dpp<0x140>(v);  // row_mirror
  return v;
}

// In HIP the second launch-bounds argument is the minimum number of waves
// per execution unit (SIMD), not blocks per CU: 2 gives a 256-VGPR budget.
template <int D, int R, bool FP16, bool PAGED>
__global__ __launch_bounds__(DEC_THREADS, 2)
void fa_decode_split_kernel(const short* __restrict__ Q,
                            const short* __restrict__ K,
                            const short* __restrict__ V,
                            const int* __restrict__ k_lens,
                            short* __restrict__ O, float* __restrict__ LSE,
                            float* __restrict__ o_part,
                            float* __restrict__ lse_part, int cap, int hq,
                            int hk, long k_sb, long k_ss, long v_sb,
                            long v_ss, float scale_log2, int wl,
                            int num_splits,
                            // PAGED only: k_sb / v_sb are the page strides,
                            // cap = table_width << page_shift
                            const int* __restrict__ block_table,
                            int page_shift, int num_pages) {
  using ET = AttnElem<FP16>;
  constexpr int LPK = D / 8;          // lanes per key
  constexpr int KPW = 64 / LPK;       // keys per wave per load
  constexpr int S = 4 * KPW;          // key slots per workgroup
  constexpr int DEC_TK = dec_tile_keys(D, R);
  constexpr int U = DEC_TK / S;       // keys per lane per tile
  constexpr float LN2 = 0.6931471805599453f;

  __shared__ float o_lds[4][R][D];
  __shared__ float m_lds[4][R];
  __shared__ float l_lds[4][R];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int slot = wid * KPW + lane / LPK;
  const int dofs = (lane % LPK) * 8;

  const int split = blockIdx.x;
  const int rep = hq / hk;
  const int ngroups = (rep + DEC_MAX_ROWS - 1) / DEC_MAX_ROWS;
  const int kh = blockIdx.y / ngroups;
  const int g = blockIdx.y % ngroups;
  const int b = blockIdx.z;
  const int h0 = kh * rep + g * DEC_MAX_ROWS;          // first q head
  const int nrows = min(R, rep - g * DEC_MAX_ROWS);    // real q rows

  // ---- this split's key chunk, from the device-side length --------------
  int klen = cap;
  if (k_lens != nullptr) klen = min(max(k_lens[b], 0), cap);
  const int lo = (wl >= 0) ? max(0, klen - 1 - wl) : 0;
  const int tiles = (klen - lo + DEC_TK - 1) / DEC_TK;
  const int tps = (tiles + num_splits - 1) / num_splits;  // tiles per split
  const int begin = lo + split * tps * DEC_TK;
  const int end = min(klen, begin + tps * DEC_TK);

  if (begin >= end) {  // empty split (uniform over the workgroup)
    if (num_splits == 1) {
      for (int e = tid; e < nrows * D; e += DEC_THREADS)
        O[(long)(b * hq + h0) * D + e] = 0;
      if (tid < nrows) LSE[b * hq + h0 + tid] = -INFINITY;
    } else if (tid < nrows) {
      lse_part[(long)(b * hq + h0 + tid) * num_splits + split] = -INFINITY;
    }
    return;
  }

  // ---- q rows, pre-scaled by softmax_scale * log2(e), fp32 ---------------
  float q[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s16x8 v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (r < nrows)
      v = *reinterpret_cast<const s16x8*>(Q + (long)(b * hq + h0 + r) * D +
                                          dofs);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[r][j] = ET::to_f32(v[j]) * scale_log2;
  }

  const short* kp = K + (PAGED ? 0L : (long)b * k_sb) + (long)kh * D + dofs;
  const short* vp = V + (PAGED ? 0L : (long)b * v_sb) + (long)kh * D + dofs;

  // PAGED: this sequence's table row, and the clamped physical pages of the
  // U keys a lane owns in a tile. Entries are read for keys < end only, i.e.
  // for logical pages < ceil(len / page_size): a lane whose key lies past
  // the chunk reads the entry of key end - 1 instead (begin < end here), so
  // the load needs no branch and the U loads of a tile issue back to back.
  const int* bt = PAGED ? block_table + (long)b * (cap >> page_shift) : nullptr;
  auto load_pages = [&](int key0, int* pg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = min(key0 + u * S + slot, end - 1);
      pg[u] = min(max(bt[key >> page_shift], 0), num_pages - 1);
    }
  };

  // keys outside [begin, end) are not loaded: their registers are zero
  auto load_tile = [&](const short* base, long sb, long ss, int key0,
                       const int* pg, s16x8* reg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = key0 + u * S + slot;
      if constexpr (PAGED) {
        const int in_page = key & ((1 << page_shift) - 1);
        reg[u] = (key < end)
                     ? *reinterpret_cast<const s16x8*>(
                           base + (long)pg[u] * sb + (long)in_page * ss)
                     : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      } else {
        reg[u] = (key < end)
                     ? *reinterpret_cast<const s16x8*>(base + (long)key * ss)
                     : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
  }

  s16x8 kreg[U], vreg[U];
  // pg: pages of the tile whose K/V are loaded next; pg_ahead: the tile
  // after that, in flight while this tile computes (PAGED only)
  int pg[U], pg_ahead[U];
  if constexpr (PAGED) load_pages(begin, pg);
  load_tile(kp, k_sb, k_ss, begin, pg, kreg);
  load_tile(vp, v_sb, v_ss, begin, pg, vreg);
  if constexpr (PAGED) load_pages(begin + DEC_TK, pg);

  for (int kt = begin; kt < end; kt += DEC_TK) {
    if constexpr (PAGED) load_pages(kt + 2 * DEC_TK, pg_ahead);
    // ---- scores: s[r][u] = q[r] . K[key_u], log2 domain ------------------
    float s[R][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = ET::to_f32(kreg[u][j]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaf(q[r][j], kf[j], a);
        s[r][u] = a;
      }
    }
    // K registers are free: the next tile's K flies under softmax and PV
    load_tile(kp, k_sb, k_ss, kt + DEC_TK, pg, kreg);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = (kt + u * S + slot) < end;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float t = dec_group_sum<LPK>(s[r][u]);
        s[r][u] = valid ? t : -INFINITY;
      }
    }

    // ---- online softmax per key group ------------------------------------
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mx = s[r][0];
#pragma unroll
      for (int u = 1; u < U; ++u) mx = fmaxf(mx, s[r][u]);
      const float m_new = fmaxf(m[r], mx);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = exp2f(m[r] - m_use);  // m = -inf -> 0
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[r][u] = exp2f(s[r][u] - m_use);       // masked -> 0
        ps += s[r][u];
      }
      l[r] = l[r] * alpha + ps;
      m[r] = m_new;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] *= alpha;
    }

    // ---- acc[r] += p[r][u] * V[key_u] ------------------------------------
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = ET::to_f32(vreg[u][j]);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r][j] = fmaf(s[r][u], vf[j], acc[r][j]);
    }
    load_tile(vp, v_sb, v_ss, kt + DEC_TK, pg, vreg);
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; ++u) pg[u] = pg_ahead[u];
    }
  }

  // ---- merge the key groups of a wave (fixed butterfly order) ------------
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float mw = m[r];
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1)
      mw = fmaxf(mw, __shfl_xor(mw, off, 64));
    const float m_use = (mw == -INFINITY) ? 0.f : mw;
    const float sc = exp2f(m[r] - m_use);
    float lr = l[r] * sc;
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) lr += __shfl_xor(lr, off, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[r][j] * sc;
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
      acc[r][j] = a;
    }
    m[r] = mw;
    l[r] = lr;
  }
  if (lane < LPK) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) o_lds[wid][r][dofs + j] = acc[r][j];
      if (lane == 0) {
        m_lds[wid][r] = m[r];
        l_lds[wid][r] = l[r];
      }
    }
  }
  __syncthreads();

  // ---- merge the 4 waves, normalise, store -------------------------------
  for (int e = tid; e < nrows * D; e += DEC_THREADS) {
    const int r = e / D, d = e % D;
    float mm = m_lds[0][r];
#pragma unroll
    for (int w = 1; w < 4; ++w) mm = fmaxf(mm, m_lds[w][r]);
    const float m_use = (mm == -INFINITY) ? 0.f : mm;
    float lsum = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float sc = exp2f(m_lds[w][r] - m_use);
      lsum += l_lds[w][r] * sc;
      o += o_lds[w][r][d] * sc;
    }
    const float on = (lsum > 0.f) ? o / lsum : 0.f;
    const float lse = (lsum > 0.f) ? mm * LN2 + __logf(lsum) : -INFINITY;
    const long row = b * hq + h0 + r;
    if (num_splits == 1) {
      O[row * D + d] = ET::from_f32(on);
      if (d == 0) LSE[row] = lse;
    } else {
      o_part[(row * num_splits + split) * D + d] = on;
      if (d == 0) lse_part[row * num_splits + split] = lse;
    }
  }
}

// 8 e4m3 codes of one lane as fp32
DEVINLINE void dec_cvt8_fp8(const u32x2& r, float* f) {
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], true);
    f[4 * w + 0] = a[0];
    f[4 * w + 1] = a[1];
    f[4 * w + 2] = b[0];
    f[4 * w + 3] = b[1];
  }
}

// fa_decode_split_kernel for float8_e4m3fn caches (see the header comment).
// A sibling, not a flag: the 16-bit kernel above stays as it was compiled,
// with its register figures. Everything not marked "fp8:" is that kernel's
// text; K / V point at bytes and every cache stride counts bytes.
template <int D, int R, bool FP16, bool PAGED>
__global__ __launch_bounds__(DEC_THREADS, 2)
void fa_decode_split_fp8_kernel(const short* __restrict__ Q,
                                const unsigned char* __restrict__ K,
                                const unsigned char* __restrict__ V,
                                const int* __restrict__ k_lens,
                                short* __restrict__ O,
                                float* __restrict__ LSE,
                                float* __restrict__ o_part,
                                float* __restrict__ lse_part, int cap, int hq,
                                int hk, long k_sb, long k_ss, long v_sb,
                                long v_ss, float scale_log2, int wl,
                                int num_splits,
                                // PAGED only: k_sb / v_sb are the page
                                // strides, cap = table_width << page_shift
                                const int* __restrict__ block_table,
                                int page_shift, int num_pages,
                                // fp8: fp32 [hk] each
                                const float* __restrict__ k_scale,
                                const float* __restrict__ v_scale) {
  using ET = AttnElem<FP16>;
  // fp8: cache element and the 8 elements a lane loads at once (8 bytes)
  using KE = unsigned char;
  using KV8 = u32x2;
  constexpr int LPK = D / 8;          // lanes per key
  constexpr int KPW = 64 / LPK;       // keys per wave per load
  constexpr int S = 4 * KPW;          // key slots per workgroup
  constexpr int DEC_TK = dec_tile_keys(D, R);
  constexpr int U = DEC_TK / S;       // keys per lane per tile
  constexpr float LN2 = 0.6931471805599453f;

  __shared__ float o_lds[4][R][D];
  __shared__ float m_lds[4][R];
  __shared__ float l_lds[4][R];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int slot = wid * KPW + lane / LPK;
  const int dofs = (lane % LPK) * 8;

  const int split = blockIdx.x;
  const int rep = hq / hk;
  const int ngroups = (rep + DEC_MAX_ROWS - 1) / DEC_MAX_ROWS;
  const int kh = blockIdx.y / ngroups;
  const int g = blockIdx.y % ngroups;
  const int b = blockIdx.z;
  const int h0 = kh * rep + g * DEC_MAX_ROWS;          // first q head
  const int nrows = min(R, rep - g * DEC_MAX_ROWS);    // real q rows

  // ---- this split's key chunk, from the device-side length --------------
  int klen = cap;
  if (k_lens != nullptr) klen = min(max(k_lens[b], 0), cap);
  const int lo = (wl >= 0) ? max(0, klen - 1 - wl) : 0;
  const int tiles = (klen - lo + DEC_TK - 1) / DEC_TK;
  const int tps = (tiles + num_splits - 1) / num_splits;  // tiles per split
  const int begin = lo + split * tps * DEC_TK;
  const int end = min(klen, begin + tps * DEC_TK);

  if (begin >= end) {  // empty split (uniform over the workgroup)
    if (num_splits == 1) {
      for (int e = tid; e < nrows * D; e += DEC_THREADS)
        O[(long)(b * hq + h0) * D + e] = 0;
      if (tid < nrows) LSE[b * hq + h0 + tid] = -INFINITY;
    } else if (tid < nrows) {
      lse_part[(long)(b * hq + h0 + tid) * num_splits + split] = -INFINITY;
    }
    return;
  }

  // ---- q rows, pre-scaled by softmax_scale * log2(e), fp32 ---------------
  // fp8: times k_scale[kh], so the scores are those of the scaled keys
  const float q_scale = scale_log2 * k_scale[kh];
  float q[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s16x8 v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (r < nrows)
      v = *reinterpret_cast<const s16x8*>(Q + (long)(b * hq + h0 + r) * D +
                                          dofs);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[r][j] = ET::to_f32(v[j]) * q_scale;
  }

  const KE* kp = K + (PAGED ? 0L : (long)b * k_sb) + (long)kh * D + dofs;
  const KE* vp = V + (PAGED ? 0L : (long)b * v_sb) + (long)kh * D + dofs;

  // PAGED: this sequence's table row, and the clamped physical pages of the
  // U keys a lane owns in a tile. Entries are read for keys < end only, i.e.
  // for logical pages < ceil(len / page_size): a lane whose key lies past
  // the chunk reads the entry of key end - 1 instead (begin < end here), so
  // the load needs no branch and the U loads of a tile issue back to back.
  const int* bt = PAGED ? block_table + (long)b * (cap >> page_shift) : nullptr;
  auto load_pages = [&](int key0, int* pg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = min(key0 + u * S + slot, end - 1);
      pg[u] = min(max(bt[key >> page_shift], 0), num_pages - 1);
    }
  };

  // keys outside [begin, end) are not loaded: their registers are zero
  auto load_tile = [&](const KE* base, long sb, long ss, int key0,
                       const int* pg, KV8* reg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = key0 + u * S + slot;
      if constexpr (PAGED) {
        const int in_page = key & ((1 << page_shift) - 1);
        reg[u] = (key < end)
                     ? *reinterpret_cast<const KV8*>(
                           base + (long)pg[u] * sb + (long)in_page * ss)
                     : KV8{};
      } else {
        reg[u] = (key < end)
                     ? *reinterpret_cast<const KV8*>(base + (long)key * ss)
                     : KV8{};
      }
    }
  };

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
  }

  KV8 kreg[U], vreg[U];
  // pg: pages of the tile whose K/V are loaded next; pg_ahead: the tile
  // after that, in flight while this tile computes (PAGED only)
  int pg[U], pg_ahead[U];
  if constexpr (PAGED) load_pages(begin, pg);
  load_tile(kp, k_sb, k_ss, begin, pg, kreg);
  load_tile(vp, v_sb, v_ss, begin, pg, vreg);
  if constexpr (PAGED) load_pages(begin + DEC_TK, pg);

  for (int kt = begin; kt < end; kt += DEC_TK) {
    if constexpr (PAGED) load_pages(kt + 2 * DEC_TK, pg_ahead);
    // ---- scores: s[r][u] = q[r] . K[key_u], log2 domain ------------------
    float s[R][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      dec_cvt8_fp8(kreg[u], kf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaf(q[r][j], kf[j], a);
        s[r][u] = a;
      }
    }
    // K registers are free: the next tile's K flies under softmax and PV
    load_tile(kp, k_sb, k_ss, kt + DEC_TK, pg, kreg);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = (kt + u * S + slot) < end;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float t = dec_group_sum<LPK>(s[r][u]);
        s[r][u] = valid ? t : -INFINITY;
      }
    }

    // ---- online softmax per key group ------------------------------------
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mx = s[r][0];
#pragma unroll
      for (int u = 1; u < U; ++u) mx = fmaxf(mx, s[r][u]);
      const float m_new = fmaxf(m[r], mx);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = exp2f(m[r] - m_use);  // m = -inf -> 0
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[r][u] = exp2f(s[r][u] - m_use);       // masked -> 0
        ps += s[r][u];
      }
      l[r] = l[r] * alpha + ps;
      m[r] = m_new;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] *= alpha;
    }

    // ---- acc[r] += p[r][u] * V[key_u] ------------------------------------
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      dec_cvt8_fp8(vreg[u], vf);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[r][j] = fmaf(s[r][u], vf[j], acc[r][j]);
    }
    load_tile(vp, v_sb, v_ss, kt + DEC_TK, pg, vreg);
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; ++u) pg[u] = pg_ahead[u];
    }
  }

  // ---- merge the key groups of a wave (fixed butterfly order) ------------
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float mw = m[r];
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1)
      mw = fmaxf(mw, __shfl_xor(mw, off, 64));
    const float m_use = (mw == -INFINITY) ? 0.f : mw;
    const float sc = exp2f(m[r] - m_use);
    float lr = l[r] * sc;
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) lr += __shfl_xor(lr, off, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[r][j] * sc;
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
      acc[r][j] = a;
    }
    m[r] = mw;
    l[r] = lr;
  }
  if (lane < LPK) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) o_lds[wid][r][dofs + j] = acc[r][j];
      if (lane == 0) {
        m_lds[wid][r] = m[r];
        l_lds[wid][r] = l[r];
      }
    }
  }
  __syncthreads();

  // ---- merge the 4 waves, normalise, store -------------------------------
  const float o_scale = v_scale[kh];   // fp8: once per normalised row
  for (int e = tid; e < nrows * D; e += DEC_THREADS) {
    const int r = e / D, d = e % D;
    float mm = m_lds[0][r];
#pragma unroll
    for (int w = 1; w < 4; ++w) mm = fmaxf(mm, m_lds[w][r]);
    const float m_use = (mm == -INFINITY) ? 0.f : mm;
    float lsum = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float sc = exp2f(m_lds[w][r] - m_use);
      lsum += l_lds[w][r] * sc;
      o += o_lds[w][r][d] * sc;
    }
    const float on = ((lsum > 0.f) ? o / lsum : 0.f) * o_scale;
    const float lse = (lsum > 0.f) ? mm * LN2 + __logf(lsum) : -INFINITY;
    const long row = b * hq + h0 + r;
    if (num_splits == 1) {
      O[row * D + d] = ET::from_f32(on);
      if (d == 0) LSE[row] = lse;
    } else {
      o_part[(row * num_splits + split) * D + d] = on;
      if (d == 0) lse_part[row * num_splits + split] = lse;
    }
  }
}

// One workgroup of D threads per (batch, q head): fixed-order log-sum-exp
// weighted sum of the normalised partials. An empty split (lse = -inf) is
// skipped without reading its (never written) partial.
template <int D, bool FP16>
__global__ __launch_bounds__(D)
void fa_decode_combine_kernel(const float* __restrict__ o_part,
                              const float* __restrict__ lse_part,
                              short* __restrict__ O, float* __restrict__ LSE,
                              int num_splits) {
  using ET = AttnElem<FP16>;
  const long row = blockIdx.x;
  const int d = threadIdx.x;
  const float* lp = lse_part + row * num_splits;
  float mx = -INFINITY;
  for (int j = 0; j < num_splits; ++j) mx = fmaxf(mx, lp[j]);
  float wsum = 0.f, o = 0.f;
  if (mx != -INFINITY) {  // otherwise -inf - -inf
    for (int j = 0; j < num_splits; ++j) {
      const float lj = lp[j];
      if (lj != -INFINITY) {
        const float w = __expf(lj - mx);
        wsum += w;
        o += w * o_part[(row * num_splits + j) * D + d];
      }
    }
  }
  O[row * D + d] = ET::from_f32(wsum > 0.f ? o / wsum : 0.f);
  if (d == 0) LSE[row] = wsum > 0.f ? mx + __logf(wsum) : -INFINITY;
}

// Host-side split choice. It sees only shapes and the CU count, never device
// data (no sync, safe under graph capture): the key chunks themselves are
// cut on the device from k_lens. Aim for ~2 workgroups per CU; a split is
// worth its partial write and the combine launch only when it can own at
// least DEC_MIN_KEYS_PER_SPLIT slots of the cache; DEC_MAX_SPLITS bounds the
// workspace and the combine loop.
int choose_num_splits(int b, int hk_groups, int cap, int num_cus) {
  const long base = (long)b * hk_groups;
  long s = (2L * num_cus) / base;
  s = std::min<long>(s, cap / DEC_MIN_KEYS_PER_SPLIT);
  s = std::min<long>(s, DEC_MAX_SPLITS);
  return (int)std::max<long>(s, 1);
}

// Contiguous: k / v are [b, cap, hk, d] and bt is null. Paged: k / v are
// pools [num_pages, page_size, hk, d], bt is the [b, cap >> page_shift]
// table; the strides handed to the kernel are then the page and slot strides.
template <int D, int R, bool FP16, bool PAGED, bool FP8>
void launch_decode(const torch::Tensor& q, const torch::Tensor& k,
                   const torch::Tensor& v, const int* klp, torch::Tensor& o,
                   torch::Tensor& lse, float* o_part, float* lse_part,
                   float scale_log2, int wl, int num_splits, int groups,
                   hipStream_t stream, int cap, const int* bt,
                   int page_shift, const float* k_scale,
                   const float* v_scale) {
  const int b = q.size(0), hq = q.size(2);
  const int hk = k.size(2);
  const int num_pages = PAGED ? (int)k.size(0) : 0;
  dim3 grid(num_splits, hk * groups, b);
  if constexpr (FP8) {
    using byte = unsigned char;
    hipLaunchKernelGGL((fa_decode_split_fp8_kernel<D, R, FP16, PAGED>), grid,
                       dim3(DEC_THREADS), 0, stream,
                       (const short*)q.data_ptr(), (const byte*)k.data_ptr(),
                       (const byte*)v.data_ptr(), klp, (short*)o.data_ptr(),
                       lse.data_ptr<float>(), o_part, lse_part, cap, hq, hk,
                       (long)k.stride(0), (long)k.stride(1),
                       (long)v.stride(0), (long)v.stride(1), scale_log2, wl,
                       num_splits, bt, page_shift, num_pages, k_scale,
                       v_scale);
  } else {
    hipLaunchKernelGGL((fa_decode_split_kernel<D, R, FP16, PAGED>), grid,
                       dim3(DEC_THREADS), 0, stream,
                       (const short*)q.data_ptr(), (const short*)k.data_ptr(),
                       (const short*)v.data_ptr(), klp, (short*)o.data_ptr(),
                       lse.data_ptr<float>(), o_part, lse_part, cap, hq, hk,
                       (long)k.stride(0), (long)k.stride(1),
                       (long)v.stride(0), (long)v.stride(1), scale_log2, wl,
                       num_splits, bt, page_shift, num_pages);
  }
  if (num_splits > 1) {
    hipLaunchKernelGGL((fa_decode_combine_kernel<D, FP16>), dim3(b * hq),
                       dim3(D), 0, stream, o_part, lse_part,
                       (short*)o.data_ptr(), lse.data_ptr<float>(),
                       num_splits);
  }
}

void check_cache(const torch::Tensor& c, const torch::Tensor& q,
                 const char* name, bool fp8 = false) {
  TORCH_CHECK(c.is_cuda() && c.dim() == 4, "fa_decode: ", name,
              " must be a 4-d GPU tensor");
  TORCH_CHECK(c.stride(3) == 1 && c.stride(2) == c.size(3),
              "fa_decode: ", name, " needs dense [heads][head_dim]");
  if (fp8) {
    TORCH_CHECK(c.scalar_type() == torch::kFloat8_e4m3fn, "fa_decode_fp8: ",
                name, " must be float8_e4m3fn");
    // 8-byte loads of one-byte elements: strides are bytes here
    TORCH_CHECK(c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(c.data_ptr()) % 8 == 0,
                "fa_decode_fp8: ", name, " rows must be 8-byte aligned");
    return;
  }
  TORCH_CHECK(c.scalar_type() == q.scalar_type(), "fa_decode: ", name,
              " must be a 4-d GPU tensor of q's dtype");
  // 16-byte loads
  TORCH_CHECK(c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 == 0,
              "fa_decode: ", name, " rows must be 16-byte aligned");
}

// fp8 caches: one fp32 scale per kv head, read by the kernel
const float* check_scale(const torch::Tensor& s, const torch::Tensor& cache,
                         const char* name) {
  TORCH_CHECK(s.is_cuda() && s.scalar_type() == torch::kFloat32 &&
                  s.dim() == 1 && s.size(0) == cache.size(2) &&
                  s.is_contiguous() && s.device() == cache.device(),
              "fa_decode_fp8: ", name, " must be a GPU fp32 [hk]");
  return s.data_ptr<float>();
}

void check_q(const torch::Tensor& q) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.is_contiguous() &&
                  q.size(1) == 1,
              "fa_decode: q must be a contiguous GPU [b, 1, hq, d]");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 ||
                  q.scalar_type() == torch::kHalf,
              "fa_decode: bf16/fp16 only");
}

const int* check_lens(const torch::Tensor& k_lens, long b) {
  TORCH_CHECK(k_lens.is_cuda() && k_lens.scalar_type() == torch::kInt32 &&
                  k_lens.dim() == 1 && k_lens.size(0) == b &&
                  k_lens.is_contiguous(),
              "fa_decode: k_lens must be a GPU int32 [b]");
  return k_lens.data_ptr<int>();
}

// Shared tail of fa_decode / fa_decode_paged: shape checks that hold for
// both layouts, split choice, workspace, launches. `cap` is the contiguous
// capacity or table_width * page_size; hk = k.size(2) in both layouts.
template <bool PAGED, bool FP8>
std::vector<torch::Tensor> run_decode(const torch::Tensor& q,
                                      const torch::Tensor& k_cache,
                                      const torch::Tensor& v_cache,
                                      const int* klp, long cap,
                                      const int* bt, int page_shift,
                                      double softmax_scale, long wl,
                                      long num_splits,
                                      const float* k_scale = nullptr,
                                      const float* v_scale = nullptr) {
  const long b = q.size(0), hq = q.size(2), D = q.size(3);
  const long hk = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128, "fa_decode: head_dim must be 64 or 128");
  TORCH_CHECK(k_cache.size(3) == D);
  TORCH_CHECK(hk > 0 && hq % hk == 0, "fa_decode: needs h_k | h_q");
  TORCH_CHECK(b >= 1 && b <= 65535 && cap >= 1 && cap <= (1L << 30));
  TORCH_CHECK(num_splits >= 0 && num_splits <= 65535,
              "fa_decode: num_splits must be in [0, 65535]");
  wl = std::min<long>(wl, 1L << 30);  // anything larger is "no window"

  const int rep = hq / hk;
  const int groups = (rep + DEC_MAX_ROWS - 1) / DEC_MAX_ROWS;
  TORCH_CHECK(hk * groups <= 65535);
  int ns = (int)num_splits;
  if (ns == 0)
    ns = choose_num_splits(
        (int)b, (int)hk * groups, (int)cap,
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount);

  auto o = torch::empty_like(q);
  auto lse = torch::empty({b, hq, 1}, q.options().dtype(torch::kFloat32));
  torch::Tensor o_part, lse_part;  // no memset: see the kernels
  float *opp = nullptr, *lpp = nullptr;
  if (ns > 1) {
    o_part = torch::empty({b, hq, ns, D}, lse.options());
    lse_part = torch::empty({b, hq, ns}, lse.options());
    opp = o_part.data_ptr<float>();
    lpp = lse_part.data_ptr<float>();
  }
  const float scale_log2 = (float)softmax_scale * LOG2E_F;
  auto stream = at::hip::getCurrentHIPStream();

#define DEC_LAUNCH(DD, RR)                                                   \
  FP16_SWITCH(q.scalar_type() == torch::kHalf,                               \
              launch_decode<DD, RR, kFP16, PAGED, FP8>(                      \
                  q, k_cache, v_cache, klp, o, lse, opp, lpp, scale_log2,    \
                  (int)wl, ns, groups, stream, (int)cap, bt, page_shift,     \
                  k_scale, v_scale))
#define DEC_ROWS(DD)                                                         \
  do {                                                                       \
    if (rep == 1) DEC_LAUNCH(DD, 1);                                         \
    else if (rep == 2) DEC_LAUNCH(DD, 2);                                    \
    else if (rep <= 4) DEC_LAUNCH(DD, 4);                                    \
    else DEC_LAUNCH(DD, 8);                                                  \
  } while (0)
  if (D == 128) DEC_ROWS(128); else DEC_ROWS(64);
#undef DEC_ROWS
#undef DEC_LAUNCH
  HIP_CHECK_LAST();
  return {o, lse};
}

// Contiguous layout; k_scale / v_scale are null for the 16-bit caches.
template <bool FP8>
std::vector<torch::Tensor> decode_contiguous(
    const torch::Tensor& q, const torch::Tensor& k_cache,
    const torch::Tensor& v_cache, const torch::Tensor& k_lens,
    double softmax_scale, long wl, long num_splits, const float* k_scale,
    const float* v_scale) {
  check_q(q);
  check_cache(k_cache, q, "k_cache", FP8);
  check_cache(v_cache, q, "v_cache", FP8);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "fa_decode: k_cache and v_cache shapes differ");
  TORCH_CHECK(k_cache.size(0) == q.size(0));
  const int* klp = nullptr;
  if (k_lens.numel() > 0) klp = check_lens(k_lens, q.size(0));
  return run_decode<false, FP8>(q, k_cache, v_cache, klp, k_cache.size(1),
                                nullptr, 0, softmax_scale, wl, num_splits,
                                k_scale, v_scale);
}

// Paged layout: k_cache / v_cache are page pools [num_pages, page_size, hk,
// d], block_table is int32 [b, table_width]. Shape-only checks, no host
// sync: the table's contents are never read on the host (the kernel clamps
// every entry it dereferences into the pool).
template <bool FP8>
std::vector<torch::Tensor> decode_paged(
    const torch::Tensor& q, const torch::Tensor& k_cache,
    const torch::Tensor& v_cache, const torch::Tensor& k_lens,
    const torch::Tensor& block_table, double softmax_scale, long wl,
    long num_splits, const float* k_scale, const float* v_scale) {
  check_q(q);
  check_cache(k_cache, q, "k_cache", FP8);
  check_cache(v_cache, q, "v_cache", FP8);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "fa_decode_paged: k_cache and v_cache shapes differ");
  const long b = q.size(0);
  const long num_pages = k_cache.size(0), ps = k_cache.size(1);
  TORCH_CHECK(num_pages >= 1 && num_pages <= (1L << 30),
              "fa_decode_paged: the pool needs 1..2^30 pages");
  TORCH_CHECK(ps >= 16 && (ps & (ps - 1)) == 0,
              "fa_decode_paged: page_size must be a power of two >= 16, got ",
              ps);
  TORCH_CHECK(block_table.is_cuda() &&
                  block_table.scalar_type() == torch::kInt32 &&
                  block_table.dim() == 2 && block_table.size(0) == b &&
                  block_table.is_contiguous(),
              "fa_decode_paged: block_table must be a contiguous GPU int32 "
              "[b, table_width]");
  const long tw = block_table.size(1);
  TORCH_CHECK(tw >= 1 && tw * ps <= (1L << 30),
              "fa_decode_paged: table_width * page_size must be in "
              "[1, 2^30]");
  const int* klp = check_lens(k_lens, b);
  int shift = 0;
  while ((1L << shift) < ps) ++shift;
  return run_decode<true, FP8>(q, k_cache, v_cache, klp, tw * ps,
                               block_table.data_ptr<int>(), shift,
                               softmax_scale, wl, num_splits, k_scale,
                               v_scale);
}

}  // namespace

std::vector<torch::Tensor> fa_decode(torch::Tensor q, torch::Tensor k_cache,
                                     torch::Tensor v_cache,
                                     torch::Tensor k_lens,
                                     double softmax_scale, long wl,
                                     long num_splits) {
  return decode_contiguous<false>(q, k_cache, v_cache, k_lens, softmax_scale,
                                  wl, num_splits, nullptr, nullptr);
}

std::vector<torch::Tensor> fa_decode_paged(torch::Tensor q,
                                           torch::Tensor k_cache,
                                           torch::Tensor v_cache,
                                           torch::Tensor k_lens,
                                           torch::Tensor block_table,
                                           double softmax_scale, long wl,
                                           long num_splits) {
  return decode_paged<false>(q, k_cache, v_cache, k_lens, block_table,
                             softmax_scale, wl, num_splits, nullptr, nullptr);
}

// float8_e4m3fn caches with per-kv-head fp32 scales [hk] on the device:
// score = softmax_scale * k_scale[kh] * (q . K8), out = v_scale[kh] * sum p V8.
std::vector<torch::Tensor> fa_decode_fp8(torch::Tensor q,
                                         torch::Tensor k_cache,
                                         torch::Tensor v_cache,
                                         torch::Tensor k_lens,
                                         torch::Tensor k_scale,
                                         torch::Tensor v_scale,
                                         double softmax_scale, long wl,
                                         long num_splits) {
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4);
  const float* ks = check_scale(k_scale, k_cache, "k_scale");
  const float* vs = check_scale(v_scale, v_cache, "v_scale");
  return decode_contiguous<true>(q, k_cache, v_cache, k_lens, softmax_scale,
                                 wl, num_splits, ks, vs);
}

std::vector<torch::Tensor> fa_decode_paged_fp8(
    torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor k_lens, torch::Tensor block_table, torch::Tensor k_scale,
    torch::Tensor v_scale, double softmax_scale, long wl, long num_splits) {
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4);
  const float* ks = check_scale(k_scale, k_cache, "k_scale");
  const float* vs = check_scale(v_scale, v_cache, "v_scale");
  return decode_paged<true>(q, k_cache, v_cache, k_lens, block_table,
                            softmax_scale, wl, num_splits, ks, vs);
}

