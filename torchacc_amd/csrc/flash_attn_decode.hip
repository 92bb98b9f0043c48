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
// fp8 variant (FP8 = true): K and V hold OCP e4m3fn codes (one byte per
// element) with one fp32 scale per kv head each; q, the output and all
// arithmetic stay as they are. The lane mapping is unchanged: D/8 lanes per
// key, 8 elements per lane, so a lane's load is 8 bytes instead of 16 and
// slot, dofs, the tile loop, the split chunks and the merge order are those
// of the 16-bit kernel. k_scale[kh] is folded into the q pre-scale and
// v_scale[kh] multiplies the normalised row once in the epilogue, so the
// inner loop gains only the fp8 -> fp32 conversions (v_cvt_pk_f32_fp8, two
// elements each). Both scales are read from device memory by the kernel.
//
// There is one kernel, parameterised on how a lane holds its 8 cache elements
// (DecCache). The scales travel in DecScales<FP8>, which is
// empty without FP8, so the 16-bit instances keep the argument list they had
// before the fp8 cache existed (register figures and the assembly
// comparison: profiles/r10_kvcache_refactor.md).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "attn_common.h"
#include "kvcache_common.h"

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

// How a lane holds the 8 cache elements it loads at once: 16-bit elements of
// q's type (16 bytes), or e4m3 codes (8 bytes). Their conversion to fp32 is
// written out under `if constexpr (FP8)` in the kernel, not as a member
// here: routed through a helper, the 16-bit loops came out of the compiler
// in another schedule and the paged 8-row instances ran 2-5 % slower
// (profiles/r10_kvcache_refactor.md).
template <bool FP8>
struct DecCache {
  using elem = short;
  using vec8 = s16x8;
  static DEVINLINE vec8 zero() { return s16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
};

template <>
struct DecCache<true> {
  using elem = unsigned char;
  using vec8 = u32x2;
  static DEVINLINE vec8 zero() { return u32x2{}; }
};

// fp32 [hk] each, read by the kernel. Empty for the 16-bit caches, whose
// kernel then receives no scale pointers.
template <bool FP8>
struct DecScales {};

template <>
struct DecScales<true> {
  const float* k;
  const float* v;
};

// In HIP the second launch-bounds argument is the minimum number of waves
// per execution unit (SIMD), not blocks per CU: 2 gives a 256-VGPR budget.
template <int D, int R, bool FP16, bool PAGED, bool FP8>
__global__ __launch_bounds__(DEC_THREADS, 2)
void fa_decode_split_kernel(
    const short* __restrict__ Q,
    // FP8: K / V point at bytes and every cache stride counts bytes
    const typename DecCache<FP8>::elem* __restrict__ K,
    const typename DecCache<FP8>::elem* __restrict__ V,
    const int* __restrict__ k_lens, short* __restrict__ O,
    float* __restrict__ LSE, float* __restrict__ o_part,
    float* __restrict__ lse_part, int cap, int hq, int hk, long k_sb,
    long k_ss, long v_sb, long v_ss, float scale_log2, int wl,
    int num_splits,
    // PAGED only: k_sb / v_sb are the page strides, cap = table_width <<
    // page_shift
    const int* __restrict__ block_table, int page_shift, int num_pages,
    DecScales<FP8> scales) {
  using ET = AttnElem<FP16>;
  using KC = DecCache<FP8>;
  using KE = typename KC::elem;
  using KV8 = typename KC::vec8;
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
  // FP8: times k_scale[kh], so the scores are those of the scaled keys
  float q_scale = scale_log2;
  if constexpr (FP8) q_scale = scale_log2 * scales.k[kh];
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
                     : KC::zero();
      } else {
        reg[u] = (key < end)
                     ? *reinterpret_cast<const KV8*>(base + (long)key * ss)
                     : KC::zero();
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
      if constexpr (FP8) {
        kvc_cvt8_fp8(kreg[u], kf);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) kf[j] = ET::to_f32(kreg[u][j]);
      }
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
      if constexpr (FP8) {
        kvc_cvt8_fp8(vreg[u], vf);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = ET::to_f32(vreg[u][j]);
      }
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
  float o_scale = 1.f;   // FP8: v_scale[kh], once per normalised row
  if constexpr (FP8) o_scale = scales.v[kh];
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
    float on = (lsum > 0.f) ? o / lsum : 0.f;
    if constexpr (FP8) on *= o_scale;
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

// Contiguous: k / v are [b, cap, hk, d]. Paged: k / v are pools [num_pages,
// page_size, hk, d] and the strides handed to the kernel are the page and
// slot strides.
template <int D, int R, bool FP16, bool PAGED, bool FP8>
void launch_decode(const torch::Tensor& q, const torch::Tensor& k,
                   const torch::Tensor& v, const int* klp, torch::Tensor& o,
                   torch::Tensor& lse, float* o_part, float* lse_part,
                   float scale_log2, int wl, int num_splits, int groups,
                   hipStream_t stream, const KvcGeometry& geo,
                   DecScales<FP8> scales) {
  using KE = typename DecCache<FP8>::elem;
  const int b = q.size(0), hq = q.size(2);
  const int hk = k.size(2);
  dim3 grid(num_splits, hk * groups, b);
  hipLaunchKernelGGL((fa_decode_split_kernel<D, R, FP16, PAGED, FP8>), grid,
                     dim3(DEC_THREADS), 0, stream, (const short*)q.data_ptr(),
                     (const KE*)k.data_ptr(), (const KE*)v.data_ptr(), klp,
                     (short*)o.data_ptr(), lse.data_ptr<float>(), o_part,
                     lse_part, (int)geo.cap, hq, hk, (long)k.stride(0),
                     (long)k.stride(1), (long)v.stride(0), (long)v.stride(1),
                     scale_log2, wl, num_splits, geo.table, geo.page_shift,
                     geo.num_pages, scales);
  if (num_splits > 1) {
    hipLaunchKernelGGL((fa_decode_combine_kernel<D, FP16>), dim3(b * hq),
                       dim3(D), 0, stream, o_part, lse_part,
                       (short*)o.data_ptr(), lse.data_ptr<float>(),
                       num_splits);
  }
}

constexpr const char* DEC_OP = "fa_decode";

// All checks, the split choice, the workspace and the launches. hk =
// k_cache.size(2) in both layouts.
template <bool PAGED, bool FP8>
std::vector<torch::Tensor> run_decode(const torch::Tensor& q,
                                      const torch::Tensor& k_cache,
                                      const torch::Tensor& v_cache,
                                      const torch::Tensor& k_lens,
                                      const torch::Tensor& block_table,
                                      const torch::Tensor& k_scale,
                                      const torch::Tensor& v_scale,
                                      double softmax_scale, long wl,
                                      long num_splits) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.is_contiguous() &&
                  q.size(1) == 1,
              "fa_decode: q must be a contiguous GPU [b, 1, hq, d]");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 ||
                  q.scalar_type() == torch::kHalf,
              "fa_decode: bf16/fp16 only");
  kvc_check_cache(DEC_OP, k_cache, q, "k_cache", FP8);
  kvc_check_cache(DEC_OP, v_cache, q, "v_cache", FP8);
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "fa_decode: k_cache and v_cache shapes differ");
  const KvcGeometry geo = kvc_check_geometry(DEC_OP, q, k_cache, block_table);
  // without a table, absent lengths mean "every sequence is cap long"
  const int* klp = nullptr;
  if (PAGED || kvc_present(k_lens))
    klp = kvc_check_lens(DEC_OP, k_lens, q, "k_lens");
  DecScales<FP8> scales;
  if constexpr (FP8) {
    scales.k = kvc_check_scale(DEC_OP, k_scale, k_cache, "k_scale");
    scales.v = kvc_check_scale(DEC_OP, v_scale, v_cache, "v_scale");
  }

  const long b = q.size(0), hq = q.size(2), D = q.size(3);
  const long hk = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 128, "fa_decode: head_dim must be 64 or 128");
  TORCH_CHECK(hk > 0 && hq % hk == 0, "fa_decode: needs h_k | h_q");
  TORCH_CHECK(b >= 1 && b <= 65535);
  TORCH_CHECK(num_splits >= 0 && num_splits <= 65535,
              "fa_decode: num_splits must be in [0, 65535]");
  wl = std::min<long>(wl, 1L << 30);  // anything larger is "no window"

  const int rep = hq / hk;
  const int groups = (rep + DEC_MAX_ROWS - 1) / DEC_MAX_ROWS;
  TORCH_CHECK(hk * groups <= 65535);
  int ns = (int)num_splits;
  if (ns == 0)
    ns = choose_num_splits(
        (int)b, (int)hk * groups, (int)geo.cap,
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
                  (int)wl, ns, groups, stream, geo, scales))
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

}  // namespace

// block_table, k_scale and v_scale are optional: an undefined or empty 1-d
// tensor means absent (so does k_lens, without a table). With a table the
// caches are
// page pools. With scales (fp32 [hk] on the device, both or neither) they
// hold float8_e4m3fn codes: score = softmax_scale * k_scale[kh] * (q . K8),
// out = v_scale[kh] * sum p V8.
std::vector<torch::Tensor> fa_decode(torch::Tensor q, torch::Tensor k_cache,
                                     torch::Tensor v_cache,
                                     torch::Tensor k_lens,
                                     torch::Tensor block_table,
                                     torch::Tensor k_scale,
                                     torch::Tensor v_scale,
                                     double softmax_scale, long wl,
                                     long num_splits) {
  const bool fp8 = kvc_present(k_scale);
  TORCH_CHECK(fp8 == kvc_present(v_scale),
              "fa_decode: k_scale and v_scale come together");
  auto run = kvc_present(block_table)
                 ? (fp8 ? run_decode<true, true> : run_decode<true, false>)
                 : (fp8 ? run_decode<false, true> : run_decode<false, false>);
  return run(q, k_cache, v_cache, k_lens, block_table, k_scale, v_scale,
             softmax_scale, wl, num_splits);
}
