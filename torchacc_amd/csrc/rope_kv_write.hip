// Fused RoPE + KV-cache write at per-token positions, gfx950: one launch
// rotates q into a fresh tensor, rotates k straight into its cache slot and
// copies (or quantises) v into its slot.
//
//   p = positions[t]; p outside [0, P): q_rot[t] = 0, nothing written
//   q_rot[t]          = rope(q[t], cos[p], sin[p])
//   k_cache[slots[t]] = rope(k[t], cos[p], sin[p])     (slot in range only)
//   v_cache[slots[t]] = v[t]
//
// The rotation is rope_kernel's (elementwise.hip): neox half-split, fp32,
// one rounding to the element type; the fp32 expressions below are kept
// textually those of rope_kernel so that FMA contraction gives the same
// bits. A float8_e4m3fn cache takes the rotated K rounded to the 16-bit
// type first and then kv_cache_write_fp8_kernel's quantisation
// (kv_cache_write.hip), again with its expressions, so the op equals
// rope_forward followed by index_copy_ / kv_cache_write_fp8 bit for bit.
//
// Caches are [n0, n1, hk, d] with dense [hk][d] and arbitrary 64-bit strides
// for dims 0 and 1, flat slot t -> [t / n1][t % n1], as in
// kv_cache_write.hip. blockIdx.y picks the section: 0 = q, 1 = k, 2 = v. A
// q / k thread owns 8 first-half and the 8 matching second-half elements of
// one head (two 16-byte loads, two 16-byte stores, or two 8-byte stores of
// fp8 codes); a v thread owns 8 elements. No LDS, no workspace; positions
// and slots are read on the device, so a captured launch follows them.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "attn_common.h"

namespace {

constexpr int RKW_THREADS = 256;
constexpr float E4M3_MAX = 448.f;

struct RkwArgs {
  const short* q;          // [b, s, hq, d], strides qb / qs in elements
  const short* k;          // [b, s, hk, d]
  const short* v;
  short* q_rot;            // [b, s, hq, d] contiguous
  unsigned char* k_cache;  // [n0, n1, hk, d], strides in BYTES
  unsigned char* v_cache;
  const float* cosp;       // [P, d / 2]
  const float* sinp;
  const float* k_scale;    // [hk], fp8 caches only
  const float* v_scale;
  long qb, qs, kb, ks, vb, vs;
  long kc0, kc1, vc0, vc1;
  long n_tok, n0, n1, P;
  int s, hq, hk, d;
};

// kv_cache_write_fp8_kernel's conversion of 8 fp32 values
DEVINLINE u32x2 rkw_quant8(const float* y) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    // NaN stays NaN (the comparison-based clamp would turn it into -448)
    f[j] = (y[j] != y[j]) ? y[j] : fminf(fmaxf(y[j], -E4M3_MAX), E4M3_MAX);
  u32x2 out;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w], f[4 * w + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2], f[4 * w + 3], p, true);
    out[w] = (unsigned)p;
  }
  return out;
}

template <bool FP16, bool FP8, typename IDX>
__global__ __launch_bounds__(RKW_THREADS)
void rope_kv_cache_write_kernel(RkwArgs g, const IDX* __restrict__ positions,
                                const IDX* __restrict__ slots) {
  using ET = AttnElem<FP16>;
  const int sec = blockIdx.y;   // uniform
  const long start = (long)blockIdx.x * RKW_THREADS + threadIdx.x;
  const long step = (long)gridDim.x * RKW_THREADS;
  const int d = g.d;
  if (sec == 2) {
    // ---- v: copy or quantise, 8 elements per thread ----------------------
    const int cpr = (g.hk * d) >> 3;
    const long total = g.n_tok * cpr;
    for (long i = start; i < total; i += step) {
      const long tok = i / cpr;
      const int e = (int)(i - tok * cpr) << 3;   // element offset in [hk][d]
      const long p = (long)positions[tok];
      const long slot = (long)slots[tok];
      if (p < 0 || p >= g.P || slot < 0 || slot >= g.n0 * g.n1) continue;
      const long bi = tok / g.s, si = tok - bi * g.s;
      const s16x8 x =
          *reinterpret_cast<const s16x8*>(g.v + bi * g.vb + si * g.vs + e);
      const long p0 = slot / g.n1, p1 = slot - p0 * g.n1;
      unsigned char* dst = g.v_cache + p0 * g.vc0 + p1 * g.vc1;
      if constexpr (FP8) {
        const float inv = 1.0f / g.v_scale[e / d];
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = ET::to_f32(x[j]) * inv;
        *reinterpret_cast<u32x2*>(dst + e) = rkw_quant8(y);
      } else {
        *reinterpret_cast<s16x8*>(dst + 2L * e) = x;
      }
    }
    return;
  }
  // ---- q / k: rotate 8 + 8 elements of one head ----------------------------
  const bool isk = sec == 1;
  const int H = isk ? g.hk : g.hq;
  const int d2 = d / 2;
  const int chunks = d2 / 8;   // d2 multiple of 8
  const short* src = isk ? g.k : g.q;
  const long sb = isk ? g.kb : g.qb, ss = isk ? g.ks : g.qs;
  const long n = g.n_tok * H * chunks;
  for (long idx = start; idx < n; idx += step) {
    const long rowhead = idx / chunks;   // (tok * H + head)
    const int c = (int)(idx - rowhead * chunks);
    const long tok = rowhead / H;
    const int head = (int)(rowhead - tok * H);
    const long p = (long)positions[tok];
    const bool real = p >= 0 && p < g.P;
    long slot = 0;
    if (isk) {
      slot = (long)slots[tok];
      if (!real || slot < 0 || slot >= g.n0 * g.n1) continue;
    } else if (!real) {
      short* orow = g.q_rot + rowhead * d + c * 8;
      const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<s16x8*>(orow) = z;
      *reinterpret_cast<s16x8*>(orow + d2) = z;
      continue;
    }
    const long bi = tok / g.s, si = tok - bi * g.s;
    const short* xr = src + bi * sb + si * ss + head * d + c * 8;
    const float* cp = g.cosp + p * d2 + c * 8;
    const float* sp = g.sinp + p * d2 + c * 8;
    s16x8 x1 = *reinterpret_cast<const s16x8*>(xr);
    s16x8 x2 = *reinterpret_cast<const s16x8*>(xr + d2);
    f32x4 c0 = *reinterpret_cast<const f32x4*>(cp);
    f32x4 c1 = *reinterpret_cast<const f32x4*>(cp + 4);
    f32x4 s0 = *reinterpret_cast<const f32x4*>(sp);
    f32x4 s1 = *reinterpret_cast<const f32x4*>(sp + 4);
    s16x8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float cj = j < 4 ? c0[j] : c1[j - 4];
      float sj = j < 4 ? s0[j] : s1[j - 4];
      float a = AttnElem<FP16>::to_f32(x1[j]);
      float b = AttnElem<FP16>::to_f32(x2[j]);
      o1[j] = AttnElem<FP16>::from_f32(a * cj - b * sj);
      o2[j] = AttnElem<FP16>::from_f32(b * cj + a * sj);
    }
    if (!isk) {
      short* orow = g.q_rot + rowhead * d + c * 8;
      *reinterpret_cast<s16x8*>(orow) = o1;
      *reinterpret_cast<s16x8*>(orow + d2) = o2;
      continue;
    }
    const long p0 = slot / g.n1, p1 = slot - p0 * g.n1;
    unsigned char* dst = g.k_cache + p0 * g.kc0 + p1 * g.kc1;
    const int e = head * d + c * 8;   // element offset in [hk][d]
    if constexpr (FP8) {
      // the rotated value, already rounded to the 16-bit type, is quantised
      const float inv = 1.0f / g.k_scale[head];
      float y1[8], y2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        y1[j] = ET::to_f32(o1[j]) * inv;
        y2[j] = ET::to_f32(o2[j]) * inv;
      }
      *reinterpret_cast<u32x2*>(dst + e) = rkw_quant8(y1);
      *reinterpret_cast<u32x2*>(dst + e + d2) = rkw_quant8(y2);
    } else {
      *reinterpret_cast<s16x8*>(dst + 2L * e) = o1;
      *reinterpret_cast<s16x8*>(dst + 2L * (e + d2)) = o2;
    }
  }
}

void check_rows(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.stride(3) == 1 && x.stride(2) == x.size(3),
              "rope_kv_cache_write: ", name,
              " needs dense [heads][head_dim]");
  // 16-byte loads of two-byte elements
  TORCH_CHECK(x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "rope_kv_cache_write: ", name, " rows must be 16-byte aligned");
}

void check_cache(const torch::Tensor& cache, const torch::Tensor& k, bool fp8,
                 const char* name) {
  TORCH_CHECK(cache.is_cuda() && cache.dim() == 4 &&
                  cache.device() == k.device() &&
                  cache.size(2) == k.size(2) && cache.size(3) == k.size(3),
              "rope_kv_cache_write: ", name,
              " must be a GPU [n0, n1, hk, d] on k's device");
  TORCH_CHECK(cache.scalar_type() ==
                  (fp8 ? torch::kFloat8_e4m3fn : k.scalar_type()),
              "rope_kv_cache_write: k_cache and v_cache must both have k's "
              "dtype or both be float8_e4m3fn");
  TORCH_CHECK(cache.stride(3) == 1 && cache.stride(2) == cache.size(3),
              "rope_kv_cache_write: ", name,
              " needs dense [heads][head_dim]");
  // 16-byte stores of 16-bit elements, 8-byte stores of fp8 codes: both are
  // 8 elements
  const uintptr_t bytes = fp8 ? 8 : 16;
  TORCH_CHECK(cache.stride(0) % 8 == 0 && cache.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(cache.data_ptr()) % bytes == 0,
              "rope_kv_cache_write: ", name, " rows must be ", bytes,
              "-byte aligned");
}

void check_scale(const torch::Tensor& scale, const torch::Tensor& k,
                 const char* name) {
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
                  scale.dim() == 1 && scale.size(0) == k.size(2) &&
                  scale.is_contiguous() && scale.device() == k.device(),
              "rope_kv_cache_write: ", name, " must be a GPU fp32 [hk]");
}

void check_index(const torch::Tensor& t, const torch::Tensor& k, long n_tok,
                 const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == k.device() && t.dim() == 1 &&
                  t.size(0) == n_tok && t.is_contiguous() &&
                  (t.scalar_type() == torch::kInt32 ||
                   t.scalar_type() == torch::kInt64),
              "rope_kv_cache_write: ", name,
              " must be a contiguous GPU int32 / int64 [b * s]");
}

}  // namespace

// k_scale / v_scale: empty 1-d = absent
torch::Tensor rope_kv_cache_write(torch::Tensor q, torch::Tensor k,
                                  torch::Tensor v, torch::Tensor cos,
                                  torch::Tensor sin, torch::Tensor positions,
                                  torch::Tensor k_cache,
                                  torch::Tensor v_cache, torch::Tensor slots,
                                  torch::Tensor k_scale,
                                  torch::Tensor v_scale) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && k.is_cuda() && k.dim() == 4 &&
                  v.is_cuda() && k.device() == q.device() &&
                  v.device() == q.device(),
              "rope_kv_cache_write: q, k and v must be 4-d on one GPU");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 ||
                  q.scalar_type() == torch::kHalf,
              "rope_kv_cache_write: bf16/fp16 only");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() &&
                  v.scalar_type() == q.scalar_type(),
              "rope_kv_cache_write: q, k and v must share one dtype");
  const long b = q.size(0), s = q.size(1), hq = q.size(2), d = q.size(3);
  const long hk = k.size(2);
  TORCH_CHECK(k.size(0) == b && k.size(1) == s && k.size(3) == d &&
                  v.sizes() == k.sizes(),
              "rope_kv_cache_write: q [b, s, hq, d] and k, v [b, s, hk, d] "
              "disagree");
  TORCH_CHECK(d % 16 == 0 && hq >= 1 && hk >= 1 && hq * d <= (1L << 30) &&
                  hk * d <= (1L << 30),
              "rope_kv_cache_write: head_dim must be a multiple of 16");
  check_rows(q, "q");
  check_rows(k, "k");
  check_rows(v, "v");
  TORCH_CHECK(cos.is_cuda() && sin.is_cuda() && cos.device() == q.device() &&
                  sin.device() == q.device() &&
                  cos.scalar_type() == torch::kFloat32 &&
                  sin.scalar_type() == torch::kFloat32 && cos.dim() == 2 &&
                  cos.size(1) == d / 2 && sin.sizes() == cos.sizes() &&
                  cos.is_contiguous() && sin.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(cos.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(sin.data_ptr()) % 16 == 0,
              "rope_kv_cache_write: cos and sin must be contiguous GPU fp32 "
              "[P, d / 2] tables on q's device");
  const long P = cos.size(0);
  TORCH_CHECK(P >= 1, "rope_kv_cache_write: cos and sin need P >= 1 rows");
  const long n_tok = b * s;
  check_index(positions, k, n_tok, "positions");
  check_index(slots, k, n_tok, "slots");
  TORCH_CHECK(positions.scalar_type() == slots.scalar_type(),
              "rope_kv_cache_write: positions and slots must share one "
              "integer dtype");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4 &&
                  k_cache.sizes() == v_cache.sizes(),
              "rope_kv_cache_write: k_cache and v_cache shapes differ");
  const bool fp8 = k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  check_cache(k_cache, k, fp8, "k_cache");
  check_cache(v_cache, k, fp8, "v_cache");
  if (fp8) {
    check_scale(k_scale, k, "k_scale");
    check_scale(v_scale, k, "v_scale");
  } else {
    TORCH_CHECK(k_scale.numel() == 0 && v_scale.numel() == 0,
                "rope_kv_cache_write: k_scale / v_scale apply to "
                "float8_e4m3fn caches only");
  }
  auto q_rot = torch::empty({b, s, hq, d}, q.options());
  if (n_tok == 0) return q_rot;
  TORCH_CHECK(s <= INT_MAX);
  const long esz = fp8 ? 1 : 2;   // cache strides go to the kernel in bytes
  RkwArgs g;
  g.q = (const short*)q.data_ptr();
  g.k = (const short*)k.data_ptr();
  g.v = (const short*)v.data_ptr();
  g.q_rot = (short*)q_rot.data_ptr();
  g.k_cache = (unsigned char*)k_cache.data_ptr();
  g.v_cache = (unsigned char*)v_cache.data_ptr();
  g.cosp = cos.data_ptr<float>();
  g.sinp = sin.data_ptr<float>();
  g.k_scale = fp8 ? k_scale.data_ptr<float>() : nullptr;
  g.v_scale = fp8 ? v_scale.data_ptr<float>() : nullptr;
  g.qb = q.stride(0); g.qs = q.stride(1);
  g.kb = k.stride(0); g.ks = k.stride(1);
  g.vb = v.stride(0); g.vs = v.stride(1);
  g.kc0 = k_cache.stride(0) * esz; g.kc1 = k_cache.stride(1) * esz;
  g.vc0 = v_cache.stride(0) * esz; g.vc1 = v_cache.stride(1) * esz;
  g.n_tok = n_tok; g.n0 = k_cache.size(0); g.n1 = k_cache.size(1); g.P = P;
  g.s = (int)s; g.hq = (int)hq; g.hk = (int)hk; g.d = (int)d;
  // the largest section sizes the grid; the others leave their loop early
  const long work = n_tok * std::max(hq * (d / 16), hk * (d / 8));
  const long blocks =
      std::min<long>((work + RKW_THREADS - 1) / RKW_THREADS, 2048);
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((unsigned)blocks, 3);
#define RKW_LAUNCH(FP8, IDX)                                                 \
  FP16_SWITCH(q.scalar_type() == torch::kHalf,                               \
              hipLaunchKernelGGL(                                            \
                  (rope_kv_cache_write_kernel<kFP16, FP8, IDX>), grid,       \
                  dim3(RKW_THREADS), 0, stream, g,                           \
                  (const IDX*)positions.data_ptr(),                          \
                  (const IDX*)slots.data_ptr()))
  const bool i32 = slots.scalar_type() == torch::kInt32;
  if (fp8 && i32) RKW_LAUNCH(true, int);
  else if (fp8) RKW_LAUNCH(true, long);
  else if (i32) RKW_LAUNCH(false, int);
  else RKW_LAUNCH(false, long);
#undef RKW_LAUNCH
  HIP_CHECK_LAST();
  return q_rot;
}
