// Quantising KV-cache write, gfx950: new K and V rows (bf16/fp16) go into
// float8_e4m3fn caches at given flat slots, one launch for K and V together.
//
//   code = rne_e4m3(clamp(x * (1 / scale[head]), -448, 448))
//
// The clamp runs in fp32 before the conversion, so a finite input saturates
// at +-448 and never becomes the NaN code; the reciprocal is an IEEE fp32
// division (no fast-math in this build). v_cvt_pk_fp8_f32 is the OCP e4m3fn
// round-to-nearest-even conversion of gfx950, two elements per instruction.
//
// The cache is [n0, n1, hk, d] with dense [hk][d] and arbitrary (64-bit)
// strides for dims 0 and 1, which covers a contiguous cache [b, cap, hk, d]
// and a page pool [num_pages, page_size, hk, d] alike. Flat slot t names
// [t / n1][t % n1]; a slot outside [0, n0 * n1) is skipped. Two tokens with
// the same slot race (unspecified which one lands).
//
// One thread converts 8 elements: a 16-byte load, four conversions, an
// 8-byte store. blockIdx.y picks K or V.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "attn_common.h"

namespace {

constexpr int KVW_THREADS = 256;
constexpr float E4M3_MAX = 448.f;

struct KvwSide {
  const short* src;       // [b, s, hk, d], strides sb / ss in elements
  unsigned char* cache;   // [n0, n1, hk, d], strides c0 / c1 in bytes
  const float* scale;     // [hk]
  long sb, ss, c0, c1;
};

template <bool FP16, typename IDX>
__global__ __launch_bounds__(KVW_THREADS)
void kv_cache_write_fp8_kernel(KvwSide kside, KvwSide vside,
                               const IDX* __restrict__ slots, long n_tok,
                               int s, int hk, int d, long n0, long n1) {
  using ET = AttnElem<FP16>;
  const KvwSide sd = blockIdx.y == 0 ? kside : vside;   // uniform select
  const int cpr = (hk * d) >> 3;   // 8-element chunks per token row
  const long total = n_tok * cpr;
  for (long i = (long)blockIdx.x * KVW_THREADS + threadIdx.x; i < total;
       i += (long)gridDim.x * KVW_THREADS) {
    const long tok = i / cpr;
    const int e = (int)(i - tok * cpr) << 3;   // element offset in [hk][d]
    const long slot = (long)slots[tok];
    if (slot < 0 || slot >= n0 * n1) continue;
    const long bi = tok / s, si = tok - bi * s;
    const s16x8 x = *reinterpret_cast<const s16x8*>(sd.src + bi * sd.sb +
                                                    si * sd.ss + e);
    const float inv = 1.0f / sd.scale[e / d];
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = ET::to_f32(x[j]) * inv;
      // NaN stays NaN (the comparison-based clamp would turn it into -448)
      f[j] = (y != y) ? y : fminf(fmaxf(y, -E4M3_MAX), E4M3_MAX);
    }
    u32x2 out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      int p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w], f[4 * w + 1], 0,
                                              false);
      p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2], f[4 * w + 3], p,
                                          true);
      out[w] = (unsigned)p;
    }
    const long p0 = slot / n1, p1 = slot - p0 * n1;
    *reinterpret_cast<u32x2*>(sd.cache + p0 * sd.c0 + p1 * sd.c1 + e) = out;
  }
}

KvwSide make_side(const torch::Tensor& x, const torch::Tensor& cache,
                  const torch::Tensor& scale, const char* name) {
  const long hk = x.size(2), d = x.size(3);
  TORCH_CHECK(x.stride(3) == 1 && x.stride(2) == d, "kv_cache_write_fp8: ",
              name, " needs dense [heads][head_dim]");
  // 16-byte loads of two-byte elements
  TORCH_CHECK(x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "kv_cache_write_fp8: ", name, " rows must be 16-byte aligned");
  TORCH_CHECK(cache.is_cuda() && cache.dim() == 4 &&
                  cache.scalar_type() == torch::kFloat8_e4m3fn &&
                  cache.size(2) == hk && cache.size(3) == d &&
                  cache.device() == x.device(),
              "kv_cache_write_fp8: ", name,
              "_cache must be a GPU float8_e4m3fn [n0, n1, hk, d]");
  TORCH_CHECK(cache.stride(3) == 1 && cache.stride(2) == d,
              "kv_cache_write_fp8: ", name,
              "_cache needs dense [heads][head_dim]");
  // 8-byte stores of one-byte elements: strides are bytes here
  TORCH_CHECK(cache.stride(0) % 8 == 0 && cache.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(cache.data_ptr()) % 8 == 0,
              "kv_cache_write_fp8: ", name,
              "_cache rows must be 8-byte aligned");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
                  scale.dim() == 1 && scale.size(0) == hk &&
                  scale.is_contiguous() && scale.device() == x.device(),
              "kv_cache_write_fp8: ", name, "_scale must be a GPU fp32 [hk]");
  return KvwSide{(const short*)x.data_ptr(),
                 (unsigned char*)cache.data_ptr(),
                 scale.data_ptr<float>(),
                 (long)x.stride(0), (long)x.stride(1),
                 (long)cache.stride(0), (long)cache.stride(1)};
}

}  // namespace

void kv_cache_write_fp8(torch::Tensor k, torch::Tensor v,
                        torch::Tensor k_cache, torch::Tensor v_cache,
                        torch::Tensor slots, torch::Tensor k_scale,
                        torch::Tensor v_scale) {
  TORCH_CHECK(k.is_cuda() && k.dim() == 4 && v.is_cuda() &&
                  v.device() == k.device() && v.sizes() == k.sizes() &&
                  v.scalar_type() == k.scalar_type(),
              "kv_cache_write_fp8: k and v must be GPU [b, s, hk, d] of one "
              "shape and dtype");
  TORCH_CHECK(k.scalar_type() == torch::kBFloat16 ||
                  k.scalar_type() == torch::kHalf,
              "kv_cache_write_fp8: bf16/fp16 only");
  const long b = k.size(0), s = k.size(1), hk = k.size(2), d = k.size(3);
  TORCH_CHECK(d % 8 == 0 && hk >= 1 && hk * d <= (1L << 30),
              "kv_cache_write_fp8: head_dim must be a multiple of 8");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4 &&
                  k_cache.sizes() == v_cache.sizes(),
              "kv_cache_write_fp8: k_cache and v_cache shapes differ");
  TORCH_CHECK(slots.is_cuda() && slots.device() == k.device() &&
                  slots.dim() == 1 && slots.size(0) == b * s &&
                  slots.is_contiguous() &&
                  (slots.scalar_type() == torch::kInt32 ||
                   slots.scalar_type() == torch::kInt64),
              "kv_cache_write_fp8: slots must be a contiguous GPU int32 / "
              "int64 [b * s]");
  const long n_tok = b * s;
  if (n_tok == 0) return;
  TORCH_CHECK(s <= INT_MAX);
  const KvwSide ks = make_side(k, k_cache, k_scale, "k");
  const KvwSide vs = make_side(v, v_cache, v_scale, "v");
  const long n0 = k_cache.size(0), n1 = k_cache.size(1);
  const long work = n_tok * (hk * d / 8);
  const long blocks =
      std::min<long>((work + KVW_THREADS - 1) / KVW_THREADS, 2048);
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((unsigned)blocks, 2);
#define KVW_LAUNCH(IDX)                                                      \
  FP16_SWITCH(k.scalar_type() == torch::kHalf,                               \
              hipLaunchKernelGGL((kv_cache_write_fp8_kernel<kFP16, IDX>),    \
                                 grid, dim3(KVW_THREADS), 0, stream, ks, vs, \
                                 (const IDX*)slots.data_ptr(), n_tok,        \
                                 (int)s, (int)hk, (int)d, n0, n1))
  if (slots.scalar_type() == torch::kInt32) KVW_LAUNCH(int);
  else KVW_LAUNCH(long);
#undef KVW_LAUNCH
  HIP_CHECK_LAST();
}
