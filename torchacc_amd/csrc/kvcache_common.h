// What the KV-cache attention kernels share (flash_attn_decode.hip,
// flash_attn_kvcache_mq.hip): the e4m3 -> fp32 conversion of the 8 codes a
// lane loads at once, and the host-side checks of the caches, lengths, scales
// and paged geometry. Every check takes the op's name for its message. They
// are shape-only (no host sync) and run before anything is dereferenced.
#pragma once

#include <torch/extension.h>
#include "common.h"

// 8 e4m3 codes as fp32 (v_cvt_pk_f32_fp8, two elements each)
DEVINLINE void kvc_cvt8_fp8(const u32x2& r, float* f) {
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

// An undefined tensor or the empty 1-d tensor stands for an absent optional
// argument. An empty tensor of another rank (a [b, 0] block table) is a
// present, invalid argument and is refused by the checks below.
inline bool kvc_present(const torch::Tensor& t) {
  return t.defined() && !(t.dim() == 1 && t.numel() == 0);
}

// A cache [n0, n1, hk, d] on q's device with dense [hk][d], q's head_dim and
// rows aligned for the kernels' 16-byte (fp8: 8-byte) loads.
inline void kvc_check_cache(const char* op, const torch::Tensor& c,
                            const torch::Tensor& q, const char* name,
                            bool fp8) {
  TORCH_CHECK(c.is_cuda() && c.dim() == 4 && c.device() == q.device(), op,
              ": ", name, " must be a 4-d tensor on q's GPU");
  TORCH_CHECK(c.stride(3) == 1 && c.stride(2) == c.size(3), op, ": ", name,
              " needs dense [heads][head_dim]");
  TORCH_CHECK(c.size(3) == q.size(3), op, ": ", name,
              " and q disagree on head_dim");
  if (fp8) {
    TORCH_CHECK(c.scalar_type() == torch::kFloat8_e4m3fn, op, ": ", name,
                " must be float8_e4m3fn");
    // 8-byte loads of one-byte elements: strides are bytes here
    TORCH_CHECK(c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(c.data_ptr()) % 8 == 0,
                op, ": ", name, " rows must be 8-byte aligned");
    return;
  }
  TORCH_CHECK(c.scalar_type() == q.scalar_type(), op, ": ", name,
              " must have q's dtype");
  // 16-byte loads
  TORCH_CHECK(c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 == 0,
              op, ": ", name, " rows must be 16-byte aligned");
}

inline const int* kvc_check_lens(const char* op, const torch::Tensor& lens,
                                 const torch::Tensor& q, const char* name) {
  TORCH_CHECK(lens.is_cuda() && lens.device() == q.device() &&
                  lens.scalar_type() == torch::kInt32 && lens.dim() == 1 &&
                  lens.size(0) == q.size(0) && lens.is_contiguous(),
              op, ": ", name, " must be an int32 [b] on q's GPU");
  return lens.data_ptr<int>();
}

// fp8 caches: one fp32 scale per kv head, read by the kernel. `cache` has
// passed kvc_check_cache.
inline const float* kvc_check_scale(const char* op, const torch::Tensor& s,
                                    const torch::Tensor& cache,
                                    const char* name) {
  TORCH_CHECK(s.is_cuda() && s.scalar_type() == torch::kFloat32 &&
                  s.dim() == 1 && s.size(0) == cache.size(2) &&
                  s.is_contiguous() && s.device() == cache.device(),
              op, ": ", name, " must be a GPU fp32 [hk]");
  return s.data_ptr<float>();
}

// Contiguous: the caches are [b, cap, hk, d], table is null. Paged: they are
// pools [num_pages, page_size, hk, d] and block_table is an int32 [b,
// table_width]; cap = table_width * page_size. The table's contents are never
// read on the host (the kernels clamp every entry they dereference).
struct KvcGeometry {
  long cap;
  const int* table;
  int page_shift;
  int num_pages;
};

inline KvcGeometry kvc_check_geometry(const char* op, const torch::Tensor& q,
                                      const torch::Tensor& k_cache,
                                      const torch::Tensor& block_table) {
  const long b = q.size(0);
  if (!kvc_present(block_table)) {
    TORCH_CHECK(k_cache.size(0) == b, op,
                ": cache and q disagree on the batch");
    const long cap = k_cache.size(1);
    TORCH_CHECK(cap >= 1 && cap <= (1L << 30), op,
                ": the cache needs 1..2^30 slots per sequence");
    return {cap, nullptr, 0, 0};
  }
  const long num_pages = k_cache.size(0), ps = k_cache.size(1);
  TORCH_CHECK(num_pages >= 1 && num_pages <= (1L << 30), op,
              ": the pool needs 1..2^30 pages");
  TORCH_CHECK(ps >= 16 && (ps & (ps - 1)) == 0, op,
              ": page_size must be a power of two >= 16, got ", ps);
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == q.device() &&
                  block_table.scalar_type() == torch::kInt32 &&
                  block_table.dim() == 2 && block_table.size(0) == b &&
                  block_table.is_contiguous(),
              op, ": block_table must be a contiguous int32 [b, table_width] "
              "on q's GPU");
  const long tw = block_table.size(1);
  TORCH_CHECK(tw >= 1 && tw * ps <= (1L << 30), op,
              ": table_width * page_size must be in [1, 2^30]");
  int shift = 0;
  while ((1L << shift) < ps) ++shift;
  return {tw * ps, block_table.data_ptr<int>(), shift, (int)num_pages};
}
