// kvcache.hip -- the small kernels around kvcache_split_kernel (kvcache_kernel.h): the append of
// new key / value rows to the cache and the combination of the key splits' partial results.
#include "kvcache_kernel.h"

namespace fa2 {

// One thread per 16-byte chunk of a new row: k_new[b, n, h] -> row `row` of slab `slab` of the
// cache (kvcache_append_pos.h), and V likewise.  (dtype-blind: 16-bit elements moved as raw bits.)
template <bool PAGED, typename Pages>
FA2_DEV void kvcache_append_rows(const fa2_kvcache_args& p, const Pages& pg) {
  constexpr int CW = 8;
#include "kvcache_append_pos.h"
  const uint16_t* ks = (const uint16_t*)p.k_new + b * p.k_new_stride[0] + n * p.k_new_stride[1] + h * p.k_new_stride[2] + 8 * c;
  const uint16_t* vs = (const uint16_t*)p.v_new + b * p.v_new_stride[0] + n * p.v_new_stride[1] + h * p.v_new_stride[2] + 8 * c;
  uint16_t* kd = (uint16_t*)p.k_cache + slab * p.k_cache_stride[0] + row * p.k_cache_stride[1] + h * p.k_cache_stride[2] + 8 * c;
  uint16_t* vd = (uint16_t*)p.v_cache + slab * p.v_cache_stride[0] + row * p.v_cache_stride[1] + h * p.v_cache_stride[2] + 8 * c;
  const u32x4 kv = *(const u32x4*)ks, vv = *(const u32x4*)vs;
  *(u32x4*)kd = kv;
  *(u32x4*)vd = vv;
}

// contiguous cache [B, capacity, Hkv, D] / pools of blocks behind a block table
__global__ void __launch_bounds__(256) kvcache_append_kernel(const fa2_kvcache_args p) { kvcache_append_rows<false>(p, KvNoPages{}); }
__global__ void __launch_bounds__(256) kvcache_paged_append_kernel(const fa2_paged_kvcache_args pp) { kvcache_append_rows<true>(pp.base, pp); }

// Per output row (b, h, i), 64 threads (4 columns each), 4 rows per workgroup:
//   m = max_s lse_s,  w_s = 2^(lse_s - m),  O = sum_s w_s O_s / sum_s w_s,  LSE2 = m + log2 sum_s w_s
// summed in split order.  A split with lse_s = -inf (no visible key) has weight 0 and its partial O
// is not read into the sum; all -inf gives O = 0, LSE2 = -inf.
template <bool BF16>
__global__ void __launch_bounds__(256) kvcache_combine_kernel(const fa2_kvcache_args p, const int nsplit) {
  using E = Elem<BF16>;
  const int D = p.head_dim, Sq = p.seqlen_q, Hq = p.heads_q;
  const int64_t nrow = (int64_t)p.batch * Hq * Sq;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrow) return;
  const int d0 = 4 * (threadIdx.x & 63);
  const float* ws_o = (const float*)p.workspace;
  const float* ws_l = ws_o + (int64_t)nsplit * nrow * D;
  float m = kNegInf;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, ws_l[s * nrow + row]);
  float sum = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const float l = ws_l[s * nrow + row];
    const float w = l == kNegInf ? 0.f : __builtin_amdgcn_exp2f(l - m);
    sum += w;
    if (w > 0.f && d0 < D) o += *(const f32x4*)(ws_o + (s * nrow + row) * D + d0) * w;
  }
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  o *= inv;
  const int i = (int)(row % Sq), h = (int)((row / Sq) % Hq), b = (int)(row / ((int64_t)Sq * Hq));
  if (d0 < D) {
    uint16_t* orow = (uint16_t*)p.o + b * p.o_stride[0] + i * p.o_stride[1] + h * p.o_stride[2];
    *(u32x2*)(orow + d0) = u32x2{E::pack2(o[0], o[1]), E::pack2(o[2], o[3])};
  }
  if ((threadIdx.x & 63) == 0 && p.lse) p.lse[row] = sum > 0.f ? m + __builtin_amdgcn_logf(sum) : kNegInf;
}

template <typename Args>
hipError_t launch_kvcache_append(const Args& args, hipStream_t st) {
  const fa2_kvcache_args& a = kv_base(args);
  const int64_t total = (int64_t)a.batch * a.seqlen_new * a.heads_kv * (a.head_dim >> 3);
  if (total <= 0) return hipSuccess;
  const dim3 grid((unsigned)((total + 255) / 256));
  if constexpr (std::is_same_v<Args, fa2_paged_kvcache_args>) hipLaunchKernelGGL(kvcache_paged_append_kernel, grid, dim3(256), 0, st, args);
  else hipLaunchKernelGGL(kvcache_append_kernel, grid, dim3(256), 0, st, args);
  return hipGetLastError();
}
template hipError_t launch_kvcache_append(const fa2_kvcache_args&, hipStream_t);
template hipError_t launch_kvcache_append(const fa2_paged_kvcache_args&, hipStream_t);

hipError_t launch_kvcache_combine(const fa2_kvcache_args& a, int nsplit, hipStream_t st) {
  const int64_t nrow = (int64_t)a.batch * a.heads_q * a.seqlen_q;
  const dim3 grid((unsigned)((nrow + 3) / 4));
  if (a.dtype == FA2_BF16) hipLaunchKernelGGL((kvcache_combine_kernel<true>), grid, dim3(256), 0, st, a, nsplit);
  else hipLaunchKernelGGL((kvcache_combine_kernel<false>), grid, dim3(256), 0, st, a, nsplit);
  return hipGetLastError();
}

}  // namespace fa2
