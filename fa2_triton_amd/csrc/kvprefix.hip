// kvprefix.hip -- the merge of shared-prefix (cascade) decode attention (fa2_fwd_kvcache_prefix,
// DESIGN 15).  The two attention passes are the split kernels of kvcache_kernel.h, unchanged: the
// prefix pass on batch 1 with B * Sq query rows, the sequence pass as fa2_fwd_kvcache runs it, both
// on their workspace path.  This kernel sums their fp32 partial results.
#include "common.h"
#include "fa2_internal.h"

namespace fa2 {

// Per output row (b, h, i), 64 threads (4 columns each), 4 rows per workgroup, as
// kvcache_combine_kernel (kvcache.hip) and with its expressions:
//   m = max_s lse_s,  w_s = 2^(lse_s - m),  O = sum_s w_s O_s / sum_s w_s,  LSE2 = m + log2 sum_s w_s
// over the ns_p prefix splits, then the ns_s sequence splits, in that order.  The prefix pass saw
// the batch as B * Sq query positions of one batch row, so its partials of row (b, h, i) lie at row
// (h * B + b) * Sq + i; the sequence pass's at (b * Hq + h) * Sq + i.  A split with lse_s = -inf has
// weight 0 and its partial O is not read; all -inf gives O = 0, LSE2 = -inf.
template <bool BF16>
__global__ void __launch_bounds__(256) kvprefix_merge_kernel(const fa2_kvcache_args p, const float* ws_p, const int ns_p,
                                                             const float* ws_s, const int ns_s) {
  using E = Elem<BF16>;
  const int D = p.head_dim, Sq = p.seqlen_q, Hq = p.heads_q;
  const int64_t nrow = (int64_t)p.batch * Hq * Sq;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrow) return;
  const int d0 = 4 * (threadIdx.x & 63);
  const int i = (int)(row % Sq), h = (int)((row / Sq) % Hq), b = (int)(row / ((int64_t)Sq * Hq));
  const int64_t prow = ((int64_t)h * p.batch + b) * Sq + i;
  const float* pl = ws_p + (int64_t)ns_p * nrow * D;
  const float* sl = ws_s + (int64_t)ns_s * nrow * D;
  float m = kNegInf;
  for (int s = 0; s < ns_p; ++s) m = fmaxf(m, pl[s * nrow + prow]);
  for (int s = 0; s < ns_s; ++s) m = fmaxf(m, sl[s * nrow + row]);
  float sum = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < ns_p; ++s) {
    const float l = pl[s * nrow + prow];
    const float w = l == kNegInf ? 0.f : __builtin_amdgcn_exp2f(l - m);
    sum += w;
    if (w > 0.f && d0 < D) o += *(const f32x4*)(ws_p + (s * nrow + prow) * D + d0) * w;
  }
  for (int s = 0; s < ns_s; ++s) {
    const float l = sl[s * nrow + row];
    const float w = l == kNegInf ? 0.f : __builtin_amdgcn_exp2f(l - m);
    sum += w;
    if (w > 0.f && d0 < D) o += *(const f32x4*)(ws_s + (s * nrow + row) * D + d0) * w;
  }
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  o *= inv;
  if (d0 < D) {
    uint16_t* orow = (uint16_t*)p.o + b * p.o_stride[0] + i * p.o_stride[1] + h * p.o_stride[2];
    *(u32x2*)(orow + d0) = u32x2{E::pack2(o[0], o[1]), E::pack2(o[2], o[3])};
  }
  if ((threadIdx.x & 63) == 0 && p.lse) p.lse[row] = sum > 0.f ? m + __builtin_amdgcn_logf(sum) : kNegInf;
}

hipError_t launch_kvprefix_merge(const fa2_kvcache_args& a, const float* ws_p, int ns_p, const float* ws_s, int ns_s,
                                 hipStream_t st) {
  const int64_t nrow = (int64_t)a.batch * a.heads_q * a.seqlen_q;
  const dim3 grid((unsigned)((nrow + 3) / 4));
  if (a.dtype == FA2_BF16) hipLaunchKernelGGL((kvprefix_merge_kernel<true>), grid, dim3(256), 0, st, a, ws_p, ns_p, ws_s, ns_s);
  else hipLaunchKernelGGL((kvprefix_merge_kernel<false>), grid, dim3(256), 0, st, a, ws_p, ns_p, ws_s, ns_s);
  return hipGetLastError();
}

}  // namespace fa2
