// kvcache_fp8.hip -- the quantising append of fa2_fwd_kvcache_fp8: new key / value rows in q's dtype
// written to an fp8 (OCP e4m3fn) cache as e4m3_rne(clamp(float(x) / d, -448, 448)), d the descale of
// the row's (batch, kv head).  Positions, dropping at the capacity and the paged route through the
// clamped table entry are the 16-bit append's (kvcache_append_pos.h).
#include "common.h"
#include "fa2_internal.h"

namespace fa2 {

// x / d (correctly rounded), clamped so that the convert below never overflows; the comparisons
// are false for a NaN, which stays one (fminf / fmaxf would drop it)
FA2_DEV float fp8_prescale(float x, float d) {
  float y = x / d;
  y = y > 448.f ? 448.f : y;
  return y < -448.f ? -448.f : y;
}

// 16 elements (two 16-byte chunks of a new row) -> 16 e4m3 bytes: v_cvt_pk_fp8_f32 rounds to
// nearest even and keeps NaN
template <bool BF16>
FA2_DEV u32x4 quantise16(u32x4 a, u32x4 b, float d) {
  using E = Elem<BF16>;
  u32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s0 = w < 2 ? a[2 * w] : b[2 * w - 4], s1 = w < 2 ? a[2 * w + 1] : b[2 * w - 3];
    const float x0 = fp8_prescale(E::to_f32((uint16_t)s0), d), x1 = fp8_prescale(E::to_f32((uint16_t)(s0 >> 16)), d);
    const float x2 = fp8_prescale(E::to_f32((uint16_t)s1), d), x3 = fp8_prescale(E::to_f32((uint16_t)(s1 >> 16)), d);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(x0, x1, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(x2, x3, r, true);
    out[w] = (uint32_t)r;
  }
  return out;
}

// One thread per 16 elements of a new row (32 bytes read, one 16-byte store per cache), placed
// like the 16-bit append's chunks (kvcache_append_pos.h).
template <bool BF16, bool PAGED>
__global__ void __launch_bounds__(256) kvcache_fp8_append_kernel(const fa2_fp8_kvcache_args fa) {
  const fa2_paged_kvcache_args& pg = fa.paged;
  const fa2_kvcache_args& p = fa.paged.base;
  constexpr int CW = 16;
#include "kvcache_append_pos.h"
  const float kd = fa.k_descale ? fa.k_descale[b * fa.k_descale_stride[0] + h * fa.k_descale_stride[1]] : 1.f;
  const float vd = fa.v_descale ? fa.v_descale[b * fa.v_descale_stride[0] + h * fa.v_descale_stride[1]] : 1.f;
  const uint16_t* ks = (const uint16_t*)p.k_new + b * p.k_new_stride[0] + n * p.k_new_stride[1] + h * p.k_new_stride[2] + 16 * c;
  const uint16_t* vs = (const uint16_t*)p.v_new + b * p.v_new_stride[0] + n * p.v_new_stride[1] + h * p.v_new_stride[2] + 16 * c;
  uint8_t* kdst = (uint8_t*)p.k_cache + slab * p.k_cache_stride[0] + row * p.k_cache_stride[1] + h * p.k_cache_stride[2] + 16 * c;
  uint8_t* vdst = (uint8_t*)p.v_cache + slab * p.v_cache_stride[0] + row * p.v_cache_stride[1] + h * p.v_cache_stride[2] + 16 * c;
  const u32x4 k0 = *(const u32x4*)ks, k1 = *(const u32x4*)(ks + 8), v0 = *(const u32x4*)vs, v1 = *(const u32x4*)(vs + 8);
  *(u32x4*)kdst = quantise16<BF16>(k0, k1, kd);
  *(u32x4*)vdst = quantise16<BF16>(v0, v1, vd);
}

template <>
hipError_t launch_kvcache_append(const fa2_fp8_kvcache_args& args, hipStream_t st) {
  const fa2_kvcache_args& a = args.paged.base;
  const int64_t total = (int64_t)a.batch * a.seqlen_new * a.heads_kv * (a.head_dim >> 4);
  if (total <= 0) return hipSuccess;
  const dim3 grid((unsigned)((total + 255) / 256));
  return dispatch(
      [&](auto bf, auto paged) {
        hipLaunchKernelGGL((kvcache_fp8_append_kernel<bf.value, paged.value>), grid, dim3(256), 0, st, args);
        return hipGetLastError();
      },
      a.dtype == FA2_BF16, bools{}, args.paged.block_table != nullptr, bools{});
}

}  // namespace fa2
