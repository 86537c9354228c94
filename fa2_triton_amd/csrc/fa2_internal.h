// fa2_internal.h -- what the C ABI (api.hip) and the kernel translation units share on the host:
// the launcher entry points, the context a call hands them, and the one dispatcher that turns
// runtime values into template arguments.  What a call launches is decided in select.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "select.h"

namespace fa2 {

// What api.hip hands every launcher besides the arguments: the stream, whether every row of every
// 16-bit tensor is 16-byte aligned, and the fa2_policy of the call (nullptr: the defaults).  The
// library keeps no state between calls and none per thread besides the error string.
struct LaunchCtx {
  hipStream_t stream;
  bool aligned;
  const fa2_policy* policy;
};

// dispatch(f, v1, values<a, b, ...>{}, v2, values<...>{}, ...) calls
// f(std::integral_constant<decltype(a), a>{}, ...) with the listed constants equal to v1, v2, ...;
// hipErrorInvalidValue when a value is not in its list.  Every combination of the lists is
// instantiated: f rules out the ones that must not exist with `if constexpr`.
template <auto... Vs>
struct values {};
using bools = values<false, true>;

template <typename F>
hipError_t dispatch(F&& f) {
  return f();
}
template <typename F, typename T, auto... Vs, typename... Rest>
hipError_t dispatch(F&& f, T v, values<Vs...>, Rest... rest) {
  hipError_t e = hipErrorInvalidValue;
  auto bound = [&](auto c) { return dispatch([&](auto... cs) { return f(c, cs...); }, rest...); };
  (void)((v == Vs && ((e = bound(std::integral_constant<decltype(Vs), Vs>{})), true)) || ...);
  return e;
}
using dtypes = bools;                     // BF16
using tiles = values<32, 64, 128, 256>;  // DT (head_dim_tile)

// compute units of the current device (persistent grids, the decode split heuristic), cached per
// device id; 256 (an MI355X) when there is none to ask
inline int device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!cached[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// Forward and backward (fwd_kernel.h, bwd_kernel.h), one translation unit per (dtype, head-dim
// tile): select_fwd / select_bwd, one dispatch over the plan, the launches.  stages: bit 0 delta,
// bit 1 dK/dV, bit 2 dQ, bit 3 the bias gradient.
template <bool BF16, int DT>
hipError_t launch_fwd_dt(const fa2_fwd_args& a, LaunchCtx ctx);
template <bool BF16, int DT>
hipError_t launch_bwd_dt(const fa2_bwd_args& a, LaunchCtx ctx, int stages);

// Sliding-window (local) attention, ABI 10 (local_kernel.h): one translation unit of its own per
// (dtype, head-dim tile).  Called by the two launchers above with a plan whose path is local;
// api.hip has normalised the window by then (causal folded into window_right = 0, a window that
// bounds nothing or only restates the causal mask turned off) and rejected bias / dropout / dbias.
template <bool BF16, int DT>
hipError_t launch_fwd_local(const fa2_fwd_args& a, const FwdPlan& plan, hipStream_t st);
template <bool BF16, int DT>
hipError_t launch_bwd_local(const fa2_bwd_args& a, const BwdPlan& plan, hipStream_t st);

hipError_t launch_cu_seqlens(const uint8_t* mask, int64_t stride, int batch, int seqlen,
                             int32_t* out, hipStream_t st);

// Dropout keep words of a forward (misc.hip, into a.dropout_mask) drawn ahead of a kernel that
// reads them; keep <=> the Philox integer x' > dropout_keep_threshold(p).
uint32_t dropout_keep_threshold(float p);
hipError_t launch_dropout_mask(const fa2_fwd_args& a, hipStream_t st);

// KV-cache decode, Args = fa2_kvcache_args, fa2_paged_kvcache_args or fa2_fp8_kvcache_args (DESIGN
// 12 - 14): the split attention kernel (kvcache_kernel.h, one translation unit per cache type,
// layout, dtype and head-dim tile; fp8 caches: the tiles of fp8_tiles, and PAGED chosen by the
// caller from fp8_paged, since one struct serves both layouts), the append of k_new / v_new
// (kvcache.hip; the quantising one of fp8 caches in kvcache_fp8.hip) and the combination of
// nsplit > 1 partial results (kvcache.hip), which is the same for all three.
using fp8_tiles = values<64, 128>;  // DT (fp8_head_dim_tile)
template <bool BF16, int DT, typename Args, bool PAGED = std::is_same_v<Args, fa2_paged_kvcache_args>>
hipError_t launch_kvcache_split(const Args& a, int nsplit, hipStream_t st);
template <typename Args>
hipError_t launch_kvcache_append(const Args& a, hipStream_t st);
template <>
hipError_t launch_kvcache_append(const fa2_fp8_kvcache_args& a, hipStream_t st);
hipError_t launch_kvcache_combine(const fa2_kvcache_args& a, int nsplit, hipStream_t st);
// Shared-prefix decode (kvprefix.hip): the merge of the prefix pass's ns_p partial results
// at ws_p ([ns_p, 1, Hq, B * Sq, D] and their LSE2) with the sequence pass's ns_s at ws_s
// ([ns_s, B, Hq, Sq, D] and theirs) into o / lse of `a`, the per-sequence call.
hipError_t launch_kvprefix_merge(const fa2_kvcache_args& a, const float* ws_p, int ns_p, const float* ws_s, int ns_s,
                                 hipStream_t st);

}  // namespace fa2
