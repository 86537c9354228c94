// fwd.hip -- FlashAttention-2 forward for gfx950 (CDNA4).
//
// Replaces _fwd_kernel + compute_row_block (/root/reference/src/forward/kernel.py:61-291,
// /root/reference/src/forward/compute_row_blocks.py:7-103) with the same semantics:
//   s_ij = scale * <q_i, k_j> + bias_ij, bottom-right causal (j <= i + Lk - Lq), key padding,
//   online softmax in base 2, optional Philox dropout on P after the row sum, O = P V / l,
//   LSE2_i = m_i + log2(l_i) (kernel.py:119, compute_row_blocks.py:58-101).
//
// Work decomposition: one workgroup = NW waves = NW*32 query rows of one (batch, q-head);
// each wave owns 32 rows.  K/V tiles of 64 keys are staged in LDS (double buffered, LDS-DMA)
// and shared by the waves.  Per 64-key tile and wave:
//   S^T[key][q] = K Q^T        16 MFMA 32x32x16 (A = K row frags from LDS, B = Q frags in VGPRs)
//   softmax on the lane pair (l, l^32) holding one query row (16+16 keys per 32-key tile)
//   O^T[d][q]  += V^T P^T      16 MFMA (A = V^T via ds_read_b64_tr_b16, B = P in registers)
//
// Ping-pong schedule (NW = 8): waves w and w+4 share a SIMD.  Each tile takes two barrier-
// separated phases; in phase A waves 0-3 run QK^T + softmax of tile i while waves 4-7 run the
// PV of tile i-1, in phase B the roles swap.  So on every SIMD one wave's softmax VALU and
// fragment reads overlap its partner's MFMAs, instead of both waves hitting LDS, MFMA and VALU
// in lockstep.  K_{i+1} is issued at the start of A_i and V_{i+1} at the start of B_i (each
// two phases ahead of its first reader), retired by counted vmcnt waits before the barriers.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "fa2_internal.h"
#include "fwd_hp_kernel.h"
#include "fwd_pipe_kernel.h"

namespace fa2 {

// Waves per workgroup: 8 (256 query rows share each K/V tile, one workgroup per CU, two waves
// per SIMD) up to DT = 128; 4 for DT = 256, whose ~300 live registers allow one wave per SIMD.
// Causal: 4 waves (two independent workgroups per CU desynchronise each SIMD's pair of waves
// by themselves, and 128-row blocks waste less on the diagonal); non-causal: 8 waves with the
// ping-pong schedule below.
template <int DT, bool CAUSAL>
struct FwdCfg {
  static constexpr int NW = (DT >= 256 || CAUSAL) ? 4 : 8;
  static constexpr int kWavesPerSimd = DT >= 256 ? 1 : 2;
};


constexpr int kFwdLead = 3;  // fragment reads in flight ahead of their MFMA

// DROP: 0 no dropout, 1 Philox draws in the softmax (writing the keep words when asked), 2 the keep
// words a dropout_mask_kernel launch wrote just before (misc.hip) are read instead
// The body is fwd_kernel_body.h, shared with the sliding-window kernel (local_kernel.h), which
// includes it with LOCAL = true (CAUSAL, BIAS and DROP off): the
// causal case's 4-wave one-barrier-per-tile form, the tile loop confined to the block's band
// [n_begin, n_end) and every mask two-sided: key j is visible to row i iff
// max(0, i + diag - left) <= j < min(Lk, i + diag + right + 1) (window_bound: no bound = far away).
template <bool BF16, int DT, bool CAUSAL, bool BIAS, int DROP, bool ALIGNED>
__global__ void __launch_bounds__((FwdCfg<DT, CAUSAL>::NW * 64), (FwdCfg<DT, CAUSAL>::kWavesPerSimd)) fwd_kernel(const fa2_fwd_args p) {
  constexpr bool LOCAL = false;
#include "fwd_kernel_body.h"
}

// ---------------------------------------------------------------------------------------------
// fwd_kernel, the general forward, with every (CAUSAL, BIAS, DROP, ALIGNED)
template <bool BF16, int DT, bool CAUSAL, bool BIAS, int DROP, bool ALIGNED>
static hipError_t launch_fwd_t(const fa2_fwd_args& a, hipStream_t st) {
  constexpr int NW = FwdCfg<DT, CAUSAL>::NW, BM = NW * 32;
  dim3 grid(((a.seqlen_q + BM - 1) / BM) * a.batch * a.heads_q);
  hipLaunchKernelGGL((fwd_kernel<BF16, DT, CAUSAL, BIAS, DROP, ALIGNED>), grid, dim3(NW * 64), 0, st, a);
  return hipGetLastError();
}

// The plan (select_fwd), then per path one dispatch over the flags that path's kernel has: the
// hand-placed kernel exists at DT = 128 only (no bias, aligned, dropout from keep words), the
// pipelined one at DT 64 / 128 with BIASK 0 / 16 / 17 (aligned, no dropout).  A plan that holds
// anything else for its path is an error.
template <bool BF16, int DT>
hipError_t launch_fwd_dt(const fa2_fwd_args& a, LaunchCtx ctx) {
  const FwdPlan p = select_fwd(a, ctx.aligned, ctx.policy);
  if (p.path == Path::local) return launch_fwd_local<BF16, DT>(a, p, ctx.stream);
  // with a keep-mask buffer the dropout bits are drawn by dropout_mask_kernel (all VALU, full
  // occupancy) and read by the forward; without one the softmax draws them
  if (p.mask_first)
    if (hipError_t e = launch_dropout_mask(a, ctx.stream); e != hipSuccess) return e;
  if (p.path == Path::hand_placed) {
    if constexpr (DT == 128)
      if (p.biask == 0 && p.drop != 1 && p.aligned)
        return dispatch([&](auto causal, auto drop) { return launch_fwd_hp<BF16, causal.value, DT, drop.value>(a, ctx); },
                        p.causal, bools{}, p.drop == 2, bools{});
  } else if (p.path == Path::pipelined) {
    if constexpr (DT == 64 || DT == 128)
      if (p.drop == 0 && p.aligned)
        return dispatch([&](auto causal, auto biask) { return launch_fwd_pipe<BF16, DT, causal.value, biask.value>(a, ctx.stream); },
                        p.causal, bools{}, p.biask, values<0, 16, 17>{});
  } else if (p.biask <= 1) {
    return dispatch(
        [&](auto causal, auto bias, auto drop, auto aligned) {
          return launch_fwd_t<BF16, DT, causal.value, bias.value, drop.value, aligned.value>(a, ctx.stream);
        },
        p.causal, bools{}, p.biask == 1, bools{}, p.drop, values<0, 1, 2>{}, p.aligned, bools{});
  }
  return hipErrorInvalidValue;
}

}  // namespace fa2
