// local_kernel.h -- sliding-window (local) attention for gfx950: forward, dQ and dK/dV (ABI 10).
//
// Key j is visible to query i iff j < Lk and i + diag - left <= j <= i + diag + right, with
// diag = Lk - Lq over the valid lengths (bottom-right aligned, oracle/reference.py window_mask);
// a negative bound is no bound.  api.hip normalises the window before it gets here: causal is
// folded into right = 0, and a window that bounds nothing, or only restates the causal mask, never
// reaches these kernels.
//
// The three kernels are the general kernels' bodies (fwd_kernel_body.h, dq_kernel_body.h,
// dkdv_kernel_body.h) included with LOCAL = true, so the tile math, the LDS layout and the schedules
// are shared; what LOCAL adds:
//  * forward and dQ (query-stationary, 128-row blocks, 64-key tiles): the tile loop runs over the
//    block's band [n_begin, n_end) only, n_begin = max(0, m0 + diag - left) rounded down to a
//    tile, n_end = min(Lk, m0 + 128 + diag + right); the first staged tile is n_begin.  Work per
//    row block is O(left + right + 128) keys instead of O(Lk).
//  * dK/dV (key-stationary, 128-key blocks, 32-row query tiles): the sweep covers the rows
//    [max(0, n0 - diag - right), min(Lq, n0 + 128 - diag + left)) only; a block with no such row
//    stages nothing, reads no Q, dO, LSE2 or delta and writes zeros.
//  * the wave-uniform tile classes (dead / needs masks / interior) and the per-lane limits are
//    two-sided.
//  * a wave whose rows straddle the band's lower edge meets tiles that are fully masked for some of
//    its rows before those rows have seen a key (running max still -inf); see qk_softmax.
// Configuration: the forward takes the causal case's 4-wave, one-barrier-per-tile form (two
// workgroups per CU); dQ the plain one-block-per-workgroup grid (band work per row block is
// uniform, so neither heaviest-first ordering nor mirrored pairs apply); dK/dV sums each GQA group
// in fp32 in one workgroup (split 1): a dkv_workspace the caller passes is left unused and no
// reduction kernel runs.  dQ writes delta for its rows (stage bit 2), which dK/dV then reads.
// delta in the windowed dQ is the diagonal of O dO^T by MFMA, i.e. summed the way the dP chains sum,
// and the masked dK/dV steps add -delta after a dP chain started from zero: a row that sees one key
// alone (O = that key's V row) then gets dS = 0 exactly, as the mathematics says.
#pragma once
#include "bwd_kernel.h"
#include "fwd_kernel.h"

namespace fa2 {

template <bool BF16, int DT, bool ALIGNED>
__global__ void __launch_bounds__((FwdCfg<DT, true>::NW * 64), (FwdCfg<DT, true>::kWavesPerSimd)) fwd_local_kernel(const fa2_fwd_args p) {
  constexpr bool CAUSAL = false, BIAS = false, LOCAL = true;
  constexpr int DROP = 0;
#include "fwd_kernel_body.h"
}

template <bool BF16, int DT, bool ALIGNED, bool DQF32>
__global__ void __launch_bounds__(DqCfg<DT>::NW * 64, DqCfg<DT>::kWavesPerSimd) dq_local_kernel(const fa2_bwd_args p) {
  constexpr bool CAUSAL = false, DROPOUT = false, LOCAL = true;
  constexpr int BIASK = 0;
#include "dq_kernel_body.h"
}

template <bool BF16, int DT, bool ALIGNED>
__global__ void __launch_bounds__(256, DT >= 256 ? 1 : 2) dkdv_local_kernel(const fa2_bwd_args p) {
  constexpr bool CAUSAL = false, DROPOUT = false, LOCAL = true;
  constexpr int BIASK = 0, nsplit = 1;
#include "dkdv_kernel_body.h"
}

template <bool BF16, int DT>
hipError_t launch_fwd_local(const fa2_fwd_args& a, const FwdPlan& plan, hipStream_t st) {
  constexpr int NW = FwdCfg<DT, true>::NW, BM = NW * 32;
  dim3 grid(((a.seqlen_q + BM - 1) / BM) * a.batch * a.heads_q);
  return dispatch(
      [&](auto aligned) {
        hipLaunchKernelGGL((fwd_local_kernel<BF16, DT, aligned.value>), grid, dim3(NW * 64), 0, st, a);
        return hipGetLastError();
      },
      plan.aligned, bools{});
}

// the stages of select_bwd's plan for a window: the standalone delta, dQ (writes delta too), dK/dV
// (the bias gradient is rejected with a window)
template <bool BF16, int DT>
hipError_t launch_bwd_local(const fa2_bwd_args& a, const BwdPlan& plan, hipStream_t st) {
  return dispatch(
      [&](auto aligned, auto f32) {
        for (int i = 0; i < plan.nstages; ++i) {
          if (plan.stage[i].kind == Stage::delta) {
            launch_delta<BF16, aligned.value>(a, st);
          } else if (plan.stage[i].kind == Stage::dq) {
            constexpr int NW = DqCfg<DT>::NW, BM = NW * 32;
            dim3 grid(((a.seqlen_q + BM - 1) / BM) * a.batch * a.heads_q);
            hipLaunchKernelGGL((dq_local_kernel<BF16, DT, aligned.value, f32.value>), grid, dim3(NW * 64), 0, st, a);
          } else if (plan.stage[i].kind == Stage::dkdv) {
            dim3 grid(((a.seqlen_k + 127) / 128) * a.batch * a.heads_kv);
            hipLaunchKernelGGL((dkdv_local_kernel<BF16, DT, aligned.value>), grid, dim3(256), 0, st, a);
          }
        }
        return hipGetLastError();
      },
      plan.aligned, bools{}, plan.dq_f32, bools{});
}

}  // namespace fa2
