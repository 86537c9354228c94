// kvcache_kernel.h -- KV-cache decode attention for gfx950 (ABI 10 minor 1, fa2_fwd_kvcache).
//
// A few query tokens per sequence against a pre-allocated key / value cache [B, capacity, Hkv, D]
// whose filled length L_b is read on the device (cache_seqlens).  The kernel is bound by reading
// the visible keys and values once, so the work is cut for that:
//  * unit = (batch, kv head, 32-row tile, key split).  The rows of a tile are the G = Hq / Hkv
//    q-heads of the group times the Sq query positions (row = i * G + g), padded to 32 with zero Q
//    rows that are never stored: K / V of a kv head are streamed once for the whole group.
//  * the 64-key tiles of a unit's key range are dealt round-robin to the NW waves of the workgroup;
//    each wave runs the forward's step on its tiles -- S^T = K Q^T and O^T = V^T P^T by MFMA
//    32x32x16 in the swapped arrangement of common.h, base-2 online softmax per lane pair -- with a
//    K and a V tile of its own in LDS (LDS-DMA, one tile ahead: K(t+1) is issued when S(t) has
//    consumed K(t), V(t+1) when the PV product has consumed V(t)) and its own (m, l, O).  The waves
//    merge once at the end through LDS, in wave order.
//  * the key range of split s is computed from the actual L_b: the visible span of the batch
//    [start, L_b), start = max(0, L_b - Sq - left) rounded down to a tile with a left window bound
//    and 0 without, is cut into nsplit runs of ceil(ceil(span / 64) / nsplit) tiles.  A split whose
//    run is empty reads no key and writes O = 0, LSE2 = -inf.  nsplit is a host function of the
//    shapes only (select.h), so nothing depends on the lengths on the host.
//  * nsplit == 1: the unit writes O and LSE2.  Otherwise it writes its normalised fp32 partial O and
//    its LSE2 into the workspace and kvcache_combine_kernel (kvcache.hip) sums them in split order.
// Masking: every score is masked per element against the row's [lo, hi] key interval (hi <= L_b - 1),
// which also covers the rows of a tile past L_b (staged as copies of row L_b - 1: cache rows at or
// past L_b are never read).  A row whose running max is still -inf exponentiates against 0, so a
// fully masked tile adds exact zeros (as the windowed forward).
//
// Paged caches (fa2_fwd_kvcache_paged): pools of blocks [num_blocks, P, Hkv, D], logical
// key j of batch b in row j % P of block block_table[b, j / P].  kvcache_paged_split_kernel is the
// same body (kvcache_kernel_body.h) with PAGED = true: what differs is the source address of a
// tile's rows (stage_tile_paged) and the lookup of the block ids one step ahead (kv_page_ids).
//
// fp8 (OCP e4m3fn) caches (fa2_fwd_kvcache_fp8): kvcache_fp8_split_kernel is the same body
// with FP8 = true: K / V tiles are staged as bytes and converted to q's dtype in registers.
//  * A cache element's value is its exact e4m3 value (every finite e4m3 value is a bf16 and an
//    fp16 value), so the conversion is lossless and the MFMAs are those of the 16-bit kernel.  The
//    per-(batch, kv head) descales never touch K or V: kd goes into the score multiplier
//    (softmax_scale * kd) * log2e, vd multiplies O in fp32 before its one rounding (on the split
//    path the fp32 partials, so kvcache_combine_kernel runs unchanged).
//  * LDS image: a 64-key x DT-byte tile is the Tile<DT / 2, 64> image of its rows read as DT / 2
//    16-bit words (byte pairs), so stage_tile / stage_tile_paged stage it as they are: DT / 16
//    LDS-DMA pieces of 16 bytes = 16 elements per lane.
//  * K rows: lane (r32, hh) reads the 8 bytes 16 ks + 8 hh .. + 7 of key r32 (ds_read_b64) and
//    converts them to one 16-byte MFMA fragment.
//  * V^T: ds_read_b64_tr_b16 on the byte pairs (lds_tr_frag on the 16-bit view).  Lane (r32, h)
//    then holds the pair (d, d + 1), d = 64 su + 2 r32, of the eight keys of a k-step in the
//    permuted key order of P; v_perm_b32 separates the even and the odd column, and the two feed two
//    accumulators: acc[2 su] holds columns 64 su + 2 m, acc[2 su + 1] columns 64 su + 2 m + 1 (m the
//    accumulator row).  The epilogue interleaves them: registers 4 g4 + e of the two accumulators
//    are the eight consecutive columns 64 su + 16 g4 + 8 hh + 2 e + parity.
//  * Bytes in flight: a workgroup's LDS is half the 16-bit kernel's (64 KiB + 1 KiB at DT = 128),
//    and the kernel is bounded to 256 VGPRs, so two workgroups share a CU: per CU the same K and V
//    bytes are ahead as in the 16-bit kernel (which fits one).
#pragma once
#include "common.h"
#include "fa2_internal.h"

namespace fa2 {

template <int DT>
struct KvCfg {
  static constexpr int NW = DT >= 256 ? 2 : 4;    // waves per workgroup
  static constexpr int kTile = 64 * DT * 2;        // bytes of a 64-key K or V tile
  static constexpr int kWave = 2 * kTile;          // a wave's K and V tile (its fp32 O image at the merge)
  static constexpr int kPieces = DT / 8;           // LDS-DMA instructions of one tile, per lane
};
template <int DT>
struct KvFp8Cfg {
  static constexpr int NW = 4;              // waves per workgroup
  static constexpr int kTile = 64 * DT;     // bytes of a 64-key K or V tile
  static constexpr int kWave = 2 * kTile;   // a wave's K and V tile (its fp32 O image at the merge)
  static constexpr int kPieces = DT / 16;   // LDS-DMA instructions of one tile, per lane
};

template <int N>
FA2_DEV void vm_wait_but() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
FA2_DEV void lds_wait_all() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// What the shared body (kvcache_kernel_body.h) names `pg` and `fa`: the paging fields of
// fa2_paged_kvcache_args and the descales of fa2_fp8_kvcache_args in the kernels that have them,
// these empty stand-ins in the others (read only inside `if constexpr (PAGED)` / `if constexpr
// (FP8)`, which those kernels discard: a non-dependent name there is still looked up).
struct KvNoPages {
  const int32_t* block_table = nullptr;
  int64_t block_table_stride = 0;
  int32_t page_block_size = 64, num_blocks = 1;
};
struct KvNoDescales {
  const float *k_descale = nullptr, *v_descale = nullptr;
  int64_t k_descale_stride[2] = {0, 0}, v_descale_stride[2] = {0, 0};
};

// The block ids of the (at most four) pages under the 64-key tile at n0 (a multiple of 64, < L),
// clamped into the pool.  Only pages that hold a key below L are looked up: page n0 / P up to page
// (min(n0 + 64, L) - 1) / P, the last one repeated.  The entries must not come through a vector
// load: it would sit between a tile's LDS-DMA pieces and the counted vmcnt wait that retires them.
// The compiler turns a uniform load into a vector one once an asm with a memory clobber (the DMA)
// has run, so the four scalar loads are written out; they are counted by lgkmcnt and retired here.
FA2_DEV const int32_t* kv_entry_ptr(const int32_t* row, int idx) { return (const int32_t*)uniform64((int64_t)(row + idx)); }
FA2_DEV int kv_clamp_block(int e, int num_blocks) { return min(max(e, 0), num_blocks - 1); }
FA2_DEV void kv_page_ids(int& p0, int& p1, int& p2, int& p3, const int32_t* row, int log_p, int num_blocks, int n0, int L) {
  const int first = n0 >> log_p, last = (min(n0 + 64, L) - 1) >> log_p;
  const int32_t* a0 = kv_entry_ptr(row, first);
  const int32_t* a1 = kv_entry_ptr(row, min(first + 1, last));
  const int32_t* a2 = kv_entry_ptr(row, min(first + 2, last));
  const int32_t* a3 = kv_entry_ptr(row, min(first + 3, last));
  int e0, e1, e2, e3;
  asm volatile(
      "s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %5, 0x0\n\ts_load_dword %2, %6, 0x0\n\t"
      "s_load_dword %3, %7, 0x0\n\ts_waitcnt lgkmcnt(0)"
      : "=&s"(e0), "=&s"(e1), "=&s"(e2), "=&s"(e3)
      : "s"(a0), "s"(a1), "s"(a2), "s"(a3)
      : "memory");
  p0 = kv_clamp_block(e0, num_blocks);
  p1 = kv_clamp_block(e1, num_blocks);
  p2 = kv_clamp_block(e2, num_blocks);
  p3 = kv_clamp_block(e3, num_blocks);
}

// stage_tile<DT, 64, 64, true> for a paged pool: the same LDS image from the same logical rows
// (n0 + r, clamped to L - 1), each found through its page's block id.  A lane's pieces lie in
// four rows only (16 q + lane / 4), so the row's address is worked out four times per tile and
// every piece adds its 16-byte chunk.  With P >= 64 every row is in page 0 of the four.
// (everything below is passed by value and kept out of arrays, structs and reference captures:
// through memory the compiler turns the selects into an indexed private array, i.e. scratch)
FA2_DEV int64_t kv_paged_row(int grow, int first, int log_p, int e0, int e1, int e2, int e3, int64_t block_stride,
                             int64_t row_stride) {
  const int j = (grow >> log_p) - first;
  int blk = e0;  // three selects of values already in registers
  blk = j > 0 ? e1 : blk;
  blk = j > 1 ? e2 : blk;
  blk = j > 2 ? e3 : blk;
  return (int64_t)blk * block_stride + (int64_t)(grow & ((1 << log_p) - 1)) * row_stride;
}
template <int DT>
FA2_DEV void stage_tile_paged(char* tile, const uint16_t* g, int64_t block_stride, int64_t row_stride, int e0, int e1, int e2, int e3,
                              int log_p, int n0, int L, int D, int lane) {
  const int dchunks = D >> 3, first = n0 >> log_p, r = n0 + (lane >> 2), last = L - 1;
  const int64_t r0 = kv_paged_row(min(r, last), first, log_p, e0, e1, e2, e3, block_stride, row_stride);
  const int64_t r1 = kv_paged_row(min(r + 16, last), first, log_p, e0, e1, e2, e3, block_stride, row_stride);
  const int64_t r2 = kv_paged_row(min(r + 32, last), first, log_p, e0, e1, e2, e3, block_stride, row_stride);
  const int64_t r3 = kv_paged_row(min(r + 48, last), first, log_p, e0, e1, e2, e3, block_stride, row_stride);
#pragma unroll
  for (int sub = 0; sub < DT / 32; ++sub) {  // pieces 4 sub + q: rows 16 q + lane / 4 of the 32-column sub-tile
    // logical chunk stored at piece 4 sub + q of this lane: the row's swizzle is (row >> 2) & 3
    const int x = (lane >> 4) & 3, c0 = sub * 4 + ((lane & 3) ^ x);
    const int gc = c0 < dchunks ? c0 : dchunks - 1;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_addr(tile + sub * 4096));
    glds16(g + r0 + gc * 8, dst);
    glds16(g + r1 + gc * 8, dst + 1024);
    glds16(g + r2 + gc * 8, dst + 2048);
    glds16(g + r3 + gc * 8, dst + 3072);
  }
}

// two e4m3 bytes (the low or the high half of w) as two elements of q's dtype, exactly
template <bool BF16>
FA2_DEV uint32_t fp8x2_to_elem(uint32_t w, bool high) {
  if constexpr (BF16) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 r = high ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, r);
  } else {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 r = high ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, r);
  }
}
template <bool BF16>
FA2_DEV u32x4 fp8x8_to_frag(uint32_t lo, uint32_t hi) {
  return u32x4{fp8x2_to_elem<BF16>(lo, false), fp8x2_to_elem<BF16>(lo, true), fp8x2_to_elem<BF16>(hi, false),
               fp8x2_to_elem<BF16>(hi, true)};
}

// K fragment of k-step ks of a byte tile (DH = DT / 2 its width in byte pairs): bytes
// 16 ks + 8 hh .. + 7 of tile row row0 + r32 (chunk ks of the row, its half hh), converted.
template <bool BF16, int DH>
FA2_DEV u32x4 lds_row_frag_fp8(const char* tile, int row0, int r32, int ks, int hh) {
  const int off = (ks >> 2) * Tile<DH, 64>::kSub + (row0 + r32) * 64 + (((ks & 3) ^ ((r32 >> 2) & 3)) << 4) + 8 * hh;
  const u32x2 w = *(const u32x2*)(tile + off);
  return fp8x8_to_frag<BF16>(w[0], w[1]);
}

// V^T fragments of keys row0 .. row0 + 15 (the permuted order of lds_tr_frag) for the byte pair
// (64 su + 2 r32, + 1): `even` and `odd` are the two columns' A operands.
template <bool BF16, int DH>
FA2_DEV void lds_tr_frag_fp8(u32x4& even, u32x4& odd, const char* tile, int row0, int su, int lane) {
  const u32x4 t = lds_tr_frag<DH, 64>(tile, row0, 32 * su, lane);  // dword i: keys 2 i, 2 i + 1 as (even, odd) bytes
  const uint32_t e0 = __builtin_amdgcn_perm(t[1], t[0], 0x06040200u), e1 = __builtin_amdgcn_perm(t[3], t[2], 0x06040200u);
  const uint32_t o0 = __builtin_amdgcn_perm(t[1], t[0], 0x07050301u), o1 = __builtin_amdgcn_perm(t[3], t[2], 0x07050301u);
  even = fp8x8_to_frag<BF16>(e0, e1);
  odd = fp8x8_to_frag<BF16>(o0, o1);
}

// The body's two choices by cache type.  kv_stage_tile: a 64-key tile through either layout; the
// overload for a byte cache stages the byte-pair view with the 16-bit stagers (strides and D
// halved: 16-byte aligned rows make every stride even).  kv_k_frag: the K fragment of k-step ks.
template <int DT, bool PAGED>
FA2_DEV void kv_stage_tile(char* tile, const uint16_t* g, int64_t block_stride, int64_t row_stride, int e0, int e1, int e2, int e3,
                           int log_p, int n0, int L, int D, int lane) {
  if constexpr (PAGED) stage_tile_paged<DT>(tile, g, block_stride, row_stride, e0, e1, e2, e3, log_p, n0, L, D, lane);
  else stage_tile<DT, 64, 64, true>(tile, g, row_stride, n0, L, D, lane);
}
template <int DT, bool PAGED>
FA2_DEV void kv_stage_tile(char* tile, const uint8_t* g, int64_t block_stride, int64_t row_stride, int e0, int e1, int e2, int e3,
                           int log_p, int n0, int L, int D, int lane) {
  kv_stage_tile<DT / 2, PAGED>(tile, (const uint16_t*)g, block_stride >> 1, row_stride >> 1, e0, e1, e2, e3, log_p, n0, L, D >> 1, lane);
}
template <bool BF16, int DT, bool FP8>
FA2_DEV u32x4 kv_k_frag(const char* tile, int row0, int r32, int ks, int hh) {
  if constexpr (FP8) return lds_row_frag_fp8<BF16, DT / 2>(tile, row0, r32, ks, hh);
  else return lds_row_frag<DT, 64>(tile, row0, r32, ks, hh);
}

template <bool BF16, int DT>
__global__ void __launch_bounds__(KvCfg<DT>::NW * 64) kvcache_split_kernel(const fa2_kvcache_args p, const int nsplit) {
  constexpr bool PAGED = false, FP8 = false;
  constexpr KvNoPages pg{};
  constexpr KvNoDescales fa{};
#include "kvcache_kernel_body.h"
}

template <bool BF16, int DT>
__global__ void __launch_bounds__(KvCfg<DT>::NW * 64) kvcache_paged_split_kernel(const fa2_paged_kvcache_args pg, const int nsplit) {
  constexpr bool PAGED = true, FP8 = false;
  constexpr KvNoDescales fa{};
  const fa2_kvcache_args& p = pg.base;
#include "kvcache_kernel_body.h"
}

// 256 threads, two workgroups per CU (at most 256 VGPRs): see "bytes in flight" above
template <bool BF16, int DT, bool PAGED>
__global__ void __launch_bounds__(256, 2) kvcache_fp8_split_kernel(const fa2_fp8_kvcache_args fa, const int nsplit) {
  constexpr bool FP8 = true;
  const fa2_paged_kvcache_args& pg = fa.paged;
  const fa2_kvcache_args& p = fa.paged.base;
#include "kvcache_kernel_body.h"
}

// One launcher for the three argument structs: the kernel follows from the struct and, for fp8
// caches (one struct for both layouts), from PAGED (fa2_internal.h has its default).
template <bool BF16, int DT, typename Args, bool PAGED>
hipError_t launch_kvcache_split(const Args& a, int nsplit, hipStream_t st) {
  constexpr bool FP8 = std::is_same_v<Args, fa2_fp8_kvcache_args>;
  const dim3 grid((unsigned)(kv_units(kv_base(a)) * nsplit)), block(std::conditional_t<FP8, KvFp8Cfg<DT>, KvCfg<DT>>::NW * 64);
  if constexpr (FP8) hipLaunchKernelGGL((kvcache_fp8_split_kernel<BF16, DT, PAGED>), grid, block, 0, st, a, nsplit);
  else if constexpr (PAGED) hipLaunchKernelGGL((kvcache_paged_split_kernel<BF16, DT>), grid, block, 0, st, a, nsplit);
  else hipLaunchKernelGGL((kvcache_split_kernel<BF16, DT>), grid, block, 0, st, a, nsplit);
  return hipGetLastError();
}

}  // namespace fa2
