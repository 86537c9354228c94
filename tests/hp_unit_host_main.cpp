// hp_unit_host_main.cpp -- the unit and tile-class arithmetic of csrc/hp_unit.h against a brute
// force over single rows and keys (tests/test_hp_unit_host.py).  Host code only: no HIP, no GPU.
//
// Visibility: key j is visible to row i iff j < Lk and, causal, j <= i + Lk - Lq.
#include <stdio.h>

#include "hp_unit.h"

using namespace fa2;

static const int kLens[] = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 383, 384, 385, 400};
static const int kNumLens = sizeof(kLens) / sizeof(kLens[0]);

template <bool CAUSAL>
static bool visible(int i, int j, int Lq, int Lk) {
  return j < Lk && (!CAUSAL || j <= i + Lk - Lq);
}

// the last key that any of rows [r0, r0 + n) sees (-1: none); rows past Lq count like any other:
// the kernels mask them by row, the tile classes only by the wave's position
template <bool CAUSAL>
static int last_key(int r0, int n, int Lq, int Lk) {
  int last = -1;
  for (int i = r0; i < r0 + n; ++i)
    for (int j = 0; j < Lk; ++j)
      if (visible<CAUSAL>(i, j, Lq, Lk) && j > last) last = j;
  return last;
}

static long g_cases = 0, g_bad = 0;
static void check(const char* what, int causal, int Lq, int Lk, int mb, int w, int got, int want) {
  ++g_cases;
  if (got != want && g_bad++ < 20)
    printf("MISMATCH %s causal=%d Lq=%d Lk=%d mb=%d wave=%d: got %d, brute force %d\n", what, causal, Lq, Lk, mb, w, got, want);
}

template <bool CAUSAL>
static void sweep() {
  for (int a = 0; a < kNumLens; ++a)
    for (int c = 0; c < kNumLens; ++c) {
      const int Lq = kLens[a], Lk = kLens[c];
      // B = 1, Hq = 4, Hkv = 2, unit of head 3 (kv head 1); one row block past the last one too
      for (int mb = 0; mb <= (Lq + 255) / 256; ++mb) {
        HpRowUnit<CAUSAL> u;
        const int hkv = u.init(4, 2, Lq, Lk, nullptr, 3, mb);
        check("b", CAUSAL, Lq, Lk, mb, -1, u.b, 0);
        check("hq", CAUSAL, Lq, Lk, mb, -1, u.hq, 3);
        check("hkv", CAUSAL, Lq, Lk, mb, -1, hkv, 1);
        check("m0", CAUSAL, Lq, Lk, mb, -1, u.m0, 256 * mb);
        // ntiles: the 64-key tiles up to the last one any of the block's 256 rows sees; none when
        // the block starts past Lq
        const int blk_last = u.m0 >= Lq ? -1 : last_key<CAUSAL>(u.m0, 256, Lq, Lk);
        check("ntiles", CAUSAL, Lq, Lk, mb, -1, u.ntiles, blk_last < 0 ? 0 : blk_last / 64 + 1);
        for (int w = 0; w < 4; ++w) {
          const int qw0 = u.m0 + 64 * w;
          const int diag = u.Lk - u.Lq;
          const int tc_n_full = hp_n_full<CAUSAL>(u.Lk, diag, qw0), tc_last = hp_last_tile<CAUSAL>(diag, qw0, u.ntiles);
          // last: the last tile any of the wave's 64 rows sees, clamped to ntiles - 1
          const int wl = last_key<CAUSAL>(qw0, 64, Lq, Lk);
          int last = wl < 0 ? -1 : wl / 64;
          if (last > u.ntiles - 1) last = u.ntiles - 1;
          check("last", CAUSAL, Lq, Lk, mb, w, tc_last, last);
          // live0 (tile 0 is live for the wave) is last >= 0: the wave sees key 0
          check("live0", CAUSAL, Lq, Lk, mb, w, tc_last >= 0, u.ntiles > 0 && visible<CAUSAL>(qw0 + 63, 0, Lq, Lk));
          // n_full: leading tiles wholly below Lk that the wave's first row sees whole
          int n_full = 0;
          for (;; ++n_full) {
            bool whole = 64 * n_full + 63 < Lk;
            for (int j = 64 * n_full; whole && j < 64 * n_full + 64; ++j) whole = visible<CAUSAL>(qw0, j, Lq, Lk);
            if (!whole) break;
          }
          check("n_full", CAUSAL, Lq, Lk, mb, w, tc_n_full, n_full);
        }
      }
    }
}

int main() {
  sweep<false>();
  sweep<true>();
  // varlen: both lengths from cu_seqlens, batch and heads from bh
  const int32_t cu[3] = {0, 100, 400};
  HpRowUnit<true> u;
  const int hkv = u.init(6, 2, 512, 512, cu, 6 + 5, 1);
  check("varlen b", 1, 300, 300, 1, -1, u.b, 1);
  check("varlen hq", 1, 300, 300, 1, -1, u.hq, 5);
  check("varlen hkv", 1, 300, 300, 1, -1, hkv, 1);
  check("varlen Lq", 1, 300, 300, 1, -1, u.Lq, 300);
  check("varlen Lk", 1, 300, 300, 1, -1, u.Lk, 300);
  check("varlen ntiles", 1, 300, 300, 1, -1, u.ntiles, 5);
  printf("%ld checks, %ld mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
