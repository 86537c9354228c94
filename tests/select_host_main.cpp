// select_host_main.cpp -- prints the plans of csrc/select.h for the calls tests/test_select_host.py
// lists, one line per case.  Host code only: no HIP, no GPU.
#include <stdio.h>

#include <functional>

#include "select.h"

using namespace fa2;

static void* const kPtr = (void*)0x1000;  // non-null, 16-byte aligned; never dereferenced
static const char* kPath[] = {"general", "pipelined", "hand_placed", "local"};
static const char* kStage[] = {"delta", "dq", "dbias", "dkdv"};

static void bshd(int64_t* s, int S, int H, int D) { s[0] = (int64_t)S * H * D, s[1] = (int64_t)H * D, s[2] = D; }

// The base call: bf16, B = 1, Hq = Hkv = 2, Sq = Sk = 256, D = 128, contiguous BSHD tensors.
template <typename Args>
static void base_sizes(Args& a, int D, int Sk, int Hq, int Hkv) {
  a.batch = 1, a.heads_q = Hq, a.heads_kv = Hkv, a.seqlen_q = 256, a.seqlen_k = Sk, a.head_dim = D;
  a.lse_row_stride = 256, a.dtype = FA2_BF16, a.softmax_scale = 1.f;
  a.q = a.k = a.v = a.o = kPtr;
  bshd(a.q_stride, 256, Hq, D), bshd(a.o_stride, 256, Hq, D), bshd(a.k_stride, Sk, Hkv, D), bshd(a.v_stride, Sk, Hkv, D);
}
template <typename Args>
static void with_bias(Args& a, int dtype) {
  a.bias = kPtr, a.bias_dtype = dtype;
  a.bias_stride[0] = (int64_t)a.heads_q * a.seqlen_q * a.seqlen_k, a.bias_stride[1] = (int64_t)a.seqlen_q * a.seqlen_k;
  a.bias_stride[2] = a.seqlen_k;
}
static fa2_fwd_args fwd_base(int D = 128, int Sk = 256) {
  fa2_fwd_args a = {};
  base_sizes(a, D, Sk, 2, 2);
  a.lse = (float*)kPtr;
  return a;
}
static fa2_bwd_args bwd_base(int Sk = 256, int Hq = 2, int Hkv = 2) {
  fa2_bwd_args a = {};
  base_sizes(a, 128, Sk, Hq, Hkv);
  a.dout = a.dq = a.dk = a.dv = kPtr, a.lse = a.delta = (float*)kPtr, a.dq_dtype = FA2_BF16;
  bshd(a.do_stride, 256, Hq, 128), bshd(a.dq_stride, 256, Hq, 128), bshd(a.dk_stride, Sk, Hkv, 128), bshd(a.dv_stride, Sk, Hkv, 128);
  return a;
}

static void fwd(const char* name, fa2_fwd_args a, const fa2_policy* policy = nullptr) {
  for (int causal = 0; causal < 2; ++causal) {
    a.causal = causal;
    const FwdPlan p = select_fwd(a, a.head_dim % 8 == 0, policy);
    printf("fwd %s causal=%d: %s tile=%d causal=%d biask=%d drop=%d aligned=%d mask_first=%d\n", name, causal, kPath[(int)p.path],
           head_dim_tile(a.head_dim), p.causal, p.biask, p.drop, p.aligned, p.mask_first);
  }
}

static void bwd(const char* name, const fa2_bwd_args& a, int stages = 6, const fa2_policy* policy = nullptr, bool aligned = true) {
  const BwdPlan p = select_bwd(a, aligned, stages, policy);
  printf("bwd %s stages=%d: causal=%d biask=%d dropout=%d aligned=%d dq_f32=%d nsplit=%d reduce=%d [", name, stages, p.causal,
         p.biask, p.dropout, p.aligned, p.dq_f32, p.nsplit, p.reduce);
  for (int i = 0; i < p.nstages; ++i) printf("%s%s:%s", i ? " " : "", kStage[(int)p.stage[i].kind], kPath[(int)p.stage[i].path]);
  printf("]\n");
}

int main() {
  const fa2_policy no_fwd = {FA2_PATH_FWD_HP, 0}, no_dq = {FA2_PATH_DQ_HP, 0}, no_dkdv = {FA2_PATH_DKDV_HP, 0};
  uint32_t* const mask = (uint32_t*)kPtr;
  auto F = [](fa2_fwd_args a, const std::function<void(fa2_fwd_args&)>& f) { return f(a), a; };
  auto B = [](fa2_bwd_args a, const std::function<void(fa2_bwd_args&)>& f) { return f(a), a; };

  fwd("base", fwd_base());
  fwd("fwd_hp_off", fwd_base(), &no_fwd);
  fwd("d64", fwd_base(64));
  fwd("d120", fwd_base(120));
  fwd("d32", fwd_base(32));
  fwd("d256", fwd_base(256));
  fwd("d111", fwd_base(111));
  fwd("bias_bf16", F(fwd_base(), [](fa2_fwd_args& a) { with_bias(a, FA2_BF16); }));
  fwd("bias_f16", F(fwd_base(), [](fa2_fwd_args& a) { with_bias(a, FA2_F16); }));
  fwd("bias_f32", F(fwd_base(), [](fa2_fwd_args& a) { with_bias(a, FA2_F32); }));
  fwd("bias_rows_unaligned", F(fwd_base(), [](fa2_fwd_args& a) { with_bias(a, FA2_BF16), a.bias_stride[2] = 260; }));
  fwd("dropout_mask", F(fwd_base(), [&](fa2_fwd_args& a) { a.dropout_p = 0.1f, a.dropout_mask = mask; }));
  fwd("dropout_mask_fwd_hp_off", F(fwd_base(), [&](fa2_fwd_args& a) { a.dropout_p = 0.1f, a.dropout_mask = mask; }), &no_fwd);
  fwd("dropout_no_mask", F(fwd_base(), [](fa2_fwd_args& a) { a.dropout_p = 0.1f; }));
  fwd("d64_dropout_mask", F(fwd_base(64), [&](fa2_fwd_args& a) { a.dropout_p = 0.1f, a.dropout_mask = mask; }));
  fwd("kv_row_strides_differ", F(fwd_base(), [](fa2_fwd_args& a) { a.v_stride[1] = 512; }));
  fwd("stride1024_sk_2p20", F(fwd_base(128, 1 << 20), [](fa2_fwd_args& a) { a.k_stride[1] = a.v_stride[1] = 1024; }));
  fwd("stride1024_sk_2p20_m256", F(fwd_base(128, (1 << 20) - 256), [](fa2_fwd_args& a) { a.k_stride[1] = a.v_stride[1] = 1024; }));
  fwd("local_left64", F(fwd_base(), [](fa2_fwd_args& a) { a.local = 1, a.window_left = 64; }));

  bwd("base", bwd_base());
  bwd("base_causal", B(bwd_base(), [](fa2_bwd_args& a) { a.causal = 1; }));
  bwd("dq_hp_off", bwd_base(), 6, &no_dq);
  bwd("dkdv_hp_off", bwd_base(), 6, &no_dkdv);
  bwd("dq_f32", B(bwd_base(), [](fa2_bwd_args& a) { a.dq_dtype = FA2_F32; }));
  bwd("dropout_no_mask", B(bwd_base(), [](fa2_bwd_args& a) { a.dropout_p = 0.1f; }));
  bwd("dropout_mask_q_do_strides_differ",
      B(bwd_base(), [&](fa2_bwd_args& a) { a.dropout_p = 0.1f, a.dropout_mask = mask, a.do_stride[1] = 512; }));
  bwd("bias_bf16", B(bwd_base(), [](fa2_bwd_args& a) { with_bias(a, FA2_BF16); }));
  bwd("bias_f16", B(bwd_base(), [](fa2_bwd_args& a) { with_bias(a, FA2_F16); }));
  bwd("bias_f32", B(bwd_base(), [](fa2_bwd_args& a) { with_bias(a, FA2_F32); }));
  bwd("bias_bf16_unaligned", B(bwd_base(), [](fa2_bwd_args& a) { with_bias(a, FA2_BF16); }), 6, nullptr, false);
  bwd("mqa_workspace", B(bwd_base(4096, 32, 1), [](fa2_bwd_args& a) { a.dkv_workspace = (float*)kPtr; }));
  bwd("mqa_no_workspace", bwd_base(4096, 32, 1));
  bwd("local_left64", B(bwd_base(), [](fa2_bwd_args& a) { a.local = 1, a.window_left = 64; }));
  bwd("local_left64", B(bwd_base(), [](fa2_bwd_args& a) { a.local = 1, a.window_left = 64; }), 7);
  bwd("local_left64_causal", B(bwd_base(), [](fa2_bwd_args& a) { a.local = 1, a.window_left = 64, a.causal = 1; }), 7);
  bwd("base", bwd_base(), 1);
  bwd("bias_dbias", B(bwd_base(), [](fa2_bwd_args& a) { with_bias(a, FA2_BF16), a.dbias = (float*)kPtr; }), 14);
  bwd("bias_dbias_sk0", B(bwd_base(0), [](fa2_bwd_args& a) { with_bias(a, FA2_BF16), a.dbias = (float*)kPtr; }), 8);

  const fa2_policy cap2 = {0, 2}, cap300 = {0, 300}, cap64 = {0, 64};
  printf("hp_grid items=8 cap=0: %d\n", hp_grid(8, 256, nullptr));
  printf("hp_grid items=8 cap=2: %d\n", hp_grid(8, 256, &cap2));
  printf("hp_grid items=1000 cap=0: %d\n", hp_grid(1000, 256, nullptr));
  printf("hp_grid items=1000 cap=300: %d\n", hp_grid(1000, 256, &cap300));
  printf("hp_grid items=1000 cap=64: %d\n", hp_grid(1000, 256, &cap64));
  return 0;
}
