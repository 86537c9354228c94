// api.hip -- the C ABI (include/fa2_amd.h): argument validation, kernel selection, errors.
//
// Validation mirrors the reference callers' asserts (/root/reference/src/forward/caller.py:27-41,
// /root/reference/src/backward/caller.py:30-53) and error types (src/utils.py:57-109); the
// Python layer re-raises our codes as the reference's exception types.
#include <stdarg.h>
#include <stdio.h>

#include "fa2_internal.h"
#if FA2_HP_STAMPS
#include "common.h"
#endif

namespace {

thread_local char g_err[512] = "";

// Every launching entry point takes the address of the error string, the library's one
// thread-local.  Built as this library is (-fPIC, shared, general-dynamic TLS without descriptors)
// that is a __tls_get_addr call, which the empty asm keeps alive; under another TLS model the line
// compiles to nothing.  With glibc older than 2.39 (BZ 19924) every __tls_get_addr of a thread, the
// HIP runtime's and the caller's too, takes the slow path from the dlopen of a module with
// thread-locals until the thread has looked up those of the newest one, usually this library.
// Measured with glibc 2.35, decode at (B, L) = (1, 8192), event time per synchronous call in fresh
// processes: 47.8 / 47.9 / 48.3 us without this lookup, 45.6 / 45.7 / 45.6 us with it.
inline void touch_thread_state() { asm volatile("" ::"r"(&g_err[0])); }

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_status(hipError_t e, const char* entry, const char* what) {
  if (e == hipSuccess) return FA2_OK;
  return fail(FA2_E_HIP, "%s %s: %s", entry, what, hipGetErrorString(e));
}

using fa2::head_dim_tile;

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }
bool strides8(const int64_t* s) { return s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0; }

// 16-byte vector path: every row of every 16-bit tensor starts on a 16-byte boundary.
bool vec_ok(int d, const void* ptr, const int64_t* s) { return d % 8 == 0 && aligned16(ptr) && strides8(s); }

int check_common(int B, int Hq, int Hkv, int Sq, int Sk, int D, int dtype, int lse_rs,
                 const int32_t* cu, float p) {
  if (B < 1 || Hq < 1 || Hkv < 1 || Sq < 0 || Sk < 0 || D < 1)
    return fail(FA2_E_INVALID, "bad sizes B=%d Hq=%d Hkv=%d Sq=%d Sk=%d D=%d", B, Hq, Hkv, Sq, Sk, D);
  if (Hq % Hkv != 0) return fail(FA2_E_INVALID, "heads_q=%d is not divisible by heads_kv=%d", Hq, Hkv);
  if (dtype != FA2_F16 && dtype != FA2_BF16) return fail(FA2_E_INVALID, "dtype %d: only fp16 and bf16", dtype);
  if (!head_dim_tile(D)) return fail(FA2_E_UNSUPPORTED, "head_dim %d > 256", D);
  if (lse_rs < ((Sq + 31) / 32) * 32 || lse_rs % 32 != 0)
    return fail(FA2_E_INVALID, "lse_row_stride %d must be a multiple of 32 and >= seqlen_q rounded up (%d)", lse_rs, Sq);
  if (cu && Sq != Sk) return fail(FA2_E_INVALID, "varlen (cu_seqlens) requires seqlen_q == seqlen_k");
  if (!(p >= 0.f && p < 1.f)) return fail(FA2_E_INVALID, "dropout_p=%f must be in [0, 1)", p);
  return FA2_OK;
}

// The sliding window of a call (ABI 10) in normal form, on the library's own copy of the args:
// causal forces right = 0; a window with no bound is no window; one that bounds only the right
// side at 0 is the causal mask.  What stays local has left >= 0 or right > 0 (negative = no
// bound); what does not launches exactly the kernels of the same call without a window.
template <typename Args>
void normalise_window(Args& n) {
  if (n.local) {
    const int left = n.window_left < 0 ? -1 : n.window_left;
    const int right = n.causal ? 0 : (n.window_right < 0 ? -1 : n.window_right);
    if (left < 0 && right < 0) {
      n.local = 0;
    } else if (left < 0 && right == 0) {
      n.local = 0;
      n.causal = 1;
    } else {
      n.local = 1;
      n.window_left = left;
      n.window_right = right;
    }
  }
  if (!n.local) n.window_left = n.window_right = 0;
}

// The sizes, dtype and split count of a KV-cache call: what fa2_kvcache_num_splits and
// fa2_kvcache_workspace_bytes need to be meaningful, checked before anything else.
int kvcache_check_sizes(const fa2_kvcache_args* a) {
  if (a->batch < 1 || a->heads_q < 1 || a->heads_kv < 1 || a->seqlen_q < 1 || a->capacity < 1 || a->head_dim < 1 ||
      a->seqlen_new < 0)
    return fail(FA2_E_INVALID, "bad sizes B=%d Hq=%d Hkv=%d Sq=%d capacity=%d D=%d seqlen_new=%d", a->batch, a->heads_q,
                a->heads_kv, a->seqlen_q, a->capacity, a->head_dim, a->seqlen_new);
  if (a->heads_q % a->heads_kv != 0)
    return fail(FA2_E_INVALID, "heads_q=%d is not divisible by heads_kv=%d", a->heads_q, a->heads_kv);
  if (a->dtype != FA2_F16 && a->dtype != FA2_BF16) return fail(FA2_E_INVALID, "dtype %d: only fp16 and bf16", a->dtype);
  if (!head_dim_tile(a->head_dim)) return fail(FA2_E_UNSUPPORTED, "head_dim %d > 256", a->head_dim);
  if (a->capacity > (1 << 30) || a->seqlen_q > (1 << 24))
    return fail(FA2_E_UNSUPPORTED, "capacity %d > 2^30 or seqlen_q %d > 2^24", a->capacity, a->seqlen_q);
  if (a->num_splits < 0 || a->num_splits > FA2_KVCACHE_MAX_SPLITS)
    return fail(FA2_E_INVALID, "num_splits=%d must be in 0 .. %d", a->num_splits, FA2_KVCACHE_MAX_SPLITS);
  return FA2_OK;
}

int check_policy(const fa2_policy* p) {
  if (!p) return FA2_OK;
  if (p->disable & ~(uint32_t)(FA2_PATH_FWD_HP | FA2_PATH_DQ_HP | FA2_PATH_DKDV_HP))
    return fail(FA2_E_INVALID, "unknown path bits 0x%x", p->disable);
  if (p->grid_cap < 0) return fail(FA2_E_INVALID, "grid_cap %d < 0", p->grid_cap);
  return FA2_OK;
}

// Everything fa2_fwd_kvcache checks after the sizes, shared with the paged call (whose pools are
// k_cache / v_cache with block, row and head strides): pointers, the new rows, 16-byte rows, the
// workspace and the grid.  On success *nsplit_out is the split count of the call.
// fp8: the caches hold bytes (fa2_fwd_kvcache_fp8): head_dim a multiple of 16 and cache strides of 16.
int kvcache_check_call(const fa2_kvcache_args* a, int* nsplit_out, bool fp8) {
  if (!a->q || !a->k_cache || !a->v_cache || !a->o) return fail(FA2_E_INVALID, "null tensor pointer");
  if ((a->k_new != nullptr) != (a->v_new != nullptr)) return fail(FA2_E_INVALID, "k_new and v_new must be given together");
  if (a->k_new ? a->seqlen_new < 1 : a->seqlen_new != 0)
    return fail(FA2_E_INVALID, "seqlen_new=%d %s k_new / v_new", a->seqlen_new, a->k_new ? "with" : "without");
  const int D = a->head_dim;
  if (D % (fp8 ? 16 : 8) != 0)
    return fail(FA2_E_UNSUPPORTED, "head_dim %d is not a multiple of %d (16-byte rows)", D, fp8 ? 16 : 8);
  bool aligned = vec_ok(D, a->q, a->q_stride) && vec_ok(D, a->o, a->o_stride);
  if (fp8) aligned = aligned && fa2::fp8_rows16(a->k_cache, a->k_cache_stride) && fa2::fp8_rows16(a->v_cache, a->v_cache_stride);
  else aligned = aligned && vec_ok(D, a->k_cache, a->k_cache_stride) && vec_ok(D, a->v_cache, a->v_cache_stride);
  if (a->k_new) aligned = aligned && vec_ok(D, a->k_new, a->k_new_stride) && vec_ok(D, a->v_new, a->v_new_stride);
  if (!aligned) return fail(FA2_E_UNSUPPORTED, "a tensor's rows are not 16-byte aligned (pointer or strides)");
  const int nsplit = fa2_kvcache_num_splits(a);
  const int64_t need = fa2::kv_workspace_bytes(*a, nsplit);
  if (need > 0) {
    if (!a->workspace || a->workspace_bytes < need)
      return fail(FA2_E_INVALID, "workspace_bytes %lld < %lld required for %d splits",
                  (long long)(a->workspace ? a->workspace_bytes : 0), (long long)need, nsplit);
    if (!aligned16(a->workspace)) return fail(FA2_E_INVALID, "workspace must be 16-byte aligned");
  }
  if (fa2::kv_units(*a) * nsplit > 0x7FFFFFFFll) return fail(FA2_E_UNSUPPORTED, "grid of %lld units x %d splits", (long long)fa2::kv_units(*a), nsplit);
  *nsplit_out = nsplit;
  return FA2_OK;
}

// A decode call (Args = fa2_kvcache_args, fa2_paged_kvcache_args or fa2_fp8_kvcache_args, its sizes
// and what only its entry point checks done): the shared checks, then the append, the split kernel
// and the combination.  fp8 caches have kernels of their own tiles, per layout.
template <typename Args>
int run_kvcache(const Args& args, const char* entry, void* stream) {
  constexpr bool fp8 = std::is_same_v<Args, fa2_fp8_kvcache_args>;
  const fa2_kvcache_args& a = fa2::kv_base(args);
  int nsplit = 1;
  if (int rc = kvcache_check_call(&a, &nsplit, fp8)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (a.k_new)
    if (int rc = hip_status(fa2::launch_kvcache_append(args, st), entry, "append launch")) return rc;
  hipError_t e;
  if constexpr (fp8)
    e = fa2::dispatch(
        [&](auto bf, auto dt, auto paged) { return fa2::launch_kvcache_split<bf.value, dt.value, Args, paged.value>(args, nsplit, st); },
        a.dtype == FA2_BF16, fa2::dtypes{}, fa2::fp8_head_dim_tile(a.head_dim), fa2::fp8_tiles{}, fa2::fp8_paged(args), fa2::bools{});
  else
    e = fa2::dispatch([&](auto bf, auto dt) { return fa2::launch_kvcache_split<bf.value, dt.value>(args, nsplit, st); },
                      a.dtype == FA2_BF16, fa2::dtypes{}, head_dim_tile(a.head_dim), fa2::tiles{});
  if (int rc = hip_status(e, entry, "launch")) return rc;
  if (nsplit > 1) return hip_status(fa2::launch_kvcache_combine(a, nsplit, st), entry, "combine launch");
  return FA2_OK;
}

// The sizes of a paged call: kvcache_check_sizes on the base, then the page size and the table
// geometry (max_blocks is capacity / page_block_size).
int paged_kvcache_check_sizes(const fa2_paged_kvcache_args* a) {
  if (int rc = kvcache_check_sizes(&a->base)) return rc;
  const int P = a->page_block_size;
  if (P < 16 || (P & (P - 1)) != 0) return fail(FA2_E_INVALID, "page_block_size=%d must be a power of two >= 16", P);
  if (a->num_blocks < 1) return fail(FA2_E_INVALID, "num_blocks=%d must be >= 1", a->num_blocks);
  if (a->base.capacity % P != 0)
    return fail(FA2_E_INVALID, "capacity=%d must be max_blocks * page_block_size (a multiple of %d)", a->base.capacity, P);
  return FA2_OK;
}

// fp8 caches: the sizes of the base call (with a block table, of the paged call), then the head
// dim the fp8 kernels cover.
int fp8_kvcache_check_sizes(const fa2_fp8_kvcache_args* a) {
  if (int rc = fa2::fp8_paged(*a) ? paged_kvcache_check_sizes(&a->paged) : kvcache_check_sizes(&a->paged.base)) return rc;
  if (!fa2::fp8_head_dim_tile(a->paged.base.head_dim))
    return fail(FA2_E_UNSUPPORTED, "head_dim %d > %d with fp8 caches", a->paged.base.head_dim, fa2::kFp8MaxHeadDim);
  return FA2_OK;
}

// A block table's rows hold the max_blocks = capacity / page_block_size entries a batch can address.
int check_table_stride(const fa2_paged_kvcache_args* a) {
  const int64_t max_blocks = a->base.capacity / a->page_block_size;
  if (a->block_table_stride < max_blocks)
    return fail(FA2_E_INVALID, "block_table_stride %lld < max_blocks %lld (capacity / page_block_size)",
                (long long)a->block_table_stride, (long long)max_blocks);
  return FA2_OK;
}

// Shared-prefix decode (fa2_fwd_kvcache_prefix): what the call runs, derived from the
// sizes alone.  `prefix` is the prefix pass as the split kernel of its layout takes it: batch 1,
// seqlen_q = B * Sq, no mask, no append; `seq` the per-sequence pass with its split count forced.
// The pointers that depend on the call (q's row stride, the workspace regions) are filled in by
// fa2_fwd_kvcache_prefix.
struct PrefixPlan {
  fa2_paged_kvcache_args prefix, seq;
  int ns_p, ns_s;
  int64_t region_p, region_s;  // bytes of the two workspace regions, each a multiple of 16
};

int check_sizes_of_layout(const fa2_paged_kvcache_args* a) {
  return a->block_table ? paged_kvcache_check_sizes(a) : kvcache_check_sizes(&a->base);
}

// a pass always hands over fp32 partials: at least two splits (kvcache_kernel_body.h writes a
// rounded O with one)
int prefix_pass_splits(const fa2_kvcache_args& a) {
  const int n = a.num_splits >= 1 ? a.num_splits : fa2::kv_auto_splits(a, fa2::device_cu_count());
  return n < 2 ? 2 : n;
}

int prefix_kvcache_plan(const fa2_prefix_kvcache_args* args, PrefixPlan* plan) {
  const fa2_kvcache_args& s = args->seq.base;
  const fa2_kvcache_args& x = args->prefix.base;
  if (int rc = check_sizes_of_layout(&args->seq)) return rc;
  if (s.window_left >= 0)
    return fail(FA2_E_UNSUPPORTED, "window_left=%d: a left window bound is not supported with a shared prefix", s.window_left);
  if (s.num_splits == 1 || x.num_splits == 1)
    return fail(FA2_E_INVALID, "num_splits=1 (%s): both passes hand fp32 partial results to the merge, which a pass with one "
                "split does not write; force 2 .. %d or pass 0", s.num_splits == 1 ? "seq" : "prefix", FA2_KVCACHE_MAX_SPLITS);
  const bool zero = !x.q && !x.o && !x.lse && !x.k_new && !x.v_new && !x.workspace && !x.workspace_bytes && !x.batch &&
                    !x.heads_q && !x.heads_kv && !x.seqlen_q && !x.head_dim && !x.seqlen_new && !x.causal && !x.window_left &&
                    !x.window_right && !x.dtype && x.softmax_scale == 0.f;
  bool zero_strides = true;
  for (const int64_t* st : {x.q_stride, x.o_stride, x.k_new_stride, x.v_new_stride})
    zero_strides = zero_strides && !st[0] && !st[1] && !st[2];
  if (!zero || !zero_strides)
    return fail(FA2_E_INVALID, "a field of `prefix` other than the caches, their strides, capacity, cache_seqlens, the paging "
                "fields and num_splits is not zero");
  const int64_t rows = (int64_t)s.batch * s.seqlen_q;
  if (rows > (1 << 24)) return fail(FA2_E_UNSUPPORTED, "batch * seqlen_q = %lld > 2^24", (long long)rows);
  plan->prefix = args->prefix;
  fa2_kvcache_args& p = plan->prefix.base;
  p.batch = 1;
  p.heads_q = s.heads_q;
  p.heads_kv = s.heads_kv;
  p.seqlen_q = (int32_t)rows;
  p.head_dim = s.head_dim;
  p.window_left = p.window_right = -1;
  p.dtype = s.dtype;
  p.softmax_scale = s.softmax_scale;
  if (int rc = check_sizes_of_layout(&plan->prefix)) return rc;
  plan->seq = args->seq;
  plan->ns_p = p.num_splits = prefix_pass_splits(p);
  plan->ns_s = plan->seq.base.num_splits = prefix_pass_splits(s);
  plan->region_p = (fa2::kv_workspace_bytes(p, plan->ns_p) + 15) & ~(int64_t)15;
  plan->region_s = (fa2::kv_workspace_bytes(s, plan->ns_s) + 15) & ~(int64_t)15;
  return FA2_OK;
}
}  // namespace

extern "C" {

int fa2_version(void) { return FA2_ABI_VERSION; }

const char* fa2_last_error(void) { return g_err; }

int fa2_fwd(const fa2_fwd_args* a, void* stream) { return fa2_fwd_ex(a, nullptr, stream); }

int fa2_fwd_ex(const fa2_fwd_args* a, const fa2_policy* policy, void* stream) {
  touch_thread_state();
  if (!a) return fail(FA2_E_INVALID, "null args");
  if (int prc = check_policy(policy)) return prc;
  int rc = check_common(a->batch, a->heads_q, a->heads_kv, a->seqlen_q, a->seqlen_k, a->head_dim, a->dtype,
                        a->lse_row_stride, a->cu_seqlens, a->dropout_p);
  if (rc) return rc;
  // an empty side may come with null pointers (torch gives size-0 tensors data_ptr 0)
  const bool qs = a->seqlen_q > 0, ks = a->seqlen_k > 0;
  if ((qs && (!a->q || !a->o || !a->lse)) || (ks && (!a->k || !a->v))) return fail(FA2_E_INVALID, "null tensor pointer");
  if (a->bias && a->bias_dtype != FA2_F16 && a->bias_dtype != FA2_BF16 && a->bias_dtype != FA2_F32)
    return fail(FA2_E_INVALID, "bias dtype %d", a->bias_dtype);
  fa2_fwd_args norm = *a;
  normalise_window(norm);
  a = &norm;
  if (a->local && (a->bias || a->dropout_p > 0.f))
    return fail(FA2_E_UNSUPPORTED, "sliding window (left %d, right %d) with %s is not implemented", a->window_left,
                a->window_right, a->bias ? "an attention bias" : "dropout");
  if (a->seqlen_q == 0) return FA2_OK;
  const int D = a->head_dim;
  const bool aligned = vec_ok(D, a->q, a->q_stride) && vec_ok(D, a->k, a->k_stride) &&
                       vec_ok(D, a->v, a->v_stride) && vec_ok(D, a->o, a->o_stride);
  const fa2::LaunchCtx ctx = {(hipStream_t)stream, aligned, policy};
  const hipError_t e = fa2::dispatch([&](auto bf, auto dt) { return fa2::launch_fwd_dt<bf.value, dt.value>(*a, ctx); },
                                     a->dtype == FA2_BF16, fa2::dtypes{}, head_dim_tile(D), fa2::tiles{});
  return hip_status(e, "fa2_fwd", "launch");
}

int fa2_bwd_stages(const fa2_bwd_args* a, int stages, void* stream) { return fa2_bwd_stages_ex(a, stages, nullptr, stream); }

int fa2_bwd_stages_ex(const fa2_bwd_args* a, int stages, const fa2_policy* policy, void* stream) {
  touch_thread_state();
  if (!a) return fail(FA2_E_INVALID, "null args");
  if (int prc = check_policy(policy)) return prc;
  int rc = check_common(a->batch, a->heads_q, a->heads_kv, a->seqlen_q, a->seqlen_k, a->head_dim, a->dtype,
                        a->lse_row_stride, a->cu_seqlens, a->dropout_p);
  if (rc) return rc;
  const bool qs = a->seqlen_q > 0, ks = a->seqlen_k > 0;
  if ((qs && (!a->q || !a->o || !a->dout || !a->lse || !a->delta || !a->dq)) || (ks && (!a->k || !a->v || !a->dk || !a->dv)))
    return fail(FA2_E_INVALID, "null tensor pointer");
  if (a->dq_dtype != a->dtype && a->dq_dtype != FA2_F32) return fail(FA2_E_INVALID, "dq dtype %d", a->dq_dtype);
  if (a->bias && a->bias_dtype != FA2_F16 && a->bias_dtype != FA2_BF16 && a->bias_dtype != FA2_F32)
    return fail(FA2_E_INVALID, "bias dtype %d", a->bias_dtype);
  if (stages & ~15) return fail(FA2_E_INVALID, "stage mask %d", stages);
  if (a->dbias && !a->bias) return fail(FA2_E_INVALID, "dbias requested without a bias");
  if ((stages & 8) && !a->dbias) return fail(FA2_E_INVALID, "stage 8 (bias gradient) without a dbias buffer");
  fa2_bwd_args norm = *a;
  normalise_window(norm);
  a = &norm;
  if (a->local && (a->bias || a->dbias || a->dropout_p > 0.f))
    return fail(FA2_E_UNSUPPORTED, "sliding window (left %d, right %d) with %s is not implemented", a->window_left,
                a->window_right, a->dbias ? "a bias gradient" : (a->bias ? "an attention bias" : "dropout"));
  if (a->seqlen_q == 0 && a->seqlen_k == 0) return FA2_OK;  // empty dQ, dK, dV
  const int D = a->head_dim;
  bool aligned = vec_ok(D, a->q, a->q_stride) && vec_ok(D, a->k, a->k_stride) && vec_ok(D, a->v, a->v_stride) &&
                 vec_ok(D, a->o, a->o_stride) && vec_ok(D, a->dout, a->do_stride) &&
                 vec_ok(D, a->dk, a->dk_stride) && vec_ok(D, a->dv, a->dv_stride) &&
                 a->k_stride[1] == a->v_stride[1];  // dq_kernel stages K and V with one offset set
  if (a->dq_dtype == FA2_F32)
    aligned = aligned && aligned16(a->dq) && a->dq_stride[0] % 4 == 0 && a->dq_stride[1] % 4 == 0 && a->dq_stride[2] % 4 == 0;
  else
    aligned = aligned && vec_ok(D, a->dq, a->dq_stride);
  if (a->dkv_workspace) {
    const int64_t need = fa2_bwd_dkv_workspace_bytes(a);
    if (need == 0) return fail(FA2_E_INVALID, "dkv_workspace given but no dK/dV split applies to these sizes");
    if (a->dkv_workspace_bytes < need)
      return fail(FA2_E_INVALID, "dkv_workspace_bytes %lld < %lld required", (long long)a->dkv_workspace_bytes, (long long)need);
    if (!aligned16(a->dkv_workspace)) return fail(FA2_E_INVALID, "dkv_workspace must be 16-byte aligned");
  }
  const fa2::LaunchCtx ctx = {(hipStream_t)stream, aligned, policy};
  const hipError_t e = fa2::dispatch([&](auto bf, auto dt) { return fa2::launch_bwd_dt<bf.value, dt.value>(*a, ctx, stages); },
                                     a->dtype == FA2_BF16, fa2::dtypes{}, head_dim_tile(D), fa2::tiles{});
  return hip_status(e, "fa2_bwd", "launch");
}

int fa2_bwd(const fa2_bwd_args* a, void* stream) { return fa2_bwd_stages(a, a && a->dbias ? 14 : 6, stream); }

int64_t fa2_bwd_dkv_workspace_bytes(const fa2_bwd_args* a) {
  if (!a || a->seqlen_q <= 0 || a->seqlen_k <= 0 || a->head_dim < 1) return 0;
  return fa2::dkv_workspace_bytes(a->batch, a->heads_q, a->heads_kv, a->seqlen_k, a->head_dim);
}

int64_t fa2_dropout_mask_bytes(int32_t batch, int32_t heads_q, int32_t seqlen_q, int32_t seqlen_k) {
  if (batch < 1 || heads_q < 1 || seqlen_q < 1 || seqlen_k < 1) return 0;
  // + one tile of slack: the hand-placed dK/dV reads a wave's two key tiles as one 256-byte run,
  // whose second tile lies past the end when the first is the last of the buffer (ABI 8)
  return (int64_t)batch * heads_q * ((seqlen_q + 31) / 32) * ((seqlen_k + 31) / 32) * 128 + 128;
}

int fa2_cu_seqlens_from_mask(const uint8_t* mask, int64_t mask_row_stride, int32_t batch, int32_t seqlen,
                             int32_t* cu_seqlens, void* stream) {
  if (!mask || !cu_seqlens || batch < 1 || seqlen < 0) return fail(FA2_E_INVALID, "bad cu_seqlens arguments");
  return hip_status(fa2::launch_cu_seqlens(mask, mask_row_stride, batch, seqlen, cu_seqlens, (hipStream_t)stream),
                    "fa2_cu_seqlens_from_mask", "launch");
}

int fa2_abi_minor(void) { return FA2_ABI_MINOR; }

int fa2_kvcache_num_splits(const fa2_kvcache_args* a) {
  if (!a || kvcache_check_sizes(a)) return 1;
  if (a->num_splits >= 1) return a->num_splits;
  return fa2::kv_auto_splits(*a, fa2::device_cu_count());
}

int64_t fa2_kvcache_workspace_bytes(const fa2_kvcache_args* a) {
  if (!a || kvcache_check_sizes(a)) return 0;
  return fa2::kv_workspace_bytes(*a, fa2_kvcache_num_splits(a));
}

int fa2_fwd_kvcache(const fa2_kvcache_args* a, void* stream) {
  touch_thread_state();
  if (!a) return fail(FA2_E_INVALID, "null args");
  if (int rc = kvcache_check_sizes(a)) return rc;
  return run_kvcache(*a, "fa2_fwd_kvcache", stream);
}

int fa2_paged_kvcache_num_splits(const fa2_paged_kvcache_args* a) {
  if (!a || paged_kvcache_check_sizes(a)) return 1;
  return fa2_kvcache_num_splits(&a->base);
}

int64_t fa2_paged_kvcache_workspace_bytes(const fa2_paged_kvcache_args* a) {
  if (!a || paged_kvcache_check_sizes(a)) return 0;
  return fa2_kvcache_workspace_bytes(&a->base);
}

int fa2_fwd_kvcache_paged(const fa2_paged_kvcache_args* a, void* stream) {
  touch_thread_state();
  if (!a) return fail(FA2_E_INVALID, "null args");
  if (int rc = paged_kvcache_check_sizes(a)) return rc;
  if (!a->block_table) return fail(FA2_E_INVALID, "null block_table");
  if (int rc = check_table_stride(a)) return rc;
  return run_kvcache(*a, "fa2_fwd_kvcache_paged", stream);
}

int fa2_fp8_kvcache_num_splits(const fa2_fp8_kvcache_args* a) {
  if (!a || fp8_kvcache_check_sizes(a)) return 1;
  return fa2_kvcache_num_splits(&a->paged.base);
}

int64_t fa2_fp8_kvcache_workspace_bytes(const fa2_fp8_kvcache_args* a) {
  if (!a || fp8_kvcache_check_sizes(a)) return 0;
  return fa2_kvcache_workspace_bytes(&a->paged.base);
}

int fa2_fwd_kvcache_fp8(const fa2_fp8_kvcache_args* args, void* stream) {
  touch_thread_state();
  if (!args) return fail(FA2_E_INVALID, "null args");
  if (int rc = fp8_kvcache_check_sizes(args)) return rc;
  if (fa2::fp8_paged(*args))
    if (int rc = check_table_stride(&args->paged)) return rc;
  if (((uintptr_t)args->k_descale | (uintptr_t)args->v_descale) & 3) return fail(FA2_E_INVALID, "k_descale / v_descale must be 4-byte aligned");
  for (const int64_t* s : {args->k_descale_stride, args->v_descale_stride})
    if (s[0] < 0 || s[1] < 0) return fail(FA2_E_INVALID, "negative descale stride (%lld, %lld)", (long long)s[0], (long long)s[1]);
  return run_kvcache(*args, "fa2_fwd_kvcache_fp8", stream);
}

int fa2_prefix_kvcache_num_splits(const fa2_prefix_kvcache_args* args, int* prefix_splits, int* seq_splits) {
  PrefixPlan plan;
  const int rc = args ? prefix_kvcache_plan(args, &plan) : fail(FA2_E_INVALID, "null args");
  if (prefix_splits) *prefix_splits = rc ? 0 : plan.ns_p;
  if (seq_splits) *seq_splits = rc ? 0 : plan.ns_s;
  return rc;
}

int64_t fa2_prefix_kvcache_workspace_bytes(const fa2_prefix_kvcache_args* args) {
  PrefixPlan plan;
  if (!args || prefix_kvcache_plan(args, &plan)) return 0;
  return plan.region_p + plan.region_s;
}

int fa2_fwd_kvcache_prefix(const fa2_prefix_kvcache_args* args, void* stream) {
  touch_thread_state();
  const char* entry = "fa2_fwd_kvcache_prefix";
  if (!args) return fail(FA2_E_INVALID, "null args");
  PrefixPlan plan;
  if (int rc = prefix_kvcache_plan(args, &plan)) return rc;
  fa2_kvcache_args& s = plan.seq.base;
  fa2_kvcache_args& p = plan.prefix.base;
  for (const fa2_paged_kvcache_args* side : {&plan.seq, &plan.prefix})
    if (side->block_table)
      if (int rc = check_table_stride(side)) return rc;
  // one caller-owned buffer, the prefix region first
  const int64_t need = plan.region_p + plan.region_s;
  if (!s.workspace || s.workspace_bytes < need)
    return fail(FA2_E_INVALID, "workspace_bytes %lld < %lld required for %d prefix + %d sequence splits",
                (long long)(s.workspace ? s.workspace_bytes : 0), (long long)need, plan.ns_p, plan.ns_s);
  if (!aligned16(s.workspace)) return fail(FA2_E_INVALID, "workspace must be 16-byte aligned");
  float* ws_p = (float*)s.workspace;
  float* ws_s = (float*)((char*)s.workspace + plan.region_p);
  // the prefix pass reads q as [1, B * Sq, Hq, D]: row b * Sq + i at (b * Sq + i) * row stride
  int64_t row_stride = s.q_stride[1];
  if (s.seqlen_q == 1) row_stride = s.q_stride[0];
  else if (s.batch > 1 && s.q_stride[0] != s.seqlen_q * s.q_stride[1])
    return fail(FA2_E_UNSUPPORTED, "q_stride[0]=%lld != seqlen_q * q_stride[1]=%lld: q does not collapse to [1, B * Sq, Hq, D]",
                (long long)s.q_stride[0], (long long)(s.seqlen_q * s.q_stride[1]));
  p.q = s.q;
  p.q_stride[0] = row_stride * p.seqlen_q;
  p.q_stride[1] = row_stride;
  p.q_stride[2] = s.q_stride[2];
  p.o = s.o;  // never written: the pass has at least two splits
  for (int i = 0; i < 3; ++i) p.o_stride[i] = s.o_stride[i];
  p.workspace = ws_p;
  p.workspace_bytes = plan.region_p;
  s.workspace = ws_s;
  s.workspace_bytes = plan.region_s;
  // the counts come back as forced: plan.ns_s and plan.ns_p
  int ns_p = 0, ns_s = 0;
  if (int rc = kvcache_check_call(&s, &ns_s, false)) return rc;
  if (int rc = kvcache_check_call(&p, &ns_p, false)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (s.k_new) {
    const hipError_t e = plan.seq.block_table ? fa2::launch_kvcache_append(plan.seq, st) : fa2::launch_kvcache_append(s, st);
    if (int rc = hip_status(e, entry, "append launch")) return rc;
  }
  const auto split_pass = [&](const fa2_paged_kvcache_args& pass, int nsplit) {
    const fa2_kvcache_args& a = pass.base;
    return fa2::dispatch(
        [&](auto bf, auto dt) {
          if (pass.block_table) return fa2::launch_kvcache_split<bf.value, dt.value>(pass, nsplit, st);
          return fa2::launch_kvcache_split<bf.value, dt.value>(a, nsplit, st);
        },
        a.dtype == FA2_BF16, fa2::dtypes{}, head_dim_tile(a.head_dim), fa2::tiles{});
  };
  if (int rc = hip_status(split_pass(plan.prefix, ns_p), entry, "prefix launch")) return rc;
  if (int rc = hip_status(split_pass(plan.seq, ns_s), entry, "launch")) return rc;
  return hip_status(fa2::launch_kvprefix_merge(s, ws_p, ns_p, ws_s, ns_s, st), entry, "merge launch");
}

#if FA2_HP_STAMPS
// development builds only (not part of the C ABI in include/fa2_amd.h): read and clear the
// hand-placed kernels' s_memtime sums
int fa2_debug_hp_stamps(unsigned long long* out16) {
  unsigned long long* b = fa2::hp_stamp_buf();
  if (!b || !out16) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(out16, b, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return hipMemset(b, 0, 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
