"""CPU tests of shared-prefix (cascade) decode attention (fa2_fwd_kvcache_prefix, added within ABI 10
minor 1 and detected by the symbol): the header, the ctypes mirror and the Python signature agree;
bad arguments are rejected before any tensor is touched or any kernel is launched; the workspace is
the stated sum of two regions, each rounded up to 16 bytes; both split counts are at least two and
otherwise those of the plain call of each pass; and the merge kernel's gfx950 code objects exist
beside the unchanged old ones.  No kernel is launched.
"""
import ctypes
import inspect
import re

import pytest
import torch

from fa2_triton_amd import _lib

from tests.test_host import HEADER, _header_struct_fields
from tests.test_kvcache_host import _args as _base_args
from tests.test_kvcache_host import kernels  # noqa: F401  (the descriptor fixture)
from tests.test_kvcache_paged_host import _args as _paged_args

SYMBOLS = ("fa2_fwd_kvcache_prefix", "fa2_prefix_kvcache_num_splits", "fa2_prefix_kvcache_workspace_bytes")
CACHE_FIELDS = ("k_cache", "v_cache", "k_cache_stride", "v_cache_stride", "capacity", "cache_seqlens", "num_splits")


def test_struct_matches_header():
    assert _header_struct_fields("fa2_prefix_kvcache_args") == [f[0] for f in _lib.PrefixKvCacheArgs._fields_] == ["seq", "prefix"]
    types = dict(_lib.PrefixKvCacheArgs._fields_)
    assert types["seq"] is _lib.PagedKvCacheArgs and types["prefix"] is _lib.PagedKvCacheArgs
    # the per-sequence call is the first member, unchanged: its base is a contiguous call's args
    assert _lib.PrefixKvCacheArgs.seq.offset == 0
    assert _lib.PrefixKvCacheArgs.prefix.offset == ctypes.sizeof(_lib.PagedKvCacheArgs)
    assert ctypes.sizeof(_lib.PrefixKvCacheArgs) == 2 * ctypes.sizeof(_lib.PagedKvCacheArgs)


def test_symbols_are_exported_and_bound_and_the_version_stays():
    lib = _lib.load()
    assert lib.fa2_version() == 10 and lib.fa2_abi_minor() == 1 == _lib.ABI_MINOR
    assert int(re.search(r"#define FA2_ABI_MINOR (\d+)", HEADER).group(1)) == 1
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(r"\b%s\(const fa2_prefix_kvcache_args\* args" % sym, HEADER), sym
    assert _lib.PREFIX_KVCACHE_SYMBOL == "fa2_fwd_kvcache_prefix"
    assert lib.fa2_fwd_kvcache_prefix.argtypes[0]._type_ is _lib.PrefixKvCacheArgs
    assert lib.fa2_prefix_kvcache_workspace_bytes.restype is ctypes.c_int64
    assert len(lib.fa2_prefix_kvcache_num_splits.argtypes) == 3


def test_a_library_without_the_symbol_is_refused_by_name(monkeypatch):
    """load() names the missing entry point and the rebuild command; no AttributeError."""

    class Old:  # a library of ABI 10.1 with the paged and fp8 entry points, from before the shared prefix
        def __getattr__(self, name):
            if name.startswith("fa2_") and "prefix" not in name:
                fn = lambda *a: {"fa2_version": 10, "fa2_abi_minor": 1}.get(name, 0)
                object.__setattr__(self, name, fn)
                return fn
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(RuntimeError, match=r"fa2_fwd_kvcache_prefix.*python -m fa2_triton_amd\.build"):
        _lib.load()
    assert _lib._lib is None


def test_python_signature():
    import fa2_triton_amd
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    assert "flash_attn_with_prefix_kvcache" in fa2_triton_amd.__all__
    params = inspect.signature(flash_attn_with_prefix_kvcache).parameters
    assert list(params) == ["q", "prefix_k", "prefix_v", "k_cache", "v_cache", "prefix_seqlen", "cache_seqlens",
                            "prefix_block_table", "block_table", "k", "v", "softmax_scale", "causal", "window_size",
                            "num_splits", "prefix_num_splits", "return_lse"]
    defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(prefix_seqlen=None, cache_seqlens=None, prefix_block_table=None, block_table=None, k=None, v=None,
                            softmax_scale=None, causal=False, window_size=(-1, -1), num_splits=0, prefix_num_splits=0,
                            return_lse=False)
    doc = flash_attn_with_prefix_kvcache.__doc__
    assert "Inference only" in doc and "prefix_block_table" in doc and "left window" in doc and "fp8" in doc


@pytest.mark.parametrize("kw,exc", [
    (dict(window_size=(1,)), ValueError), (dict(window_size=(0, -1)), NotImplementedError),
    (dict(window_size=(100, 0)), NotImplementedError), (dict(num_splits=1), ValueError), (dict(num_splits=129), ValueError),
    (dict(num_splits=-1), ValueError), (dict(num_splits=True), ValueError), (dict(prefix_num_splits=1), ValueError),
    (dict(prefix_num_splits=129), ValueError), (dict(prefix_num_splits=2.0), ValueError), (dict(k=object()), ValueError),
    (dict(v=object()), ValueError), (dict(cache_seqlens=1.5), TypeError), (dict(prefix_seqlen=1.5), TypeError),
    (dict(prefix_seqlen=True), TypeError), (dict(block_table=object(), cache_seqlens=None), TypeError)])
def test_bad_arguments_raise_before_a_tensor_is_touched(kw, exc):
    from fa2_triton_amd import flash_attn_with_prefix_kvcache

    with pytest.raises(exc):
        flash_attn_with_prefix_kvcache(None, None, None, None, None, **kw)


def test_left_window_and_one_split_are_named():
    from fa2_triton_amd import flash_attn_with_prefix_kvcache as prefix

    with pytest.raises(NotImplementedError, match="window_size"):
        prefix(None, None, None, None, None, window_size=(5, -1))
    with pytest.raises(ValueError, match=r"^num_splits = 1.*fp32 partial"):
        prefix(None, None, None, None, None, num_splits=1)
    with pytest.raises(ValueError, match=r"^prefix_num_splits = 1.*fp32 partial"):
        prefix(None, None, None, None, None, prefix_num_splits=1)


def test_tensor_checks_on_cpu_tensors():
    from fa2_triton_amd import flash_attn_with_prefix_kvcache as prefix

    bf = torch.bfloat16
    q, kc, pk = torch.zeros(2, 1, 4, 64, dtype=bf), torch.zeros(2, 16, 2, 64, dtype=bf), torch.zeros(1, 32, 2, 64, dtype=bf)
    pool, table = torch.zeros(6, 16, 2, 64, dtype=bf), torch.zeros(2, 3, dtype=torch.int32)
    for name, args in (("prefix_k", (pk.to(torch.float8_e4m3fn), pk, kc, kc)), ("prefix_v", (pk, pk.to(torch.float8_e4m3fn), kc, kc)),
                       ("k_cache", (pk, pk, kc.to(torch.float8_e4m3fn), kc)), ("v_cache", (pk, pk, kc, kc.to(torch.float8_e5m2)))):
        with pytest.raises(NotImplementedError, match=name + r" is torch\.float8.*fp8"):
            prefix(q, *args)
    with pytest.raises(ValueError, match=r"prefix_k must be a 4-d tensor \[1, cap_p"):  # prefix_k with batch 2
        prefix(q, kc, kc, kc, kc)
    with pytest.raises(ValueError, match=r"prefix_v must be a 4-d tensor \[1, cap_p"):
        prefix(q, pk, kc, kc, kc)
    with pytest.raises(ValueError, match=r"prefix_k must be a 4-d"):
        prefix(q, pk[0], pk, kc, kc)
    with pytest.raises(ValueError, match="k and v"):
        prefix(q, pk, pk, kc, kc, k=kc[:, :1])
    with pytest.raises(ValueError, match="seqlen_new"):
        prefix(q, pk, pk, kc, kc, k=kc[:, :1, :1], v=kc[:, :1, :1])
    with pytest.raises(ValueError, match="q must be a 4-d"):
        prefix(q[0], pk, pk, kc, kc)
    with pytest.raises(ValueError, match="block_table must be a 2-d"):
        prefix(q, pk, pk, pool, pool, block_table=table[0], cache_seqlens=5)
    with pytest.raises(ValueError, match="prefix_block_table must be a 2-d"):
        prefix(q, pool, pool, kc, kc, prefix_block_table=table[0])
    with pytest.raises(ValueError, match="GPU"):  # everything else is in order: the device is checked last
        prefix(q, pk, pk, kc, kc)
    with pytest.raises(ValueError, match="GPU"):
        prefix(q, pool, pool, pool, pool, prefix_block_table=table[:1], block_table=table, cache_seqlens=5)


def _prefix_side(paged=False, **kw):
    """The prefix of a valid call: [1, 4096, 8, 128] contiguous, or 64 pages of 64 keys, on
    never-dereferenced pointers; every field the library derives is zero."""
    side = _lib.PagedKvCacheArgs()
    side.base.k_cache = side.base.v_cache = 4096
    side.base.capacity = 4096
    for name in ("k_cache_stride", "v_cache_stride"):
        getattr(side.base, name)[:] = (64 * 8 * 128, 8 * 128, 128) if paged else (4096 * 8 * 128, 8 * 128, 128)
    if paged:
        side.block_table, side.block_table_stride, side.page_block_size, side.num_blocks = 4096, 64, 64, 1000
    for key, val in kw.items():
        setattr(side if key in ("block_table", "block_table_stride", "page_block_size", "num_blocks") else side.base, key, val)
    return side


def _args(seq=None, prefix=None, paged=False, prefix_paged=False, workspace=True):
    """A valid cascade call: B = 1, Hq = 32, Hkv = 8, Sq = 1, cap = 8192, D = 128, bf16."""
    a = _lib.PrefixKvCacheArgs()
    a.seq = _paged_args(**(seq or {})) if paged else _lib.PagedKvCacheArgs(base=_base_args(**(seq or {})))
    a.prefix = _prefix_side(prefix_paged, **(prefix or {}))
    if workspace and not a.seq.base.workspace:
        a.seq.base.workspace, a.seq.base.workspace_bytes = 4096, 1 << 40
    return a


def test_a_valid_call_passes_validation_up_to_the_counts():
    lib = _lib.load()
    for paged in (False, True):
        for prefix_paged in (False, True):
            a = _args(paged=paged, prefix_paged=prefix_paged)
            np_, ns = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.fa2_prefix_kvcache_num_splits(ctypes.byref(a), ctypes.byref(np_), ctypes.byref(ns)) == _lib.FA2_OK
            assert np_.value >= 2 and ns.value >= 2
            assert lib.fa2_prefix_kvcache_workspace_bytes(ctypes.byref(a)) == (np_.value + ns.value) * 32 * 129 * 4


REJECTED = [
    # (seq fields, prefix fields, status, text)
    (dict(window_left=0), {}, _lib.FA2_E_UNSUPPORTED, b"window_left"),
    (dict(window_left=100, causal=1), {}, _lib.FA2_E_UNSUPPORTED, b"window_left"),
    (dict(num_splits=1), {}, _lib.FA2_E_INVALID, b"num_splits=1 (seq)"),
    ({}, dict(num_splits=1), _lib.FA2_E_INVALID, b"num_splits=1 (prefix)"),
    (dict(num_splits=129), {}, _lib.FA2_E_INVALID, b"num_splits"),
    ({}, dict(num_splits=129), _lib.FA2_E_INVALID, b"num_splits"),
    ({}, dict(num_splits=-1), _lib.FA2_E_INVALID, b"num_splits"),
    (dict(workspace=None, workspace_bytes=0), {}, _lib.FA2_E_INVALID, b"workspace"),                 # none given
    (dict(workspace=4096, workspace_bytes=1000), {}, _lib.FA2_E_INVALID, b"workspace"),              # too small
    (dict(workspace=4100, workspace_bytes=1 << 30), {}, _lib.FA2_E_INVALID, b"aligned"),
    # a field of `prefix` that the library derives
    ({}, dict(q=4096), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(o=4096), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(k_new=4096), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(workspace=4096), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(batch=1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(heads_kv=8), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(seqlen_q=1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(head_dim=128), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(seqlen_new=1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(causal=1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(window_left=-1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(window_right=-1), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(dtype=_lib.FA2_BF16), _lib.FA2_E_INVALID, b"prefix"),
    ({}, dict(softmax_scale=0.5), _lib.FA2_E_INVALID, b"prefix"),
    # what both sides check as the plain calls do
    ({}, dict(capacity=0), _lib.FA2_E_INVALID, b"sizes"),
    ({}, dict(k_cache=None), _lib.FA2_E_INVALID, b"null"),
    ({}, dict(v_cache=4104), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(q=None), {}, _lib.FA2_E_INVALID, b"null"),
    (dict(heads_q=30), {}, _lib.FA2_E_INVALID, b"divisible"),
    (dict(head_dim=100), {}, _lib.FA2_E_UNSUPPORTED, b"multiple of 8"),
    (dict(k_new=4096, seqlen_new=1), {}, _lib.FA2_E_INVALID, b"together"),
    (dict(batch=1 << 13, seqlen_q=1 << 12), {}, _lib.FA2_E_UNSUPPORTED, b"2^24"),
]


@pytest.mark.parametrize("seq,prefix,code,text", REJECTED,
                         ids=[",".join(list(r[0]) + ["prefix." + k for k in r[1]]) + f"-{i}" for i, r in enumerate(REJECTED)])
def test_library_rejects_without_a_gpu(seq, prefix, code, text):
    lib = _lib.load()
    a = _args(seq=seq, prefix=prefix, workspace="workspace" not in seq)
    assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == code
    assert text in lib.fa2_last_error(), lib.fa2_last_error()
    assert lib.fa2_fwd_kvcache_prefix(None, None) == _lib.FA2_E_INVALID


def test_prefix_strides_and_the_paging_fields_are_checked():
    lib = _lib.load()
    for stride in ("q_stride", "o_stride", "k_new_stride", "v_new_stride"):  # derived: must be zero
        a = _args()
        getattr(a.prefix.base, stride)[1] = 8
        assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and b"prefix" in lib.fa2_last_error()
    for kw, text in ((dict(page_block_size=48), b"power of two"), (dict(num_blocks=0), b"num_blocks"),
                     (dict(block_table_stride=63), b"block_table_stride"), (dict(capacity=4096 + 8), b"max_blocks * page_block_size")):
        a = _args(prefix=kw, prefix_paged=True)
        assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and text in lib.fa2_last_error(), kw
    a = _args(seq=dict(block_table_stride=511), paged=True)
    assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and b"block_table_stride" in lib.fa2_last_error()


def test_q_must_collapse_to_one_batch_row():
    """Sq = 1: the batch stride is the row stride, whatever it is.  Sq > 1: q_stride[0] must be
    Sq * q_stride[1] unless B = 1.  (A call that passes here fails next at the null stream's launch,
    which no CPU test may reach: the accepted forms are checked through a missing k_cache.)"""
    lib = _lib.load()
    a = _args(seq=dict(batch=3, seqlen_q=2))
    a.seq.base.q_stride[:] = (4 * 32 * 128, 32 * 128, 128)
    assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_UNSUPPORTED
    assert b"q_stride" in lib.fa2_last_error() and b"collapse" in lib.fa2_last_error()
    for batch, sq, stride0 in ((3, 2, 2 * 32 * 128), (1, 2, 12345 * 8), (3, 1, 3 * 32 * 128 + 64)):
        a = _args(seq=dict(batch=batch, seqlen_q=sq, k_cache=None))
        a.seq.base.q_stride[:] = (stride0, 32 * 128, 128)
        assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and b"null" in lib.fa2_last_error()


def test_status_codes_map_to_the_same_exceptions():
    lib = _lib.load()
    with pytest.raises(NotImplementedError, match="window_left"):
        _lib.check(lib.fa2_fwd_kvcache_prefix(ctypes.byref(_args(seq=dict(window_left=4))), None))
    with pytest.raises(ValueError, match="num_splits=1"):
        _lib.check(lib.fa2_fwd_kvcache_prefix(ctypes.byref(_args(prefix=dict(num_splits=1))), None))


def _round16(n):
    return (n + 15) // 16 * 16


def test_workspace_is_two_regions_each_rounded_to_16_bytes():
    lib = _lib.load()
    bites = 0
    for b, hq, hkv, sq, d, ns_p, ns_s in [(1, 32, 8, 1, 128, 2, 2), (3, 5, 1, 1, 96, 3, 2), (1, 1, 1, 1, 96, 3, 5), (3, 3, 3, 1, 32, 3, 2),
                                          (5, 3, 1, 3, 64, 7, 9), (2, 8, 8, 2, 256, 128, 128), (1, 7, 7, 1, 8, 3, 3)]:
        a = _args(seq=dict(batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, head_dim=d, num_splits=ns_s), prefix=dict(num_splits=ns_p))
        rows = b * hq * sq
        region_p, region_s = ns_p * rows * (d + 1) * 4, ns_s * rows * (d + 1) * 4
        assert lib.fa2_prefix_kvcache_workspace_bytes(ctypes.byref(a)) == _round16(region_p) + _round16(region_s), (b, hq, sq, d)
        bites += region_p % 16 != 0
        np_, ns = ctypes.c_int(), ctypes.c_int()
        assert lib.fa2_prefix_kvcache_num_splits(ctypes.byref(a), ctypes.byref(np_), ctypes.byref(ns)) == 0
        assert (np_.value, ns.value) == (ns_p, ns_s)
        # one byte short of the sum is refused, the sum itself passes the workspace check
        a.seq.base.workspace_bytes = _round16(region_p) + _round16(region_s) - 1
        a.seq.base.k_cache = None
        a.seq.base.q_stride[:] = (sq * hq * d, hq * d, d)
        assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and b"workspace" in lib.fa2_last_error()
        a.seq.base.workspace_bytes += 1
        assert lib.fa2_fwd_kvcache_prefix(ctypes.byref(a), None) == _lib.FA2_E_INVALID and b"null" in lib.fa2_last_error()
    assert bites >= 4  # D = 96, B * Hq * Sq odd, ns_p = 3 among them: the prefix region ends off a 16-byte boundary
    # rejected sizes: no workspace, counts 0, the status of the call
    bad = _args(seq=dict(window_left=3))
    np_, ns = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.fa2_prefix_kvcache_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.fa2_prefix_kvcache_num_splits(ctypes.byref(bad), ctypes.byref(np_), ctypes.byref(ns)) == _lib.FA2_E_UNSUPPORTED
    assert (np_.value, ns.value) == (0, 0)
    assert lib.fa2_prefix_kvcache_workspace_bytes(None) == 0
    assert lib.fa2_prefix_kvcache_num_splits(None, None, None) == _lib.FA2_E_INVALID
    assert lib.fa2_prefix_kvcache_num_splits(ctypes.byref(_args()), None, None) == 0  # either pointer may be NULL


def test_split_counts_are_at_least_two_and_else_those_of_the_plain_calls():
    lib = _lib.load()
    seen_p, seen_s = set(), set()
    for b in (1, 3, 8, 64):
        for hq, hkv in ((32, 8), (8, 8), (16, 1)):
            for sq in (1, 3):
                for cap, cap_p in ((256, 8192), (8192, 256), (1 << 20, 1 << 20), (64, 64)):
                    for forced_s, forced_p in ((0, 0), (2, 7), (128, 0), (0, 5)):
                        for paged in (False, True):
                            kw = dict(batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, capacity=cap, num_splits=forced_s)
                            a = _args(seq=dict(kw, **(dict(block_table_stride=cap // 16) if paged else {})),
                                      prefix=dict(capacity=cap_p, num_splits=forced_p), paged=paged)
                            np_, ns = ctypes.c_int(), ctypes.c_int()
                            assert lib.fa2_prefix_kvcache_num_splits(ctypes.byref(a), ctypes.byref(np_), ctypes.byref(ns)) == 0
                            plain_s = _base_args(**kw)
                            plain_p = _base_args(**dict(kw, batch=1, seqlen_q=b * sq, capacity=cap_p, num_splits=forced_p))
                            assert ns.value == max(2, lib.fa2_kvcache_num_splits(ctypes.byref(plain_s))), kw
                            assert np_.value == max(2, lib.fa2_kvcache_num_splits(ctypes.byref(plain_p))), (kw, cap_p)
                            assert 2 <= np_.value <= 128 and 2 <= ns.value <= 128
                            seen_p.add(np_.value)
                            seen_s.add(ns.value)
    # the grid reaches the floor of two, the heuristic above it and the forced counts
    assert {2, 5, 7} <= seen_p and {2, 128} <= seen_s and len(seen_p) > 5 and len(seen_s) > 4


def test_merge_kernels_exist_and_the_old_counts_stay(kernels):  # noqa: F811
    merge = {k: v for k, v in kernels.items() if "kvprefix_merge_kernel" in k}
    assert sorted(merge) == ["_ZN3fa221kvprefix_merge_kernelILb0EEEv16fa2_kvcache_argsPKfiS3_i",
                             "_ZN3fa221kvprefix_merge_kernelILb1EEEv16fa2_kvcache_argsPKfiS3_i"], sorted(merge)
    for k, (scratch, vgprs, lds) in merge.items():
        assert scratch == 0 and lds == 0 and vgprs <= 64, (k, scratch, vgprs, lds)
    # the counts the other host tests assert, unchanged
    assert len([k for k in kernels if re.match(r"_ZN3fa220kvcache_split_kernelILb[01]ELi\d+EEEv16fa2_kvcache_argsi$", k)]) == 8
    assert len([k for k in kernels
                if re.match(r"_ZN3fa226kvcache_paged_split_kernelILb[01]ELi\d+EEEv22fa2_paged_kvcache_argsi$", k)]) == 8
    assert len([k for k in kernels if "kvcache_combine_kernel" in k]) == 2
    assert len([k for k in kernels if "kvcache_append_kernel" in k]) == 1
    assert len([k for k in kernels if "kvcache_paged_append_kernel" in k]) == 1
    assert len([k for k in kernels if "kvcache_fp8_split_kernel" in k]) == 8
    for k in merge:  # patterns other tests count kernels by
        assert not any(s in k for s in ("kvcache_combine_kernel", "kvcache_append_kernel", "kvcache_split_kernel",
                                        "kvcache_paged_split_kernel", "kvcache_fp8_", "_local_kernel", "dbias_kernel",
                                        "fwd_kernel", "dq_kernel", "dkdv_kernel")), k
