"""CPU tests of the paged KV-cache decode path (fa2_fwd_kvcache_paged, added within ABI 10 minor 1
and detected by the symbol): the header, the ctypes mirror and the Python signature agree; bad
arguments are rejected before any tensor is touched or any kernel is launched; the split count and
the workspace are those of the contiguous call on the same shapes; and the new kernels' gfx950 code
objects exist beside the unchanged old ones and keep to the resource rules.  No kernel is launched.
"""
import ctypes
import inspect
import re

import pytest

from fa2_triton_amd import _lib

from tests.test_host import HEADER, _header_struct_fields
from tests.test_kvcache_host import _args as _base_args
from tests.test_kvcache_host import kernels  # noqa: F401  (the descriptor fixture)

SYMBOLS = ("fa2_fwd_kvcache_paged", "fa2_paged_kvcache_num_splits", "fa2_paged_kvcache_workspace_bytes")


def test_struct_matches_header():
    assert _header_struct_fields("fa2_paged_kvcache_args") == [f[0] for f in _lib.PagedKvCacheArgs._fields_]
    types = dict(_lib.PagedKvCacheArgs._fields_)
    assert types["base"] is _lib.KvCacheArgs and types["block_table"] is ctypes.c_void_p
    assert types["block_table_stride"] is ctypes.c_int64
    assert types["page_block_size"] is ctypes.c_int32 and types["num_blocks"] is ctypes.c_int32
    # the base struct is the first member, unchanged: a paged call's base is a contiguous call's args
    assert _lib.PagedKvCacheArgs.base.offset == 0
    assert ctypes.sizeof(_lib.PagedKvCacheArgs) == ctypes.sizeof(_lib.KvCacheArgs) + 24


def test_symbols_are_exported_and_bound_and_the_version_stays():
    lib = _lib.load()
    assert lib.fa2_version() == 10 and lib.fa2_abi_minor() == 1
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(r"\b%s\(const fa2_paged_kvcache_args\* args" % sym, HEADER), sym
    assert _lib.PAGED_KVCACHE_SYMBOL == "fa2_fwd_kvcache_paged"
    assert lib.fa2_fwd_kvcache_paged.argtypes[0]._type_ is _lib.PagedKvCacheArgs
    assert lib.fa2_paged_kvcache_workspace_bytes.restype is ctypes.c_int64


def test_a_library_without_the_symbol_is_refused_by_name(monkeypatch):
    """load() names the missing entry point and the rebuild command; no AttributeError."""

    class Old:  # a library of ABI 10.1 from before the paged entry points
        def __getattr__(self, name):
            if name.startswith("fa2_") and "paged" not in name:
                fn = lambda *a: {"fa2_version": 10, "fa2_abi_minor": 1}.get(name, 0)
                object.__setattr__(self, name, fn)
                return fn
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(RuntimeError, match=r"fa2_fwd_kvcache_paged.*python -m fa2_triton_amd\.build"):
        _lib.load()
    assert _lib._lib is None


def test_python_signature():
    import fa2_triton_amd
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    assert "flash_attn_with_paged_kvcache" in fa2_triton_amd.__all__
    params = inspect.signature(flash_attn_with_paged_kvcache).parameters
    assert list(params) == ["q", "k_cache", "v_cache", "block_table", "cache_seqlens", "k", "v", "softmax_scale", "causal",
                            "window_size", "num_splits", "return_lse"]
    defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(k=None, v=None, softmax_scale=None, causal=False, window_size=(-1, -1), num_splits=0,
                            return_lse=False)
    doc = flash_attn_with_paged_kvcache.__doc__
    assert "Inference only" in doc and "block_table" in doc and "rotary" in doc
    assert "flash_attn_with_paged_kvcache" in fa2_triton_amd.flash_attn_with_kvcache.__doc__


@pytest.mark.parametrize("kw", [dict(window_size=(1,)), dict(window_size=(1.0, 2)), dict(num_splits=-1),
                                dict(num_splits=129), dict(num_splits=2.0), dict(num_splits=True), dict(k=object()),
                                dict(v=object()), dict(cache_seqlens=1.5), dict(cache_seqlens=True),
                                dict(cache_seqlens=None)])
def test_bad_arguments_raise_before_a_tensor_is_touched(kw):
    from fa2_triton_amd import flash_attn_with_paged_kvcache

    kw = dict(dict(cache_seqlens=1), **kw)
    with pytest.raises((ValueError, TypeError)):
        flash_attn_with_paged_kvcache(None, None, None, None, **kw)


def test_tensor_checks_on_cpu_tensors():
    import torch

    from fa2_triton_amd import flash_attn_with_paged_kvcache as paged

    q, pool = torch.zeros(2, 1, 4, 64, dtype=torch.bfloat16), torch.zeros(6, 16, 2, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="block_table"):
        paged(q, pool, pool, table[0], 5)
    with pytest.raises(ValueError, match="q must be a 4-d"):
        paged(q[0], pool, pool, table, 5)
    with pytest.raises(ValueError, match="k_cache must be a 4-d"):
        paged(q, pool[0], pool, table, 5)
    with pytest.raises(ValueError, match="divisible"):
        paged(q[:, :, :3], pool, pool, table, 5)
    with pytest.raises(ValueError, match="v_cache.shape"):
        paged(q, pool, pool[:4], table, 5)
    with pytest.raises(TypeError, match="v_cache is"):
        paged(q, pool, pool.float(), table, 5)
    with pytest.raises(ValueError, match="q must be on q's GPU device, got cpu"):
        paged(q, pool, pool, table, 5)
    with pytest.raises(ValueError, match="k must be"):
        paged(q, pool, pool, table, 5, k=pool[:2, :1, :1], v=pool[:2, :1, :1])


def _args(**kw):
    """A valid paged call on never-dereferenced pointers: 512 pages of 16 keys per sequence."""
    a = _lib.PagedKvCacheArgs()
    base_kw = {k: kw.pop(k) for k in list(kw) if k not in ("block_table", "block_table_stride", "page_block_size", "num_blocks")}
    a.base = _base_args(**base_kw)
    for name in ("k_cache_stride", "v_cache_stride"):
        getattr(a.base, name)[:] = (16 * 8 * 128, 8 * 128, 128)
    a.block_table, a.block_table_stride, a.page_block_size, a.num_blocks = 4096, 512, 16, 1000
    for key, val in kw.items():
        setattr(a, key, val)
    return a


REJECTED = [
    # everything the contiguous call checks
    (dict(q=None), _lib.FA2_E_INVALID, b"null"),
    (dict(k_cache=None), _lib.FA2_E_INVALID, b"null"),
    (dict(heads_q=30), _lib.FA2_E_INVALID, b"divisible"),
    (dict(dtype=_lib.FA2_F32), _lib.FA2_E_INVALID, b"dtype"),
    (dict(head_dim=264), _lib.FA2_E_UNSUPPORTED, b"> 256"),
    (dict(k_new=4096, seqlen_new=1), _lib.FA2_E_INVALID, b"together"),
    (dict(k_new=4096, v_new=4096, seqlen_new=0), _lib.FA2_E_INVALID, b"seqlen_new"),
    (dict(num_splits=129), _lib.FA2_E_INVALID, b"num_splits"),
    (dict(num_splits=4), _lib.FA2_E_INVALID, b"workspace"),
    (dict(num_splits=4, workspace=4100, workspace_bytes=1 << 30), _lib.FA2_E_INVALID, b"aligned"),
    (dict(head_dim=100), _lib.FA2_E_UNSUPPORTED, b"multiple of 8"),
    (dict(capacity=0), _lib.FA2_E_INVALID, b"sizes"),
    # the paging fields
    (dict(block_table=None), _lib.FA2_E_INVALID, b"null block_table"),
    (dict(page_block_size=48, capacity=48 * 512), _lib.FA2_E_INVALID, b"power of two"),
    (dict(page_block_size=8, capacity=8 * 512), _lib.FA2_E_INVALID, b"power of two"),
    (dict(page_block_size=0), _lib.FA2_E_INVALID, b"power of two"),
    (dict(page_block_size=-16), _lib.FA2_E_INVALID, b"power of two"),
    (dict(num_blocks=0), _lib.FA2_E_INVALID, b"num_blocks"),
    (dict(block_table_stride=511), _lib.FA2_E_INVALID, b"block_table_stride"),
    (dict(capacity=8192 + 8), _lib.FA2_E_INVALID, b"max_blocks * page_block_size"),
    (dict(capacity=(1 << 30) + 16, block_table_stride=1 << 27), _lib.FA2_E_UNSUPPORTED, b"2^30"),
    # 16-byte rows of the pools
    (dict(k_cache=4098), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(v_cache=4104), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
]


@pytest.mark.parametrize("kw,code,text", REJECTED, ids=[",".join(r[0]) + f"-{i}" for i, r in enumerate(REJECTED)])
def test_library_rejects_without_a_gpu(kw, code, text):
    lib = _lib.load()
    assert lib.fa2_fwd_kvcache_paged(ctypes.byref(_args(**kw)), None) == code
    assert text in lib.fa2_last_error(), lib.fa2_last_error()
    assert lib.fa2_fwd_kvcache_paged(None, None) == _lib.FA2_E_INVALID


def test_pool_strides_must_keep_rows_aligned():
    lib = _lib.load()
    for which in ("k_cache_stride", "v_cache_stride"):
        for dim in range(3):
            a = _args()
            getattr(a.base, which)[dim] += 4
            assert lib.fa2_fwd_kvcache_paged(ctypes.byref(a), None) == _lib.FA2_E_UNSUPPORTED
            assert b"16-byte" in lib.fa2_last_error()


def test_status_codes_map_to_the_same_exceptions():
    lib = _lib.load()
    with pytest.raises(ValueError, match="page_block_size"):
        _lib.check(lib.fa2_fwd_kvcache_paged(ctypes.byref(_args(page_block_size=24)), None))
    with pytest.raises(NotImplementedError, match="head_dim"):
        _lib.check(lib.fa2_fwd_kvcache_paged(ctypes.byref(_args(head_dim=100)), None))


def test_splits_and_workspace_equal_the_contiguous_call():
    """The split rule and the workspace size are those of `base`, whatever the page size."""
    lib = _lib.load()
    seen = set()
    for b in (1, 2, 3, 8, 64):
        for hq, hkv in ((32, 8), (8, 8), (16, 1)):
            for sq in (1, 5):
                for cap in (256, 1024, 8192, 1 << 20):
                    for d in (64, 128, 256):
                        for left in (-1, 100, 5000):
                            for forced in (0, 1, 7):
                                for page in (16, 64, 256):
                                    kw = dict(batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, capacity=cap, head_dim=d,
                                              window_left=left, num_splits=forced)
                                    a = _args(page_block_size=page, block_table_stride=cap // page, **kw)
                                    base = _base_args(**kw)
                                    n = lib.fa2_paged_kvcache_num_splits(ctypes.byref(a))
                                    assert n == lib.fa2_kvcache_num_splits(ctypes.byref(base)), (kw, page)
                                    assert (lib.fa2_paged_kvcache_workspace_bytes(ctypes.byref(a))
                                            == lib.fa2_kvcache_workspace_bytes(ctypes.byref(base))), (kw, page)
                                    seen.add(n)
    assert len(seen) > 4 and max(seen) > 7  # the grid reaches the heuristic, not only forced counts
    # arguments the call would reject: 1 split, no workspace (as the contiguous functions)
    bad = _args(page_block_size=24, num_splits=4)
    assert lib.fa2_paged_kvcache_num_splits(ctypes.byref(bad)) == 1
    assert lib.fa2_paged_kvcache_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.fa2_paged_kvcache_num_splits(None) == 1 and lib.fa2_paged_kvcache_workspace_bytes(None) == 0


def test_paged_kernels_exist_and_fit(kernels):  # noqa: F811
    split = {k: v for k, v in kernels.items()
             if re.match(r"_ZN3fa226kvcache_paged_split_kernelILb[01]ELi(32|64|128|256)EEEv22fa2_paged_kvcache_argsi$", k)}
    assert len(split) == 8, sorted(split)  # both dtypes x four head-dim tiles
    for k, (scratch, vgprs, lds) in split.items():
        assert vgprs <= 512 and lds <= 160 * 1024, (k, vgprs, lds)
        # the counted waits assume that no spill traffic sits between the DMA pieces
        assert scratch == 0, (k, scratch)
    assert len([k for k in kernels if "kvcache_paged_append_kernel" in k]) == 1
    # the contiguous kernels are all still there, under their names
    assert len([k for k in kernels if re.match(r"_ZN3fa220kvcache_split_kernelILb[01]ELi\d+EEEv16fa2_kvcache_argsi$", k)]) == 8
    assert len([k for k in kernels if "kvcache_combine_kernel" in k]) == 2
    assert len([k for k in kernels if "kvcache_append_kernel" in k]) == 1
    for k in kernels:
        if "kvcache" in k:  # patterns other tests count kernels by
            assert not any(s in k for s in ("_local_kernel", "dbias_kernel", "fwd_kernel", "dq_kernel", "dkdv_kernel")), k
