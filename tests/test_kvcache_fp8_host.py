"""CPU tests of the fp8 KV-cache decode path (fa2_fwd_kvcache_fp8, added within ABI 10 minor 1 and
detected by the symbol): the header, the ctypes mirror and the Python signature agree; bad arguments
are rejected before any tensor is touched or any kernel is launched; the split count and the
workspace are those of the contiguous call on the same shapes; every finite e4m3 value is a bf16 and
an fp16 value; and the new kernels' gfx950 code objects exist beside the unchanged old ones and keep
to the resource rules.  No kernel is launched.
"""
import ctypes
import inspect
import re

import pytest
import torch

from fa2_triton_amd import _lib

from tests.test_host import HEADER, _header_struct_fields
from tests.test_kvcache_host import REJECTED as BASE_REJECTED
from tests.test_kvcache_host import _args as _base_args
from tests.test_kvcache_host import kernels  # noqa: F401  (the descriptor fixture)
from tests.test_kvcache_paged_host import _args as _paged_args

SYMBOLS = ("fa2_fwd_kvcache_fp8", "fa2_fp8_kvcache_num_splits", "fa2_fp8_kvcache_workspace_bytes")


def test_struct_matches_header():
    assert _header_struct_fields("fa2_fp8_kvcache_args") == [f[0] for f in _lib.Fp8KvCacheArgs._fields_]
    types = dict(_lib.Fp8KvCacheArgs._fields_)
    assert types["paged"] is _lib.PagedKvCacheArgs
    assert types["k_descale"] is ctypes.c_void_p and types["v_descale"] is ctypes.c_void_p
    assert types["k_descale_stride"] is types["v_descale_stride"] and ctypes.sizeof(types["k_descale_stride"]) == 16
    # the paged struct is the first member, unchanged, and its base a contiguous call's args
    assert _lib.Fp8KvCacheArgs.paged.offset == 0
    assert ctypes.sizeof(_lib.Fp8KvCacheArgs) == ctypes.sizeof(_lib.PagedKvCacheArgs) + 48


def test_symbols_are_exported_and_bound_and_the_version_stays():
    lib = _lib.load()
    assert lib.fa2_version() == 10 and lib.fa2_abi_minor() == 1
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(r"\b%s\(const fa2_fp8_kvcache_args\* args" % sym, HEADER), sym
    assert _lib.FP8_KVCACHE_SYMBOL == "fa2_fwd_kvcache_fp8"
    assert lib.fa2_fwd_kvcache_fp8.argtypes[0]._type_ is _lib.Fp8KvCacheArgs
    assert lib.fa2_fp8_kvcache_workspace_bytes.restype is ctypes.c_int64


def test_a_library_without_the_symbol_is_refused_by_name(monkeypatch):
    """load() names the missing entry point and the rebuild command; no AttributeError."""

    class Old:  # a library of ABI 10.1 with the paged entry points, from before the fp8 ones
        def __getattr__(self, name):
            if name.startswith("fa2_") and "fp8" not in name:
                fn = lambda *a: {"fa2_version": 10, "fa2_abi_minor": 1}.get(name, 0)
                object.__setattr__(self, name, fn)
                return fn
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(RuntimeError, match=r"fa2_fwd_kvcache_fp8.*python -m fa2_triton_amd\.build"):
        _lib.load()
    assert _lib._lib is None


def test_python_signature():
    import fa2_triton_amd
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    assert "flash_attn_with_fp8_kvcache" in fa2_triton_amd.__all__
    params = inspect.signature(flash_attn_with_fp8_kvcache).parameters
    assert list(params) == ["q", "k_cache", "v_cache", "k_descale", "v_descale", "block_table", "cache_seqlens", "k", "v",
                            "softmax_scale", "causal", "window_size", "num_splits", "return_lse"]
    defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(k_descale=None, v_descale=None, block_table=None, cache_seqlens=None, k=None, v=None,
                            softmax_scale=None, causal=False, window_size=(-1, -1), num_splits=0, return_lse=False)
    doc = flash_attn_with_fp8_kvcache.__doc__
    assert "Inference only" in doc and "block_table" in doc and "rotary" in doc and "e4m3" in doc
    for other in (fa2_triton_amd.flash_attn_with_kvcache, fa2_triton_amd.flash_attn_with_paged_kvcache):
        assert "flash_attn_with_fp8_kvcache" in other.__doc__


@pytest.mark.parametrize("kw", [dict(k_descale=0.0), dict(v_descale=0.0), dict(k_descale=-1.0), dict(v_descale=-0.5),
                                dict(k_descale=True), dict(v_descale=False), dict(k_descale="1"), dict(v_descale=(1.0,)),
                                dict(k_descale=float("nan")), dict(v_descale=float("inf")),
                                dict(block_table=object()), dict(block_table=object(), cache_seqlens=None),
                                # the list of the 16-bit functions
                                dict(window_size=(1,)), dict(window_size=(1.0, 2)), dict(num_splits=-1), dict(num_splits=129),
                                dict(num_splits=2.0), dict(num_splits=True), dict(k=object()), dict(v=object()),
                                dict(cache_seqlens=1.5), dict(cache_seqlens=True)])
def test_bad_arguments_raise_before_a_tensor_is_touched(kw):
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    if "block_table" in kw and "cache_seqlens" not in kw:
        kw = dict(kw, cache_seqlens=1)  # reaches the table check itself
    with pytest.raises((ValueError, TypeError)):
        flash_attn_with_fp8_kvcache(None, None, None, **kw)


def test_block_table_needs_the_lengths():
    from fa2_triton_amd import flash_attn_with_fp8_kvcache

    with pytest.raises(TypeError, match="cache_seqlens is required"):
        flash_attn_with_fp8_kvcache(None, None, None, block_table=torch.zeros(1, 1, dtype=torch.int32))


def test_tensor_checks_on_cpu_tensors():
    from fa2_triton_amd import flash_attn_with_fp8_kvcache as fp8, flash_attn_with_kvcache

    q = torch.zeros(2, 1, 4, 64, dtype=torch.bfloat16)
    kc = torch.zeros(2, 16, 2, 64, dtype=torch.uint8).view(torch.float8_e4m3fn)
    table = torch.zeros(2, 3, dtype=torch.int32)
    for bad in (kc.view(torch.float8_e5m2), kc.view(torch.uint8), kc.to(torch.bfloat16), kc.float()):
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            fp8(q, bad, kc)
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            fp8(q, kc, bad)
    with pytest.raises(TypeError, match="fp16 and bf16"):
        fp8(q.float(), kc, kc)
    with pytest.raises(TypeError, match="k is"):
        fp8(q, kc, kc, k=kc[:, :1], v=kc[:, :1])  # the new rows come in q's dtype
    with pytest.raises(ValueError, match="4-d"):
        fp8(q[0], kc, kc)
    with pytest.raises(ValueError, match="divisible"):
        fp8(q[:, :, :3], kc, kc)
    with pytest.raises(ValueError, match="shape"):
        fp8(q, kc, kc[:, :8])
    with pytest.raises(ValueError, match="block_table"):
        fp8(q, kc, kc, block_table=table[0], cache_seqlens=5)
    with pytest.raises(ValueError, match="GPU"):
        fp8(q, kc, kc)
    with pytest.raises(TypeError, match="dtype"):  # the 16-bit function keeps refusing fp8 caches
        flash_attn_with_kvcache(q, kc, kc)


def test_descale_tensor_checks():
    """The descale checks come after the tensor checks, which CPU tensors fail on the device test;
    they are exercised on their own."""
    from fa2_triton_amd.kvcache import _check_descale, _descale_on_device

    dev = torch.device("cpu")
    assert _descale_on_device("k_descale", None, 2, 4, dev) is None
    full = _descale_on_device("k_descale", 0.5, 2, 4, dev)
    assert full.shape == (2, 4) and full.stride() == (0, 0) and full.dtype == torch.float32 and float(full[1, 3]) == 0.5
    for good in (torch.ones(2, 4), torch.ones(1, 4), torch.ones(2, 1), torch.ones(4), torch.ones(()), torch.ones(1, 1).expand(2, 4)):
        assert _descale_on_device("k_descale", good, 2, 4, dev).shape == (2, 4)
    for bad in (torch.ones(3, 4), torch.ones(2, 3), torch.ones(2), torch.ones(1, 2, 4)):
        with pytest.raises(ValueError, match=r"v_descale must be broadcastable to \[batch=2, heads_kv=4\]"):
            _descale_on_device("v_descale", bad, 2, 4, dev)
    for bad in (torch.ones(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.bfloat16), torch.ones(2, 4, dtype=torch.int32)):
        with pytest.raises(TypeError, match="k_descale must be an fp32 tensor"):
            _descale_on_device("k_descale", bad, 2, 4, dev)
    with pytest.raises(ValueError, match="must be on q's GPU device"):
        _descale_on_device("k_descale", torch.ones(2, 4), 2, 4, torch.device("cuda", 0))
    _check_descale("k_descale", torch.zeros(3))  # a tensor's contents are never read on the host
    _check_descale("k_descale", 2)


def test_every_e4m3_value_is_a_bf16_and_an_fp16_value():
    """What makes the in-register conversion lossless: all 256 codes survive both round trips."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn)
    exact = codes.float()
    finite = torch.isfinite(exact)
    assert int((~finite).sum()) == 2 and torch.isnan(exact[~finite]).all()  # 0x7f, 0xff: no infinities in e4m3fn
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(codes.to(dtype).float()[finite], exact[finite]), dtype
        assert torch.equal(exact.to(dtype).float()[finite], exact[finite]), dtype
    assert float(exact[finite].abs().max()) == 448.0 and float(exact[1]) == 2.0 ** -9


def _args(paged=False, **kw):
    """A valid fp8 call on never-dereferenced pointers: the 16-bit tests' shapes with byte caches."""
    a = _lib.Fp8KvCacheArgs()
    own = {k: kw.pop(k) for k in list(kw) if k in ("k_descale", "v_descale")}
    strides = {k: kw.pop(k) for k in list(kw) if k in ("k_descale_stride", "v_descale_stride")}
    if paged:
        a.paged = _paged_args(**kw)
    else:
        a.paged.base = _base_args(**kw)
    for key, val in own.items():
        setattr(a, key, val)
    for key, val in strides.items():
        getattr(a, key)[:] = val
    return a


REJECTED = [
    (dict(head_dim=144), _lib.FA2_E_UNSUPPORTED, b"> 128"),
    (dict(head_dim=256), _lib.FA2_E_UNSUPPORTED, b"> 128"),
    (dict(head_dim=72), _lib.FA2_E_UNSUPPORTED, b"multiple of 16"),
    (dict(head_dim=8), _lib.FA2_E_UNSUPPORTED, b"multiple of 16"),
    (dict(k_cache=4096 + 8), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(v_cache=4096 + 8), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(k_descale=4098), _lib.FA2_E_INVALID, b"4-byte"),
    (dict(k_descale=4096, k_descale_stride=(-1, 0)), _lib.FA2_E_INVALID, b"descale stride"),
]
# everything fa2_fwd_kvcache rejects (head_dim = 100 is caught by the fp8 path's own multiple)
BASE = [(kw, code, b"multiple of 16" if kw == dict(head_dim=100) else text) for kw, code, text in BASE_REJECTED]
# the paging rejections when block_table is set
PAGED = [
    (dict(page_block_size=48, capacity=48 * 512), _lib.FA2_E_INVALID, b"power of two"),
    (dict(page_block_size=8, capacity=8 * 512), _lib.FA2_E_INVALID, b"power of two"),
    (dict(page_block_size=0), _lib.FA2_E_INVALID, b"power of two"),
    (dict(num_blocks=0), _lib.FA2_E_INVALID, b"num_blocks"),
    (dict(block_table_stride=511), _lib.FA2_E_INVALID, b"block_table_stride"),
    (dict(capacity=8192 + 8), _lib.FA2_E_INVALID, b"max_blocks * page_block_size"),
    (dict(capacity=(1 << 30) + 16, block_table_stride=1 << 27), _lib.FA2_E_UNSUPPORTED, b"2^30"),
    (dict(k_cache=4096 + 8), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(head_dim=144), _lib.FA2_E_UNSUPPORTED, b"> 128"),
    (dict(head_dim=72), _lib.FA2_E_UNSUPPORTED, b"multiple of 16"),
    (dict(q=None), _lib.FA2_E_INVALID, b"null"),
    (dict(num_splits=4), _lib.FA2_E_INVALID, b"workspace"),
]
ALL = [(False,) + r for r in REJECTED + BASE] + [(True,) + r for r in PAGED]


@pytest.mark.parametrize("paged,kw,code,text", ALL,
                         ids=[("paged-" if r[0] else "") + ",".join(r[1]) + f"-{i}" for i, r in enumerate(ALL)])
def test_library_rejects_without_a_gpu(paged, kw, code, text):
    lib = _lib.load()
    assert lib.fa2_fwd_kvcache_fp8(ctypes.byref(_args(paged, **kw)), None) == code
    assert text in lib.fa2_last_error(), lib.fa2_last_error()
    assert lib.fa2_fwd_kvcache_fp8(None, None) == _lib.FA2_E_INVALID


def test_paging_fields_are_ignored_without_a_block_table():
    """A NULL block_table is the contiguous layout: a page size that the paged call rejects is not
    looked at, and the rejection that follows is the contiguous call's."""
    lib = _lib.load()
    a = _args(num_splits=4)  # passes every check up to the missing workspace
    a.paged.page_block_size, a.paged.num_blocks, a.paged.block_table_stride = 24, -3, -1
    assert lib.fa2_fwd_kvcache_fp8(ctypes.byref(a), None) == _lib.FA2_E_INVALID
    assert b"workspace" in lib.fa2_last_error()
    assert lib.fa2_fp8_kvcache_num_splits(ctypes.byref(a)) == 4


def test_cache_strides_must_keep_rows_aligned():
    """Cache strides are in bytes: off by 8 is a misaligned row (it would be fine for 16-bit rows)."""
    lib = _lib.load()
    for paged in (False, True):
        for which in ("k_cache_stride", "v_cache_stride"):
            for dim in range(3):
                a = _args(paged)
                getattr(a.paged.base, which)[dim] += 8
                assert lib.fa2_fwd_kvcache_fp8(ctypes.byref(a), None) == _lib.FA2_E_UNSUPPORTED
                assert b"16-byte" in lib.fa2_last_error()


def test_status_codes_map_to_the_same_exceptions():
    lib = _lib.load()
    with pytest.raises(NotImplementedError, match="head_dim 144 > 128"):
        _lib.check(lib.fa2_fwd_kvcache_fp8(ctypes.byref(_args(head_dim=144)), None))
    with pytest.raises(ValueError, match="page_block_size"):
        _lib.check(lib.fa2_fwd_kvcache_fp8(ctypes.byref(_args(True, page_block_size=24)), None))


def test_splits_and_workspace_equal_the_contiguous_call():
    lib = _lib.load()
    seen = set()
    for b in (1, 2, 3, 8, 64):
        for hq, hkv in ((32, 8), (8, 8), (16, 1)):
            for sq in (1, 5):
                for cap in (256, 1024, 8192, 1 << 20):
                    for d in (16, 48, 64, 128):
                        for left in (-1, 100, 5000):
                            for forced in (0, 1, 7):
                                kw = dict(batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, capacity=cap, head_dim=d,
                                          window_left=left, num_splits=forced)
                                base = _base_args(**kw)
                                want = (lib.fa2_kvcache_num_splits(ctypes.byref(base)),
                                        lib.fa2_kvcache_workspace_bytes(ctypes.byref(base)))
                                for a in (_args(**kw), _args(True, page_block_size=64, block_table_stride=cap // 64, **kw)):
                                    got = (lib.fa2_fp8_kvcache_num_splits(ctypes.byref(a)),
                                           lib.fa2_fp8_kvcache_workspace_bytes(ctypes.byref(a)))
                                    assert got == want, kw
                                seen.add(want[0])
    assert len(seen) > 4 and max(seen) > 7  # the grid reaches the heuristic, not only forced counts
    # arguments the call would reject: 1 split, no workspace (as the contiguous functions)
    for bad in (_args(head_dim=144, num_splits=4), _args(True, page_block_size=24, num_splits=4)):
        assert lib.fa2_fp8_kvcache_num_splits(ctypes.byref(bad)) == 1
        assert lib.fa2_fp8_kvcache_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.fa2_fp8_kvcache_num_splits(None) == 1 and lib.fa2_fp8_kvcache_workspace_bytes(None) == 0


COUNTED = ("kvcache_combine_kernel", "kvcache_append_kernel", "_local_kernel", "dbias_kernel", "fwd_kernel", "dq_kernel",
           "dkdv_kernel")


def test_fp8_kernels_exist_and_fit(kernels):  # noqa: F811
    split = {k: v for k, v in kernels.items() if "kvcache_fp8_split_kernel" in k or "kvcache_fp8_paged_split_kernel" in k}
    assert len(split) == 8, sorted(split)  # both dtypes x head-dim tiles 64, 128 x both layouts
    wide = {(m.group(1), int(m.group(2))): v for k, v in kernels.items()
            for m in [re.match(r"_ZN3fa220kvcache_split_kernelILb([01])ELi(\d+)EEEv16fa2_kvcache_argsi$", k)] if m}
    tiles = set()
    for k, (scratch, vgprs, lds) in split.items():
        m = re.search(r"kernelILb([01])ELi(64|128)ELb[01]EEE", k)
        assert m, k
        tiles.add((m.group(1), int(m.group(2))))
        assert vgprs <= 512 and lds <= 160 * 1024, (k, vgprs, lds)
        # the counted waits assume that no spill traffic sits between the DMA pieces
        assert scratch == 0, (k, scratch)
        # no more LDS than the 16-bit kernel of the same tile
        assert lds <= wide[(m.group(1), int(m.group(2)))][2], (k, lds)
        # two workgroups share a CU (bytes in flight): LDS and the 256-VGPR bound
        assert 2 * lds <= 160 * 1024 and vgprs <= 256, (k, vgprs, lds)
    assert len(tiles) == 4
    assert len([k for k in kernels if "kvcache_fp8_append_kernel" in k]) == 4  # dtypes x layouts
    for k in kernels:
        if "fp8" in k:
            assert not any(s in k for s in COUNTED), k
            assert not re.match(r"_ZN3fa22\dkvcache_(paged_)?split_kernelILb", k), k
    # the existing counts are unchanged
    assert len(wide) == 8
    assert len([k for k in kernels
                if re.match(r"_ZN3fa226kvcache_paged_split_kernelILb[01]ELi\d+EEEv22fa2_paged_kvcache_argsi$", k)]) == 8
    assert len([k for k in kernels if "kvcache_combine_kernel" in k]) == 2
    assert len([k for k in kernels if "kvcache_append_kernel" in k]) == 1
    assert len([k for k in kernels if "kvcache_paged_append_kernel" in k]) == 1
