"""CPU tests of the KV-cache decode path (ABI 10 minor 1): the header, the ctypes mirror and the
Python signature agree; bad arguments are rejected before any tensor is touched or any kernel is
launched; the workspace size and the split heuristic are the stated host arithmetic; and the new
kernels' gfx950 code objects exist and keep to the resource rules.  No kernel is launched.
"""
import ctypes
import inspect
import os
import re

import pytest

from fa2_triton_amd import _lib, flash_attn_with_kvcache

from tests.test_code_objects import _code_objects, _kernel_descriptors  # the descriptor reader
from tests.test_host import HEADER, _header_struct_fields

MIN_TILES = 4  # FA2_KVCACHE_MIN_SPLIT_TILES


def test_struct_matches_header():
    assert _header_struct_fields("fa2_kvcache_args") == [f[0] for f in _lib.KvCacheArgs._fields_]
    types = dict(_lib.KvCacheArgs._fields_)
    assert types["workspace_bytes"] is ctypes.c_int64 and types["softmax_scale"] is ctypes.c_float
    assert all(types[n] is ctypes.c_int32 for n in ("batch", "capacity", "seqlen_new", "num_splits", "window_left"))


def test_minor_version_and_exports():
    lib = _lib.load()
    assert lib.fa2_version() == 10 and lib.fa2_abi_minor() == 1 == _lib.ABI_MINOR
    assert int(re.search(r"#define FA2_ABI_MINOR (\d+)", HEADER).group(1)) == 1
    assert int(re.search(r"#define FA2_KVCACHE_MIN_SPLIT_TILES (\d+)", HEADER).group(1)) == MIN_TILES
    assert (_lib.KVCACHE_MIN_SPLIT_TILES, _lib.KVCACHE_MAX_SPLITS) == (MIN_TILES, 128)
    for sym in ("fa2_fwd_kvcache", "fa2_kvcache_workspace_bytes", "fa2_kvcache_num_splits", "fa2_abi_minor"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


def test_python_signature():
    import fa2_triton_amd

    assert "flash_attn_with_kvcache" in fa2_triton_amd.__all__
    params = inspect.signature(flash_attn_with_kvcache).parameters
    assert list(params) == ["q", "k_cache", "v_cache", "k", "v", "cache_seqlens", "softmax_scale", "causal",
                            "window_size", "num_splits", "return_lse"]
    defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(k=None, v=None, cache_seqlens=None, softmax_scale=None, causal=False, window_size=(-1, -1),
                            num_splits=0, return_lse=False)
    doc = flash_attn_with_kvcache.__doc__
    assert "Inference only" in doc and "paged" in doc and "rotary" in doc


@pytest.mark.parametrize("kw", [dict(window_size=(1,)), dict(window_size=(1.0, 2)), dict(num_splits=-1),
                                dict(num_splits=129), dict(num_splits=2.0), dict(num_splits=True), dict(k=object()),
                                dict(v=object()), dict(cache_seqlens=1.5), dict(cache_seqlens=True)])
def test_bad_arguments_raise_before_a_tensor_is_touched(kw):
    with pytest.raises((ValueError, TypeError)):
        flash_attn_with_kvcache(None, None, None, **kw)


def test_tensor_checks_on_cpu_tensors():
    import torch

    q, kc = torch.zeros(1, 1, 4, 64, dtype=torch.bfloat16), torch.zeros(1, 16, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="4-d"):
        flash_attn_with_kvcache(q[0], kc, kc)
    with pytest.raises(ValueError, match="divisible"):
        flash_attn_with_kvcache(q[:, :, :3], kc, kc)
    with pytest.raises(ValueError, match="shape"):
        flash_attn_with_kvcache(q, kc, kc[:, :8])
    with pytest.raises(ValueError, match="seqlen_new"):
        flash_attn_with_kvcache(q, kc, kc, k=kc[:, :1, :1], v=kc[:, :1, :1])
    with pytest.raises(TypeError, match="dtype"):
        flash_attn_with_kvcache(q, kc, kc.float())
    with pytest.raises(TypeError, match="fp16 and bf16"):
        flash_attn_with_kvcache(q.float(), kc.float(), kc.float())
    with pytest.raises(ValueError, match="GPU"):
        flash_attn_with_kvcache(q, kc, kc)


def _args(**kw):
    a = _lib.KvCacheArgs()
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.capacity, a.head_dim = 1, 32, 8, 1, 8192, 128
    a.dtype, a.window_left, a.window_right, a.softmax_scale = _lib.FA2_BF16, -1, -1, 0.1
    for name in ("q", "k_cache", "v_cache", "o"):
        setattr(a, name, 4096)  # never dereferenced: validation fails first
    for name in ("q_stride", "k_cache_stride", "v_cache_stride", "o_stride", "k_new_stride", "v_new_stride"):
        getattr(a, name)[:] = (8192 * 8 * 128, 8 * 128, 128)
    for key, val in kw.items():
        setattr(a, key, val)
    return a


REJECTED = [
    (dict(q=None), _lib.FA2_E_INVALID, b"null"),
    (dict(k_cache=None), _lib.FA2_E_INVALID, b"null"),
    (dict(o=None), _lib.FA2_E_INVALID, b"null"),
    (dict(heads_q=30), _lib.FA2_E_INVALID, b"divisible"),
    (dict(dtype=_lib.FA2_F32), _lib.FA2_E_INVALID, b"dtype"),
    (dict(head_dim=264), _lib.FA2_E_UNSUPPORTED, b"> 256"),
    (dict(k_new=4096, seqlen_new=1), _lib.FA2_E_INVALID, b"together"),
    (dict(v_new=4096, seqlen_new=1), _lib.FA2_E_INVALID, b"together"),
    (dict(k_new=4096, v_new=4096, seqlen_new=0), _lib.FA2_E_INVALID, b"seqlen_new"),
    (dict(num_splits=-1), _lib.FA2_E_INVALID, b"num_splits"),
    (dict(num_splits=129), _lib.FA2_E_INVALID, b"num_splits"),
    (dict(num_splits=4), _lib.FA2_E_INVALID, b"workspace"),                                # none given
    (dict(num_splits=4, workspace=4096, workspace_bytes=1000), _lib.FA2_E_INVALID, b"workspace"),  # too small
    (dict(num_splits=4, workspace=4100, workspace_bytes=1 << 30), _lib.FA2_E_INVALID, b"aligned"),
    (dict(head_dim=100), _lib.FA2_E_UNSUPPORTED, b"multiple of 8"),
    (dict(q=4098), _lib.FA2_E_UNSUPPORTED, b"16-byte"),
    (dict(capacity=0), _lib.FA2_E_INVALID, b"sizes"),
]


@pytest.mark.parametrize("kw,code,text", REJECTED, ids=[",".join(r[0]) + f"-{i}" for i, r in enumerate(REJECTED)])
def test_library_rejects_without_a_gpu(kw, code, text):
    lib = _lib.load()
    assert lib.fa2_fwd_kvcache(ctypes.byref(_args(**kw)), None) == code
    assert text in lib.fa2_last_error(), lib.fa2_last_error()
    assert lib.fa2_fwd_kvcache(None, None) == _lib.FA2_E_INVALID


def test_status_codes_map_to_the_same_exceptions():
    lib = _lib.load()
    with pytest.raises(NotImplementedError, match="head_dim"):
        _lib.check(lib.fa2_fwd_kvcache(ctypes.byref(_args(head_dim=100)), None))
    with pytest.raises(ValueError, match="num_splits"):
        _lib.check(lib.fa2_fwd_kvcache(ctypes.byref(_args(num_splits=500)), None))


def test_workspace_bytes():
    lib = _lib.load()
    for b, hq, hkv, sq, d, n in [(1, 32, 8, 1, 128, 4), (3, 16, 2, 5, 96, 7), (2, 8, 8, 2, 256, 128)]:
        a = _args(batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, head_dim=d, num_splits=n)
        assert lib.fa2_kvcache_workspace_bytes(ctypes.byref(a)) == n * b * hq * sq * d * 4 + n * b * hq * sq * 4
        a.num_splits = 1
        assert lib.fa2_kvcache_workspace_bytes(ctypes.byref(a)) == 0
    # unforced: the size for the count the call will use
    a = _args()
    n = lib.fa2_kvcache_num_splits(ctypes.byref(a))
    assert n > 1 and lib.fa2_kvcache_workspace_bytes(ctypes.byref(a)) == n * 32 * 129 * 4


def test_num_splits_heuristic():
    lib = _lib.load()
    splits = lambda **kw: lib.fa2_kvcache_num_splits(ctypes.byref(_args(**kw)))
    assert splits(batch=64) == 1            # 512 units: the grid is already two workgroups per CU
    assert splits(batch=1) > 1
    for forced in (1, 2, 77, 128):
        assert splits(num_splits=forced) == forced
        assert splits(batch=64, num_splits=forced) == forced
    for b in (1, 2, 3, 8, 17):
        for hkv in (1, 2, 8):
            for cap in (1, 64, 255, 256, 300, 1000, 8192, 131072, 1 << 22):
                for left in (-1, 0, 100, 5000):
                    n = splits(batch=b, heads_kv=hkv, capacity=cap, window_left=left)
                    span = cap if left < 0 else min(cap, left + 1 + 63)
                    tiles = -(-span // 64)
                    assert 1 <= n <= 128
                    if n > 1:
                        assert tiles // n >= MIN_TILES, (b, hkv, cap, left, n)
                        units = b * hkv
                        assert (n - 1) * units < 512 or n == 1  # the smallest count that reaches the target
    assert splits(capacity=1 << 22) == 64  # 8 units: 64 splits reach 512 workgroups
    assert splits(heads_kv=1, heads_q=1, capacity=1 << 22) == 128  # capped
    assert splits(window_left=100) == 1    # a 164-key span is 3 tiles: never cut


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    kd = {}
    for co in _code_objects(_lib.LIB_PATH):
        kd.update(_kernel_descriptors(co))
    return kd


def test_kvcache_kernels_exist_and_fit(kernels):
    split = {k: v for k, v in kernels.items()
             if re.match(r"_ZN3fa220kvcache_split_kernelILb[01]ELi(32|64|128|256)EEEv16fa2_kvcache_argsi$", k)}
    assert len(split) == 8, sorted(split)  # both dtypes x four head-dim tiles
    for k, (scratch, vgprs, lds) in split.items():
        assert vgprs <= 512 and lds <= 160 * 1024, (k, vgprs, lds)
        # the counted waits of the kernel assume that no spill traffic sits between its DMA pieces
        assert scratch == 0, (k, scratch)
    assert len([k for k in kernels if "kvcache_combine_kernel" in k]) == 2
    assert len([k for k in kernels if "kvcache_append_kernel" in k]) == 1
    for k in kernels:
        if "kvcache" in k:  # patterns other tests count kernels by
            assert not any(s in k for s in ("_local_kernel", "dbias_kernel", "fwd_kernel", "dq_kernel", "dkdv_kernel")), k
