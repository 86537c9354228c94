"""CPU tests of sliding-window attention (ABI 10): the header, the ctypes mirror and the Python
signature carry the window; the library rejects the combinations it does not implement before any
launch; and the windowed kernels' gfx950 code objects keep to the hot kernels' resource rules.
No kernel is launched.
"""
import ctypes
import inspect
import os
import re

import pytest

from fa2_triton_amd import _lib, flash_attn_func
from fa2_triton_amd.utils import check_window_size, set_window

from tests.test_code_objects import _code_objects, _kernel_descriptors  # the descriptor reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fa2_amd.h")).read()


def test_abi_version_is_10():
    assert int(re.search(r"FA2_ABI_VERSION (\d+)", HEADER).group(1)) == 10
    assert _lib.ABI_VERSION == 10
    assert _lib.load().fa2_version() == 10


@pytest.mark.parametrize("cname,pystruct", [("fa2_fwd_args", _lib.FwdArgs), ("fa2_bwd_args", _lib.BwdArgs)])
def test_structs_end_in_the_window(cname, pystruct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    last = [d.strip() for d in body.split(";") if d.strip()][-1]
    assert re.sub(r"\s+", " ", last) == "int32_t local, window_left, window_right"
    fields = pystruct._fields_
    assert [f[0] for f in fields[-3:]] == ["local", "window_left", "window_right"]
    assert all(f[1] is ctypes.c_int32 for f in fields[-3:])
    assert fields[-4][0] == "dropout_mask"
    # a zero-initialised struct has no window
    assert pystruct().local == 0


def test_flash_attn_func_signature_ends_in_window_size():
    params = list(inspect.signature(flash_attn_func).parameters.values())
    assert params[-1].name == "window_size" and params[-1].default == (-1, -1)
    assert params[-2].name == "dropout_seed"  # positional callers are unaffected


@pytest.mark.parametrize("bad", [None, 5, (1,), (1, 2, 3), (1.0, 2), ("1", 2), (True, 1), [1, None]])
def test_window_size_must_be_a_pair_of_ints(bad):
    with pytest.raises(ValueError):
        check_window_size(bad)
    with pytest.raises(ValueError):
        flash_attn_func(None, None, None, window_size=bad)  # rejected before any tensor is touched


def test_set_window_fields():
    a = _lib.FwdArgs()
    set_window(a, (-1, -1))
    assert (a.local, a.window_left, a.window_right) == (0, 0, 0)
    set_window(a, (-7, 3))
    assert (a.local, a.window_left, a.window_right) == (1, -1, 3)
    set_window(a, [0, 0])
    assert (a.local, a.window_left, a.window_right) == (1, 0, 0)


def _fwd_args():
    a = _lib.FwdArgs()
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.seqlen_k, a.head_dim = 1, 2, 2, 64, 64, 128
    a.dtype, a.lse_row_stride = _lib.FA2_BF16, 128
    for name in ("q", "k", "v", "o", "lse"):
        setattr(a, name, 4096)  # never dereferenced: validation fails first
    return a


def _bwd_args():
    a = _lib.BwdArgs()
    a.batch, a.heads_q, a.heads_kv, a.seqlen_q, a.seqlen_k, a.head_dim = 1, 2, 2, 64, 64, 128
    a.dtype, a.dq_dtype, a.lse_row_stride = _lib.FA2_BF16, _lib.FA2_BF16, 128
    for name in ("q", "k", "v", "o", "dout", "lse", "delta", "dq", "dk", "dv"):
        setattr(a, name, 4096)
    return a


def _unsupported(rc, lib):
    return rc == _lib.FA2_E_UNSUPPORTED and b"window" in lib.fa2_last_error()


def test_window_with_bias_or_dropout_is_rejected_without_a_gpu():
    lib = _lib.load()
    a = _fwd_args()
    a.local, a.window_left, a.window_right = 1, 8, 8
    a.bias, a.bias_dtype = 4096, _lib.FA2_BF16
    assert _unsupported(lib.fa2_fwd(ctypes.byref(a), None), lib)
    a.bias, a.bias_dtype, a.dropout_p = None, 0, 0.1
    assert _unsupported(lib.fa2_fwd(ctypes.byref(a), None), lib)
    with pytest.raises(NotImplementedError, match="window"):
        _lib.check(lib.fa2_fwd(ctypes.byref(a), None))

    b = _bwd_args()
    b.local, b.window_left, b.window_right = 1, 8, -1
    b.bias, b.bias_dtype = 4096, _lib.FA2_F16
    assert _unsupported(lib.fa2_bwd(ctypes.byref(b), None), lib)
    b.dbias = 4096
    assert _unsupported(lib.fa2_bwd(ctypes.byref(b), None), lib)
    assert _unsupported(lib.fa2_bwd_stages(ctypes.byref(b), 14, None), lib)
    b.bias, b.bias_dtype, b.dbias, b.dropout_p = None, 0, None, 0.1
    assert _unsupported(lib.fa2_bwd(ctypes.byref(b), None), lib)
    # causal folds into right = 0, the window stays: still rejected
    b.causal = 1
    assert _unsupported(lib.fa2_bwd(ctypes.byref(b), None), lib)


# ---- code objects --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    kd = {}
    for co in _code_objects(_lib.LIB_PATH):
        kd.update(_kernel_descriptors(co))
    return kd


# bf16 / fp16 (Lb1 / Lb0), head-dim tiles 64 and 128, aligned; dQ in the input dtype and in fp32
LOCAL_HOT = {
    "fwd_local": (r"_ZN3fa216fwd_local_kernelILb[01]ELi(64|128)ELb1EEEv12fa2_fwd_args", 4),
    "dq_local": (r"_ZN3fa215dq_local_kernelILb[01]ELi(64|128)ELb1ELb[01]EEEv12fa2_bwd_args", 8),
    "dkdv_local": (r"_ZN3fa217dkdv_local_kernelILb[01]ELi(64|128)ELb1EEEv12fa2_bwd_args", 4),
}


@pytest.mark.parametrize("kind", sorted(LOCAL_HOT))
def test_windowed_kernels_have_no_scratch(kernels, kind):
    pat, count = LOCAL_HOT[kind]
    found = {k: v for k, v in kernels.items() if re.match(pat + "$", k)}
    assert len(found) == count, (kind, sorted(found))
    spilled = {k: v[0] for k, v in found.items() if v[0] != 0}
    assert not spilled, f"scratch bytes per lane: {spilled}"
    for k, (_, vgprs, lds) in found.items():
        assert vgprs <= 256, (k, vgprs)  # two waves per SIMD
        assert lds <= 80 * 1024, (k, lds)  # two workgroups per CU


def test_every_windowed_kernel_exists_and_fits_the_cu(kernels):
    """Both dtypes x four head-dim tiles x aligned / not (x two dQ dtypes), none named like the
    bias-gradient kernels (tests/test_code_objects.py counts those by substring)."""
    found = {k: v for k, v in kernels.items() if "_local_kernel" in k}
    assert len(found) == 16 + 32 + 16, sorted(found)
    for k, (scratch, vgprs, lds) in found.items():
        assert "dbias_kernel" not in k
        assert vgprs <= 512 and lds <= 160 * 1024, (k, vgprs, lds)
