"""Which kernels a call launches, pinned on the CPU (no GPU, no HIP call).

csrc/select.h decides it as pure functions (select_fwd, select_bwd, hp_grid); the launchers launch
exactly what the plan names.  tests/select_host_main.cpp, next to this file, includes that header,
fills argument structs and prints one line per case; this test compiles it as host code, runs it
and compares every line with the literal values below.  Those were read from the launchers as they
were before selection became a function (the table of DESIGN.md 1), not from select.h.

Base call: bf16, B = 1, Hq = Hkv = 2, Sq = Sk = 256, D = 128, contiguous BSHD tensors, 16-byte
aligned non-null pointers, no policy.
"""
import os
import subprocess

import pytest

from fa2_triton_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "select_host_main.cpp")

# forward, each case causal and not: (case, path, head-dim tile, bias kind, DROP, aligned, mask kernel first)
FWD = [
    ("base", "hand_placed", 128, 0, 0, 1, 0),
    ("fwd_hp_off", "pipelined", 128, 0, 0, 1, 0),  # FA2_PATH_FWD_HP disabled
    ("d64", "pipelined", 64, 0, 0, 1, 0),
    ("d120", "pipelined", 128, 0, 0, 1, 0),
    ("d32", "general", 32, 0, 0, 1, 0),
    ("d256", "general", 256, 0, 0, 1, 0),
    ("d111", "general", 128, 0, 0, 0, 0),
    ("bias_bf16", "pipelined", 128, 17, 0, 1, 0),
    ("bias_f16", "pipelined", 128, 16, 0, 1, 0),
    ("bias_f32", "general", 128, 1, 0, 1, 0),
    ("bias_rows_unaligned", "general", 128, 1, 0, 1, 0),  # 16-bit bias, bias_stride[2] % 8 != 0
    ("dropout_mask", "hand_placed", 128, 0, 2, 1, 1),
    ("dropout_mask_fwd_hp_off", "general", 128, 0, 2, 1, 1),
    ("dropout_no_mask", "general", 128, 0, 1, 1, 0),
    ("d64_dropout_mask", "general", 64, 0, 2, 1, 1),
    ("kv_row_strides_differ", "general", 128, 0, 0, 1, 0),
    ("stride1024_sk_2p20", "pipelined", 128, 0, 0, 1, 0),  # (Sk + 128) * stride * 2 >= 2^31
    ("stride1024_sk_2p20_m256", "hand_placed", 128, 0, 0, 1, 0),
    ("local_left64", "local", 128, 0, 0, 1, 0),
]

# backward: (case, stage mask, causal, bias kind, dropout, aligned, dQ in fp32, nsplit, reduce, launches in order)
BWD = [
    ("base", 6, 0, 0, 0, 1, 0, 1, 0, "dq:hand_placed dkdv:hand_placed"),
    ("base_causal", 6, 1, 0, 0, 1, 0, 1, 0, "dq:hand_placed dkdv:hand_placed"),
    ("dq_hp_off", 6, 0, 0, 0, 1, 0, 1, 0, "dq:general dkdv:hand_placed"),
    ("dkdv_hp_off", 6, 0, 0, 0, 1, 0, 1, 0, "dq:hand_placed dkdv:general"),
    ("dq_f32", 6, 0, 0, 0, 1, 1, 1, 0, "dq:general dkdv:hand_placed"),
    ("dropout_no_mask", 6, 0, 0, 1, 1, 0, 1, 0, "dq:general dkdv:general"),
    ("dropout_mask_q_do_strides_differ", 6, 0, 0, 1, 1, 0, 1, 0, "dq:hand_placed dkdv:general"),
    ("bias_bf16", 6, 0, 17, 0, 1, 0, 1, 0, "dq:general dkdv:general"),
    ("bias_f16", 6, 0, 16, 0, 1, 0, 1, 0, "dq:general dkdv:general"),
    ("bias_f32", 6, 0, 1, 0, 1, 0, 1, 0, "dq:general dkdv:general"),
    ("bias_bf16_unaligned", 6, 0, 1, 0, 0, 0, 1, 0, "dq:general dkdv:general"),
    ("mqa_workspace", 6, 0, 0, 0, 1, 0, 16, 1, "dq:hand_placed dkdv:hand_placed"),  # B=1 Hq=32 Hkv=1 Sk=4096
    ("mqa_no_workspace", 6, 0, 0, 0, 1, 0, 1, 0, "dq:hand_placed dkdv:hand_placed"),
    ("local_left64", 6, 0, 0, 0, 1, 0, 1, 0, "dq:local dkdv:local"),
    ("local_left64", 7, 0, 0, 0, 1, 0, 1, 0, "delta:general dq:local dkdv:local"),
    # the window holds the causal bound (right = 0): the local kernels have no causal flag
    ("local_left64_causal", 7, 0, 0, 0, 1, 0, 1, 0, "delta:general dq:local dkdv:local"),
    ("base", 1, 0, 0, 0, 1, 0, 1, 0, "delta:general"),
    ("bias_dbias", 14, 0, 17, 0, 1, 0, 1, 0, "dq:general dbias:general dkdv:general"),
    ("bias_dbias_sk0", 8, 0, 17, 0, 1, 0, 1, 0, ""),
]

# hp_grid at 256 compute units: (items, grid_cap, grid)
HP_GRID = [(8, 0, 8), (8, 2, 2), (1000, 0, 256), (1000, 300, 256), (1000, 64, 64)]


def expected_lines():
    out = []
    for name, path, tile, biask, drop, aligned, mask in FWD:
        for causal in (0, 1):
            plan_causal = 0 if path == "local" else causal  # the window holds the causal bound
            out.append(f"fwd {name} causal={causal}: {path} tile={tile} causal={plan_causal} biask={biask} drop={drop} "
                       f"aligned={aligned} mask_first={mask}")
    for name, stages, causal, biask, dropout, aligned, f32, nsplit, reduce, launches in BWD:
        out.append(f"bwd {name} stages={stages}: causal={causal} biask={biask} dropout={dropout} aligned={aligned} "
                   f"dq_f32={f32} nsplit={nsplit} reduce={reduce} [{launches}]")
    out += [f"hp_grid items={items} cap={cap}: {grid}" for items, cap, grid in HP_GRID]
    return out


@pytest.fixture(scope="module")
def compiler():
    try:
        return build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc to compile the host program with")


def run_program(compiler, tmp_path, *flags):
    exe = tmp_path / "select_host_main"
    cmd = [compiler, "-x", "c++", "-std=c++17", "-O1", "-g", *flags, "-I", build.CSRC, "-I", build.INCLUDE, MAIN, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return res.stdout.splitlines()


def check_lines(got):
    want = expected_lines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_selection_matches_the_table(compiler, tmp_path):
    check_lines(run_program(compiler, tmp_path))


def test_selection_is_clean_under_sanitizers(compiler, tmp_path):
    """The same stand-alone host program under AddressSanitizer and UBSan: the same table, and no report."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    res = subprocess.run([compiler, "-x", "c++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if res.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime to link")
    check_lines(run_program(compiler, tmp_path, *flags))


def test_select_header_is_pure_host_code():
    """select.h includes the C ABI header and standard headers only, and names no HIP call."""
    text = open(os.path.join(build.CSRC, "select.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>", '"fa2_amd.h"'], includes
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())  # without the comments
    assert "hip" not in code.lower()
    assert "thread_local" not in code and "static " not in code and "extern " not in code
