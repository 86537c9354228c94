"""bench.py's plain run, `--dump-outputs` and `--full`.

A plain run prints the headline line only (value, ms_per_step, the workload) and, with
`--dump-outputs DIR`, writes what the last timed step returned as DIR/<name>.npy in float32 --
whole arrays up to bench.DUMP_SAMPLE elements, a fixed seeded sample of a larger one.  The inputs
are seeded, so two runs with the same arguments write the same files bit for bit (the kernels are
deterministic, tests/test_repeatability.py).  `--full` adds the per-launch times, the rooflines
and the CPU oracle baseline to the line.  The GPU tests call bench.main() in this process.
"""
import json
import sys

import numpy as np
import pytest
import torch

import bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("kernels", "roofline", "roofline_fwd", "roofline_dq", "cpu_baseline", "fwd_tflops", "bwd_tflops")


def test_dump_outputs_whole_and_sampled(tmp_path):
    small = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).to(torch.bfloat16)
    n = 2 * bench.DUMP_SAMPLE + 3
    large = torch.arange(n, dtype=torch.float32).reshape(1, n)  # value == flat index (exact below 2^24)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"small": small, "large": large, "large2": large + 1.0})
    a = {name: np.load(tmp_path / "a" / f"{name}.npy") for name in ("small", "large", "large2")}
    assert a["small"].dtype == a["large"].dtype == np.float32
    assert a["small"].shape == (2, 3, 4) and np.array_equal(a["small"], small.float().numpy())
    idx = a["large"]
    assert idx.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < n and idx == pytest.approx(np.round(idx))
    assert len(np.unique(idx)) > 0.7 * bench.DUMP_SAMPLE  # a spread sample, not one region
    # the same indices for every array of one size, and from run to run
    assert np.array_equal(a["large2"], idx + 1.0)
    for name, arr in a.items():
        assert np.array_equal(arr, np.load(tmp_path / "b" / f"{name}.npy")), name
    assert sum(arr.nbytes for arr in a.values()) <= 64 << 20


def _run_bench(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(key, raising=False)
    with torch.random.fork_rng(devices=[0]):
        bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(monkeypatch, capsys, tmp_path):
    # B=2 H=4 S=2048 D=128: 2^21 elements per array, so every file is the 2^20-element sample
    shape = ("--batch", "2", "--heads", "4", "--heads-kv", "4", "--seqlen", "2048", "--steps", "3", "--warmup", "1")
    lines = [_run_bench(monkeypatch, capsys, *shape, "--dump-outputs", str(tmp_path / run)) for run in ("a", "b")]
    for line in lines:
        assert all(key in line for key in HEADLINE), line
        assert not any(key in line for key in FULL_ONLY), line
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "TFLOP/s"
        assert line["dtype"] == "bf16" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0 and line["value"] > 0
    total = 0
    for name in ("out", "dq", "dk", "dv"):
        a, b = (np.load(tmp_path / run / f"{name}.npy") for run in ("a", "b"))
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,), (name, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["dk.npy", "dq.npy", "dv.npy", "out.npy"]


@pytest.mark.gpu
def test_dumped_outputs_are_what_the_op_returns(monkeypatch, capsys, tmp_path):
    """Small enough to be written whole: the files equal a direct call of the op on the bench's
    own seeded inputs (same generator calls as bench.main)."""
    from fa2_triton_amd import flash_attn_func

    b, h, s, d = 1, 2, 300, 128
    _run_bench(monkeypatch, capsys, "--batch", str(b), "--heads", str(h), "--heads-kv", str(h), "--seqlen", str(s),
               "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path))
    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(1234)
        q, k, v = (torch.empty(b, s, h, d, device="cuda:0", dtype=torch.bfloat16).normal_(0, 0.5).requires_grad_()
                   for _ in range(3))
        do = torch.randn(b, s, h, d, device="cuda:0", dtype=torch.bfloat16)
    out = flash_attn_func(q, k, v, None, None, 0.0, True, None, None)
    grads = torch.autograd.grad(out, (q, k, v), do)
    for name, t in zip(("out", "dq", "dk", "dv"), (out,) + tuple(grads)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.shape == (b, s, h, d) and np.array_equal(got, t.detach().float().cpu().numpy()), name


@pytest.mark.gpu
def test_full_run_adds_kernels_rooflines_and_cpu_baseline(monkeypatch, capsys):
    line = _run_bench(monkeypatch, capsys, "--batch", "1", "--heads", "2", "--heads-kv", "2", "--seqlen", "256",
                      "--steps", "2", "--warmup", "1", "--full")
    assert all(key in line for key in HEADLINE + FULL_ONLY), sorted(line)
    assert set(line["kernels"]) == {"fwd_kernel", "dq_kernel", "dkdv_kernel"}
    assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["achieved"] > 0
