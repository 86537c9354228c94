"""Where the unit hand-over of the hand-placed dQ and dK/dV goes, from s_memtime stamps (dev tool).

Needs stamp builds (FA2_HIPCC_FLAGS=-DFA2_HP_STAMPS=1 with FA2_BUILD_DIR / FA2_LIB_OUT away from
the shipped library).  Run: python scripts/hp_stamps_bwd.py ab_libs/NAME.so [...]  (each library
in a child process; cfg3 causal and non-causal).  One JSON line per (library, kernel, mask):
cycles of the shader clock per wave and unit between the marks of the kernel's unit loop
(HpStamps, csrc/common.h) -- the statement, the requests for the next unit, the accumulator
read-out, the epilogue blocks (and store_rows_lds's parts summed over the unit's blocks: pack +
LDS write, read back, global stores), dQ's wait for the next unit's Q / dO and its O / delta /
LSE2 pass, and the set-up between the last mark of a unit and the next statement.
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

NAMES = {
    "dq": {0: "statement", 2: "readout", 3: "block0", 4: "block1", 6: "wait_next_q_do", 7: "o_rows_delta_lse",
           8: "setup", 9: "pack_ldswrite", 10: "readback", 11: "stores", 12: "dropout_load_next"},
    "dkdv": {0: "statement", 1: "next_block_issue", 2: "readout_kb0", 3: "stores_kb0", 4: "readout_kb1", 6: "stores_kb1",
             7: "setup", 9: "pack_ldswrite", 10: "readback", 11: "stores"},
}
STAGE = {"dq": 4, "dkdv": 2}


def run_one(lib_path):
    os.environ["FA2_AMD_LIB"] = os.path.abspath(lib_path)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from fa2_triton_amd import _lib
    from fa2_triton_amd.backward import _flash_attn_backward
    from fa2_triton_amd.forward import _flash_attn_forward

    lib = _lib.load()
    rd = lib.fa2_debug_hp_stamps
    rd.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]

    def stamps():
        buf = (ctypes.c_ulonglong * 16)()
        assert rd(buf) == 0
        return list(buf)

    b, h, s, d = 8, 32, 4096, 128
    torch.manual_seed(0)
    q, k, v = (torch.empty(b, s, h, d, device="cuda", dtype=torch.bfloat16).normal_(0, 0.5) for _ in range(3))
    do = torch.randn_like(q)
    for causal in (True, False):
        o, lse, scale, _ = _flash_attn_forward(q, k, v, None, None, 0.0, causal, None, None)
        delta = torch.empty_like(lse)
        _flash_attn_backward(do, q, k, v, None, None, o, lse, 0.0, causal, scale, None, _stages=1, _delta=delta)
        for kern in ("dq", "dkdv"):
            call = lambda: _flash_attn_backward(do, q, k, v, None, None, o, lse, 0.0, causal, scale, None,  # noqa: E731
                                                _stages=STAGE[kern], _delta=delta)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            stamps()
            reps = 5
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            st = stamps()
            waves = st[5]  # units x waves x reps
            rec = {"lib": os.path.basename(os.path.dirname(os.path.abspath(lib_path))) + "/" + os.path.basename(lib_path),
                   "kernel": kern, "causal": causal, "ms": round(e0.elapsed_time(e1) / reps, 4),
                   "units_per_workgroup": round(waves / 4 / reps / 256, 2)}
            for i, name in NAMES[kern].items():
                rec[name] = round(st[i] / waves, 1)
            total = sum(st[i] for i in NAMES[kern] if i < 9 or i == 12)
            rec["handover"] = round((total - st[0]) / waves, 1)  # everything but the statement
            # cycles per SIMD per launch (one wave per SIMD) over the launch time: the in-kernel clock
            rec["clock_ghz"] = round(total / 1024 / reps / (rec["ms"] * 1e6), 3)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 or (len(sys.argv) == 2 and sys.argv[1] != "--child"):
        rc = 0
        for lib in sys.argv[1:]:
            r = subprocess.run([sys.executable, __file__, "--child"], env=dict(os.environ, FA2_STAMP_LIB=lib))
            rc = rc or r.returncode
            if r.returncode:
                break
        sys.exit(rc)
    run_one(os.environ["FA2_STAMP_LIB"])
