"""The two engines of the hand-placed kernel generator (fa2_triton_amd/hp_gen/emitter.py), CPU only.

Every emitted kernel leans on these: the `Emitter` pads the register hazards the hardware does not
interlock and computes the LDS waits, the `GapScheduler` decides which filler goes into which MFMA
gap.  The cases pin their rules on streams of a few instructions; the generated headers themselves
are not pinned (every kernel change rewrites them).
"""
import pytest

from fa2_triton_amd.hp_gen.dq import DqGen
from fa2_triton_amd.hp_gen.emitter import Emitter, GapScheduler

MOP = "v_mfma_f32_32x32x16_bf16"


# -- Emitter ---------------------------------------------------------------------------------------
def test_valu_write_then_mfma_operand_is_padded():
    e = Emitter()
    e.valu("v_mov_b32 v0, 0", "v0")
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    assert e.out == ["v_mov_b32 v0, 0", "s_nop 2", f"{MOP} v[16:31], v[0:3], v[4:7], 0"]


def test_mfma_result_read_by_next_valu_is_padded():
    e = Emitter()
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    e.valu("v_add_f32 v40, v40, v16", "v40", ["v40", "v16"])
    assert e.out[1:] == ["s_nop 12", "v_add_f32 v40, v40, v16"]
    # the wait states already spent count: one instruction in between, one fewer
    e = Emitter()
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    e.valu("v_mov_b32 v50, 0", "v50")
    e.valu("v_add_f32 v40, v40, v16", "v40", ["v40", "v16"])
    assert e.out[1:] == ["v_mov_b32 v50, 0", "s_nop 11", "v_add_f32 v40, v40, v16"]


def test_back_to_back_mfma_chain_needs_no_padding():
    e = Emitter()
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    e.mfma(MOP, "v[16:31]", "v[8:11]", "v[12:15]", "v[16:31]")
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "v[16:31]")
    assert len(e.out) == 3 and all(ln.startswith(MOP) for ln in e.out) and e.n_mfma == 3
    # ... but the result as the A operand of another MFMA is no chain
    e.mfma(MOP, "v[32:47]", "v[16:19]", "v[4:7]", "0")
    assert e.out[3] == "s_nop 12" and len(e.out) == 5


def test_lds_waits_are_counted_from_the_issue_order():
    e = Emitter()
    e.ds_read("ds_read_b128 v[0:3], v100", "v[0:3]")
    e.ds_read("ds_read_b128 v[4:7], v100 offset:16", "v[4:7]")
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[8:11]", "0")      # the older read: one may stay outstanding
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[8:11]", "v[16:31]")  # nothing pending on these registers
    e.mfma(MOP, "v[16:31]", "v[4:7]", "v[8:11]", "v[16:31]")
    assert e.out == ["ds_read_b128 v[0:3], v100", "ds_read_b128 v[4:7], v100 offset:16",
                     "s_waitcnt lgkmcnt(1)", f"{MOP} v[16:31], v[0:3], v[8:11], 0",
                     f"{MOP} v[16:31], v[0:3], v[8:11], v[16:31]",
                     "s_waitcnt lgkmcnt(0)", f"{MOP} v[16:31], v[4:7], v[8:11], v[16:31]"]
    assert e.ds == []


def test_waiting_for_the_newest_read_covers_the_older_ones():
    e = Emitter()
    e.ds_read("ds_read_b128 v[0:3], v100", "v[0:3]")
    e.ds_read("ds_read_b128 v[4:7], v100 offset:16", "v[4:7]")
    e.valu("v_mov_b32 v50, v4", "v50", ["v4"])
    e.valu("v_mov_b32 v51, v0", "v51", ["v0"])
    assert [ln for ln in e.out if ln.startswith("s_waitcnt")] == ["s_waitcnt lgkmcnt(0)"]


def test_snapshot_restore_carries_an_open_mfma_window():
    e = Emitter()
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    snap = e.snapshot()
    nxt = Emitter()
    nxt.valu("v_mov_b32 v60, 0", "v60")  # (the positions are relative: any start)
    nxt.restore([snap])
    nxt.valu("v_add_f32 v40, v40, v16", "v40", ["v40", "v16"])
    assert nxt.out[1:] == ["s_nop 12", "v_add_f32 v40, v40, v16"]
    # of several predecessors the most restrictive one holds
    old = Emitter()
    old.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "0")
    for i in range(5):
        old.valu(f"v_mov_b32 v{50 + i}, 0", f"v{50 + i}")
    for snaps in ([old.snapshot(), snap], [snap, old.snapshot()]):
        nxt = Emitter()
        nxt.restore(snaps)
        nxt.valu("v_add_f32 v40, v40, v16", "v40", ["v40", "v16"])
        assert nxt.out == ["s_nop 12", "v_add_f32 v40, v40, v16"]
    # a reset (a barrier in between) forgets it
    e.reset()
    e.valu("v_add_f32 v40, v40, v16", "v40", ["v40", "v16"])
    assert e.out[1:] == ["v_add_f32 v40, v40, v16"]


def test_close_windows_leaves_nothing_open():
    e = Emitter()
    e.mfma(MOP, "v[16:31]", "v[0:3]", "v[4:7]", "v[16:31]")
    e.close_windows()
    assert e.ws == Emitter.MFMA_C_WAR  # the longest window, counted from the MFMA's own issue
    n = len(e.out)
    e.valu("v_mov_b32 v16, 0", "v16")
    e.valu("v_mov_b32 v0, 0", "v0")
    assert len(e.out) == n + 2


def test_reset_and_snapshot_refuse_a_pending_lds_read():
    e = Emitter()
    e.ds_read("ds_read_b128 v[0:3], v100", "v[0:3]")
    with pytest.raises(AssertionError):
        e.reset()
    with pytest.raises(AssertionError):
        e.snapshot()
    e.drain_lds()
    assert e.out[-1] == "s_waitcnt lgkmcnt(0)"
    e.reset()


def test_drop_pattern_suppresses_matching_instructions_only():
    import re

    e = Emitter()
    e.drop = re.compile(r"^v_exp")
    e.valu("v_exp_f32 v0, v0", "v0", ["v0"], kind="trans")
    e.valu("v_mov_b32 v1, v0", "v1", ["v0"])
    assert e.out == ["v_mov_b32 v1, v0"]


# -- GapScheduler ----------------------------------------------------------------------------------
class _Sched(GapScheduler):
    """Records the emission order in `log`: ("m", i) for MFMA i, else the item's name."""

    def __init__(self, n, **kw):
        super().__init__(n, **kw)
        self.log = []

    def go(self, pre_budget=0):
        self.run(lambda i: self.log.append(("m", i)), pre_budget=pre_budget)
        return self.log


def _add(g, name, stream, cost, rel, dl, **kw):
    g.add(stream, cost, rel, dl, lambda: g.log.append(name), **kw)


def _gap_of(log, name):
    """Index of the MFMA an item follows (-1: before the first)."""
    seen = -1
    for x in log:
        if x == name:
            return seen
        if isinstance(x, tuple):
            seen = x[1]
    raise AssertionError(f"{name} not emitted")


def test_no_item_before_its_release_gap():
    g = _Sched(6)
    _add(g, "a", "a", 4, 3, 5)
    _add(g, "b", "b", 4, -1, 5)
    _add(g, "c", "c", 4, 0, 5)
    log = g.go(pre_budget=100)
    assert _gap_of(log, "a") == 3 and _gap_of(log, "b") == -1 and _gap_of(log, "c") == 0


def test_deadline_beats_the_budget():
    g = _Sched(6)
    _add(g, "big", "x", 100, 0, 2)      # never fits a gap's budget: waits for its deadline
    _add(g, "small", "y", 4, 0, 5)
    log = g.go()
    assert _gap_of(log, "big") == 2 and _gap_of(log, "small") == 0
    # within the budget the earliest deadline goes first, and a gap holds BUDGET issue cycles
    g = _Sched(4)
    for n in range(8):
        _add(g, f"e{n}", f"s{n}", 8, 0, 3)
    log = g.go()
    assert [_gap_of(log, f"e{n}") for n in range(8)] == [0, 0, 0, 1, 1, 1, 2, 2]
    assert GapScheduler.BUDGET == 24


def test_streams_keep_their_order():
    g = _Sched(8)
    _add(g, "a0", "a", 4, 2, 7)   # released late and due late ...
    _add(g, "a1", "a", 4, -1, 0)  # ... holds back its successor, whatever that one's deadline
    _add(g, "b0", "b", 4, -1, 7)
    log = g.go(pre_budget=100)
    assert log.index("a0") < log.index("a1") and _gap_of(log, "a0") == 2 and _gap_of(log, "a1") == 2
    assert _gap_of(log, "b0") == -1


def test_leftovers_follow_the_last_mfma():
    g = _Sched(2)
    _add(g, "late", "a", 4, 10, 12)
    _add(g, "late2", "a", 4, 10, 12)
    _add(g, "other", "b", 4, 5, 5)
    log = g.go()
    assert log == [("m", 0), ("m", 1), "late", "late2", "other"]
    # and with no MFMA at all the items come in the order they were added
    g = _Sched(0)
    _add(g, "x", "a", 50, -1, 3)
    _add(g, "y", "b", 4, -1, 0)
    assert g.go() == ["x", "y"]


def test_lds_cap_defers_a_read_unless_at_its_deadline():
    g = _Sched(4, lds_cap=3)
    _add(g, "r0", "a", 4, 0, 3, lds=2)
    _add(g, "r1", "b", 4, 0, 3, lds=2)
    _add(g, "r2", "c", 4, 0, 3, lds=1)
    log = g.go()
    assert _gap_of(log, "r0") == 0 and _gap_of(log, "r1") == 1 and _gap_of(log, "r2") == 0
    g = _Sched(4, lds_cap=3)
    _add(g, "r0", "a", 4, 0, 0, lds=2)
    _add(g, "r1", "b", 4, 0, 0, lds=2)
    log = g.go()
    assert _gap_of(log, "r0") == 0 and _gap_of(log, "r1") == 0
    g = _Sched(4)  # no cap
    _add(g, "r0", "a", 4, 0, 3, lds=2)
    _add(g, "r1", "b", 4, 0, 3, lds=2)
    log = g.go()
    assert _gap_of(log, "r0") == 0 and _gap_of(log, "r1") == 0


# -- determinism -------------------------------------------------------------------------------------
def test_a_statement_builds_the_same_lines_twice():
    a, b = DqGen(True, True).build(), DqGen(True, True).build()
    assert a == b and len(a) > 1000
    assert DqGen(True, True).e.out == []  # (no state shared between generators)
