"""The two engines of the generator: `Emitter`, a straight-line instruction emitter that pads
register hazards and computes the LDS waits from a register-state model, and `GapScheduler`,
which places filler items into the gaps between MFMAs; and the helpers that turn the emitted lines
into an inline-asm statement."""
import re


def _regs(spec):
    """'v[3:5]' / 'a7' / 's[64:65]' -> ['v3', 'v4', 'v5'] ..."""
    spec = spec.strip()
    m = re.fullmatch(r"([vas])\[(\d+):(\d+)\]", spec)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    m = re.fullmatch(r"([vas])(\d+)", spec)
    if m:
        return [spec]
    return []  # operands (%[..]), constants, literals: not tracked


def rng(kind, base, n):
    return f"{kind}{base}" if n == 1 else f"{kind}[{base}:{base + n - 1}]"


class Emitter:
    """Straight-line instruction emitter with a hazard / LDS-wait model.

    Wait states are counted per issued instruction (s_nop N = N + 1), the unit of the hazard
    tables; the values below carry margin over the gfx950 minima (8-pass XDL result -> vector
    read 12, vector write -> MFMA operand 2, transcendental -> use 1, VALU -> permlane 2)."""

    MFMA_RESULT = 14   # MFMA writes r  -> any non-chain access of r (8-pass XDL: 12, +2 margin)
    TO_MFMA = 3        # VALU / accvgpr_write writes r -> MFMA reads r
    TRANS_USE = 2      # v_exp writes r -> vector use
    TO_PERM = 3        # VALU writes r -> v_permlane32_swap reads r
    MFMA_READ_WAR = 2  # MFMA reads r (A/B) -> a vector instruction writes r (LDS returns land later)
    MFMA_C_WAR = 18    # MFMA reads r as C -> something writes r
    M0_DMA = 2         # s_* writes m0 -> LDS-DMA

    def __init__(self):
        self.drop = None   # development timing ablations: instructions matching it are not emitted
        self.out = []
        self.ws = 0
        self.wr = {}       # reg -> (ws, kind)
        self.rd_ab = {}    # reg -> ws of the last MFMA A/B read
        self.rd_c = {}     # reg -> ws of the last MFMA C read
        self.ds = []       # pending LDS reads, oldest first: sets of destination regs
        self.n_mfma = 0

    # -- bookkeeping -------------------------------------------------------------------------
    def _line(self, text, ws=1):
        self.out.append(text)
        self.ws += ws

    def reset(self):
        """Block boundary after a barrier / wait: every producer is long done (the barrier waits
        far longer than any hazard window) and no LDS read is pending."""
        assert not self.ds, "LDS reads pending across a block boundary"
        self.wr.clear()
        self.rd_ab.clear()
        self.rd_c.clear()

    def _window(self, kind):
        return {"mfma": self.MFMA_RESULT, "trans": self.TRANS_USE, "m0": self.M0_DMA}.get(
            kind, max(self.TO_MFMA, self.TO_PERM))

    def close_windows(self):
        """Pad until no tracked hazard window is open."""
        need = 0
        for w, k in self.wr.values():
            need = max(need, self._window(k) - (self.ws - w))
        for w in self.rd_ab.values():
            need = max(need, self.MFMA_READ_WAR - (self.ws - w))
        for w in self.rd_c.values():
            need = max(need, self.MFMA_C_WAR - (self.ws - w))
        self._pad(need)

    def snapshot(self):
        """Hazard state relative to the current position (a block boundary without a barrier)."""
        assert not self.ds, "LDS reads pending across a block boundary"
        return ({r: (self.ws - w, k) for r, (w, k) in self.wr.items()},
                {r: self.ws - w for r, w in self.rd_ab.items()},
                {r: self.ws - w for r, w in self.rd_c.items()})

    def restore(self, snaps):
        """Start a block that may follow any of the blocks whose end states are snaps: per
        register the most restrictive of them (no barrier in between)."""
        wr, ab, c = {}, {}, {}
        for swr, sab, sc in snaps:
            for r, (rel, k) in swr.items():
                rem = self._window(k) - rel
                if rem > 0 and (r not in wr or rem > wr[r][2]):
                    wr[r] = (rel, k, rem)
            for src, dst in ((sab, ab), (sc, c)):
                for r, rel in src.items():
                    dst[r] = min(rel, dst.get(r, rel))
        self.ds = []
        self.wr = {r: (self.ws - rel, k) for r, (rel, k, _) in wr.items()}
        self.rd_ab = {r: self.ws - rel for r, rel in ab.items()}
        self.rd_c = {r: self.ws - rel for r, rel in c.items()}

    def _need_lgkm(self, regs):
        hit = -1
        for j, dst in enumerate(self.ds):
            if dst & regs:
                hit = j
        if hit >= 0:
            n = len(self.ds) - 1 - hit
            # the counter holds at most 15: waiting for <= 15 outstanding covers every older read
            # (LDS reads complete in order)
            self._line(f"s_waitcnt lgkmcnt({min(n, 15)})")
            self.ds = self.ds[hit + 1:] if n <= 15 else self.ds[-15:]

    def _pad(self, need):
        need = max(need, 0)
        while need > 0:
            k = min(need, 16)
            self._line(f"s_nop {k - 1}", k)
            need -= k

    def _hazards(self, kind, reads, writes, c_regs=(), chain=False):
        need = 0
        for r in reads | writes:
            w = self.wr.get(r)
            if w is None:
                continue
            dist = self.ws - w[0]
            pk = w[1]
            if pk == "mfma":
                if kind == "mfma" and chain and r in c_regs:
                    continue
                need = max(need, self.MFMA_RESULT - dist)
                continue
            if kind == "mfma" and r in reads:
                need = max(need, self.TO_MFMA - dist)
            if pk == "trans" and r in reads:
                need = max(need, self.TRANS_USE - dist)
            if kind == "perm" and pk in ("valu", "trans", "accr") and r in reads:
                need = max(need, self.TO_PERM - dist)
            if pk == "m0" and kind == "dma":
                need = max(need, self.M0_DMA - dist)
        for r in writes:
            if kind == "mfma" and chain:
                break
            if r in self.rd_ab and kind != "ds":
                need = max(need, self.MFMA_READ_WAR - (self.ws - self.rd_ab[r]))
            # (an MFMA writing a register an earlier MFMA read as C: ordered by the in-order
            # matrix pipe, which reads C before any later MFMA's result lands)
            if r in self.rd_c and kind != "mfma":
                need = max(need, self.MFMA_C_WAR - (self.ws - self.rd_c[r]))
        self._pad(need)

    def _commit(self, kind, writes):
        for r in writes:
            self.wr[r] = (self.ws, kind)

    # -- instructions ------------------------------------------------------------------------
    def mfma(self, op, d, a, b, c):
        rd, ra, rb, rc = map(set, map(_regs, (d, a, b, c)))
        chain = rc == rd
        self._need_lgkm(ra | rb | rc | rd)
        self._hazards("mfma", ra | rb | rc, rd, c_regs=rc, chain=chain)
        for r in ra | rb:
            self.rd_ab[r] = self.ws
        for r in rc:
            self.rd_c[r] = self.ws
        self._commit("mfma", rd)
        self._line(f"{op} {d}, {a}, {b}, {c}")
        self.n_mfma += 1

    def valu(self, text, dst, srcs=(), kind="valu"):
        if self.drop and self.drop.search(text):
            return
        wr = set()
        for d in ([dst] if isinstance(dst, str) else (dst or [])):
            wr |= set(_regs(d))
        rd = set()
        for s in srcs:
            rd |= set(_regs(s))
        self._need_lgkm(rd | wr)
        self._hazards(kind, rd, wr)
        self._line(text)
        self._commit(kind, wr)

    def ds_read(self, text, dst, addr=None):
        if self.drop and self.drop.search(text):
            return
        wr = set(_regs(dst))
        self._need_lgkm(wr)
        self._hazards("ds", set(_regs(addr)) if addr else set(), wr)
        self._line(text)
        self.ds.append(wr)

    def salu(self, text, m0=False):
        if self.drop and self.drop.search(text) and not m0:
            return
        self._line(text)
        if m0:
            self.wr["m0"] = (self.ws, "m0")

    def dma(self, text):
        if self.drop and self.drop.search(text):
            return
        self._hazards("dma", {"m0"}, set())
        self._line(text)

    def raw(self, text, ws=1):
        self._line(text, ws)

    def label(self, name):
        self.out.append(f"{name}:")

    def drain_lds(self):
        if self.ds:
            self._line("s_waitcnt lgkmcnt(0)")
            self.ds = []

    def drain_mfma(self):
        """Pad until every MFMA result may be read by any instruction."""
        need = 0
        for r, (w, k) in self.wr.items():
            if k == "mfma":
                need = max(need, self.MFMA_RESULT - (self.ws - w))
        self._pad(need)


class GapScheduler:
    """Fills the gaps between n MFMAs with filler items.

    An item (stream, cost, release, deadline, emit) may go into gap g (after MFMA g; gap -1 =
    before the first MFMA) once g >= release and its predecessor in the same stream is placed.
    Gap by gap, eligible items are taken earliest-deadline-first while the gap's issue budget
    (32-cycle MFMA gap minus the MFMA's own 8 issue cycles) lasts; an item at its deadline goes in
    regardless.  Costs: v_exp 8, other vector / LDS instructions 4, an LDS-DMA piece 16
    (MI355X_MICROARCH.md, per-instruction issue costs)."""

    BUDGET = 24

    def __init__(self, n, lds_cap=None):
        """lds_cap: at most this much LDS read weight per gap (items added with lds = their weight,
        e.g. 2 per 1 KiB ds_read_b128, 1 per 512 B ds_read_b64_tr_b16), unless at their
        deadline: the four waves of a CU share 256 B/clk of LDS reads, and a burst of reads
        queues behind itself (and a wave stalls at issue with 15 LDS operations outstanding)."""
        self.n = n
        self.items = []
        self.lds_cap = lds_cap

    def add(self, stream, cost, release, deadline, emit, lds=False):
        self.items.append(dict(stream=stream, cost=cost, rel=release, dl=deadline, emit=emit, seq=len(self.items),
                               lds=lds))

    def run(self, mfma, pre_budget=0):
        pending = list(self.items)

        def heads():
            seen, out = set(), []
            for it in pending:
                if it["stream"] not in seen:
                    seen.add(it["stream"])
                    out.append(it)
            return out

        last_use = {}
        tick = [0]

        def fill(g, budget):
            nl = 0
            cap = self.lds_cap
            while True:
                el = [it for it in heads()
                      if it["rel"] <= g and not (cap is not None and it["lds"] and nl + it["lds"] > cap and it["dl"] > g)]
                if not el:
                    return
                # earliest deadline first; among equals the stream served longest ago (two
                # dependent chains alternate instead of running back to back)
                el.sort(key=lambda it: (it["dl"], last_use.get(it["stream"], -1), it["seq"]))
                it = el[0]
                if it["cost"] > budget and it["dl"] > g:
                    # something cheaper that fits?
                    fit = [x for x in el if x["cost"] <= budget]
                    if not fit:
                        return
                    it = fit[0]
                pending.remove(it)
                it["emit"]()
                last_use[it["stream"]] = tick[0]
                tick[0] += 1
                budget -= it["cost"]
                nl += it["lds"] or 0

        fill(-1, pre_budget)
        for g in range(self.n):
            mfma(g)
            fill(g, self.BUDGET)
        while pending:  # no MFMA left to cover them
            it = heads()[0]
            pending.remove(it)
            it["emit"]()


def _asm_body(lines):
    return "\n".join(f'      "{l}\\n"' for l in lines)


def _sgprs_used(lines):
    """The fixed SGPRs a statement names (its clobbers: no more than it uses, so the compiler
    keeps the rest for the values live across it)."""
    used = set()
    for l in lines:
        for m in re.finditer(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b", l):
            if m.group(3):
                used.add(int(m.group(3)))
            else:
                used.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return sorted(used)
