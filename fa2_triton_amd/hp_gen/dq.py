"""The dQ statements (dq_hp_kernel): register map, `DqGen`, the dropout variant's next-unit loads."""
from . import ABL
from .emitter import Emitter, GapScheduler, _asm_body, _regs, _sgprs_used, rng
# the cursor / descriptor scalar state and the descriptor update are the forward's
from .fwd import SI, SKD, SKP, SKR, SM0, SMASK, SVD, SVP, SVR, descriptors

# ----------------------------------------------------------------------------------------------
# dQ: dq_hp_kernel (csrc/dq_hp_kernel.h)
#
# Register map of the statement:
#   v[0:63]     S^T[rb][h] (scores of key half h; then P), v[64:127] dP^T[rb][h] (then dS, then
#               in place the packed dS^T DSP[rb][kk]: the B operands of dQ^T += K^T dS^T)
#   v[128:143]  K row-fragment ring, v[144:159] V row-fragment ring, v[160:175] K^T ring
#   v[176:177]  mask limits of a masked tile
#   a[0:127]    dQ^T[rb][dt]; a[128:255] the Q and dO fragments ("a" operands)
def QS(rb, h, i=None):
    base = (rb * 2 + h) * 16
    return rng("v", base, 16) if i is None else f"v{base + i}"


def QDP(rb, h, i=None):
    base = 64 + (rb * 2 + h) * 16
    return rng("v", base, 16) if i is None else f"v{base + i}"


def QDSP(rb, kk, j=None):
    """Packed dS^T of 16-key step kk, in place over dP^T[rb][kk >> 1]: pack j of the 8-element
    group 8 (kk & 1) .. + 7 reads elements 2j, 2j + 1 and writes element j (consumed by pack j // 2,
    issued before it in the same stream), so the four packs land in consecutive registers."""
    base = 64 + (rb * 2 + (kk >> 1)) * 16 + 8 * (kk & 1)
    return rng("v", base, 4) if j is None else f"v{base + j}"


def QKR(n):
    return rng("v", 128 + 4 * (n % 4), 4)


def QVR(n):
    return rng("v", 144 + 4 * (n % 4), 4)


def QTR(n, half=None):
    base = 160 + 4 * (n % 4)
    return rng("v", base, 4) if half is None else rng("v", base + 2 * half, 2)


QREL = ["v176", "v177"]
# round 6 (no dropout): -delta of the lane's row in all 16 registers of a block per row block: the
# C operand of the first dP MFMA of both key halves, so the chain yields dP - delta and dS is one
# multiply (as dkdv_hp; dq_kernel seeds its chain the same way, the two stay bitwise equal)


def QNDEL(rb):
    return rng("v", 178 + 16 * rb, 16)


DQ_NVGPR = 178
# dropout (the forward's saved keep words, one 32-key word per row): the words of the current and
# the next tile, per (rb, key half h); per-stream temporaries; the lane's word offsets (cursor)
def QMW(st, rb, h):
    return f"v{DQ_NVGPR + 4 * st + 2 * rb + h}"


def QMT(h, rb):
    """dS temporaries: the K ring's slot 0, free once the S chains are issued (the dS phase
    starts 18 MFMAs later)."""
    return f"v{128 + 2 * h + rb}"


QMO = f"v{DQ_NVGPR + 8}"  # lane byte offset of row block 0's tile-0 words (row block 1: + %[mrs])
DQ_NVGPR_DROP = DQ_NVGPR + 9
Q_MD = "%[mdesc]"  # keep-word descriptor (a 4-SGPR operand)
Q_MOFF = ["s96", "s97"]  # byte offsets of the requested tile's words, row block 0 / 1


def QDQ(rb, dt):
    return rng("a", (rb * 4 + dt) * 16, 16)


# scalar state of the dQ statement (shares the forward's cursor registers)
Q_SN0 = "s66"  # first key of the current tile
Q_PAR = "s67"  # buffer parity of the current tile: (i + boff) & 1
Q_FIN = "s83"  # index of the unit's final tile
Q_NA = "s84"   # class A tiles the A chain runs: min(na, final)


class DqGen:
    """dQ (recompute form, deterministic): 4 waves x 64 query rows (two 32-row blocks rb per
    wave, one wave per SIMD); per 64-key tile 96 MFMAs: S^T = K Q'^T (32), dP^T = V dO^T (32),
    dQ^T += K^T dS^T (32); every K, V and K^T fragment read from LDS feeds both row blocks.
    Same math as the reference's dQ loop (/root/reference/src/backward/compute_dq.py:38-78)
    and dq_kernel: P = exp2(s scale log2 e - LSE2), dS = P (dP - delta), dQ = scale dS K."""

    def __init__(self, bf16, causal, dropout=False):
        self.bf16, self.causal, self.dropout = bf16, causal, dropout
        self.seed = not dropout  # dP chains seeded with -delta (QNDEL)
        self.mop = "v_mfma_f32_32x32x16_bf16" if bf16 else "v_mfma_f32_32x32x16_f16"
        self.cvtop = "v_cvt_pk_bf16_f32" if bf16 else "v_cvt_pk_f16_f32"
        self.e = Emitter()

    def mask_items(self, par):
        """Dropout: the keep words of the next tile (rows of rb, keys 32 h ..) into set 1 - par;
        four dword loads, then the cursor moves one tile (64 keys = 2 words = 256 bytes per row
        block tile of 32 rows)."""
        e = self.e
        out = []
        for rb in range(2):
            for h in range(2):
                def f(rb=rb, h=h):
                    e.raw(f"buffer_load_dword {QMW(1 - par, rb, h)}, {QMO}, {Q_MD}, {Q_MOFF[rb]} offen offset:{128 * h}")
                    if rb == 1 and h == 1:
                        e.salu(f"s_add_u32 {Q_MOFF[0]}, {Q_MOFF[0]}, 256")
                        e.salu(f"s_add_u32 {Q_MOFF[1]}, {Q_MOFF[1]}, 256")
                out.append((16, f))
        return out

    def k_read(self, par, n):
        h, ks = n // 8, n % 8
        imm = par * 16384 + (ks >> 1) * 4096 + 32 * h * 64
        d = QKR(n)
        self.e.ds_read(f"ds_read_b128 {d}, {'%[kb1]' if ks & 1 else '%[kb0]'} offset:{imm}", d)

    def v_read(self, par, n):
        h, ks = n // 8, n % 8
        imm = 32768 + par * 16384 + (ks >> 1) * 4096 + 32 * h * 64
        d = QVR(n)
        self.e.ds_read(f"ds_read_b128 {d}, {'%[kb1]' if ks & 1 else '%[kb0]'} offset:{imm}", d)

    def t_read(self, par, n, half):
        kk, dt = n // 4, n % 4
        imm = par * 16384 + dt * 4096 + 16 * kk * 64
        d = QTR(n, half)
        self.e.ds_read(f"ds_read_b64_tr_b16 {d}, {'%[tb]' if half else '%[ta]'} offset:{imm}", d)

    def dma_items(self, par):
        """K(i+1), V(i+1) into buffer 1 - par (m0 one item ahead)."""
        nb = 1 - par
        pieces = [("k", it) for it in range(4)] + [("v", it) for it in range(4)]

        def m0_of(w_, it):
            return nb * 16384 + it * 4096 + (32768 if w_ == "v" else 0)

        out = []
        for n, (w_, it) in enumerate(pieces):
            def f(n=n, w_=w_, it=it):
                if n == 0:
                    self.e.salu(f"s_add_u32 m0, %[mlds], {m0_of(w_, it)}", m0=True)
                self.e.dma(f"buffer_load_dwordx4 %[off{it}], {SKD if w_ == 'k' else SVD}, 0 offen lds")
                if n + 1 < len(pieces):
                    self.e.salu(f"s_add_u32 m0, %[mlds], {m0_of(*pieces[n + 1])}", m0=True)
            out.append((16, f))
        return out

    def mask_elem(self, rb, h, i):
        """P = key offset o < REL[rb] ? P : 0 (o = 32 h + (i & 3) + 8 (i >> 2))."""
        e = self.e
        o = 32 * h + (i & 3) + 8 * (i >> 2)
        r = QS(rb, h, i)
        sm = SMASK[i & 1]
        e.valu(f"v_cmp_gt_i32_e64 {sm}, {QREL[rb]}, {o}", None, [QREL[rb]])
        e.valu(f"v_cndmask_b32_e64 {r}, 0, {r}, {sm}", r, [r])

    def cvt(self, d, a, b):
        self.e.valu(f"{self.cvtop} {d}, {a}, {b}", d, [a, b])

    def period(self, par, cls):
        e = self.e
        descriptors(e)
        dma = self.dma_items(par) +(self.mask_items(par) if self.dropout else [])
        if cls == "D":
            for _, f in dma:
                f()
        else:
            masked = cls == "B"
            if masked:
                for rb in range(2):
                    e.valu(f"v_subrev_u32 {QREL[rb]}, {Q_SN0}, %[rel{rb}]", QREL[rb], [])
            g = GapScheduler(96)
            for n in range(16):  # K row fragments, then V row fragments: 3 ahead (ring of 4)
                mf = 2 * n
                rel = -1 if n < 3 else mf - 6
                g.add("k", 4, rel, max(rel, mf - 4), lambda n=n: self.k_read(par, n))
            for n in range(16):
                mf = 32 + 2 * n
                rel = max(-1, mf - 6)
                g.add("v", 4, rel, mf - 4, lambda n=n: self.v_read(par, n))
            for n in range(16):  # K^T fragments for dQ: 3 ahead
                mf = 64 + 2 * n
                for hf in range(2):
                    g.add("t", 4, mf - 6, mf - 3, lambda n=n, hf=hf: self.t_read(par, n, hf))
            for h in range(2):
                rel0 = 18 + 16 * h
                for rb in range(2):
                    for i in range(16):
                        r = QS(rb, h, i)
                        st = f"p{h}{rb}"
                        g.add(st, 4, rel0, 38 + 16 * h,
                              lambda r=r, rb=rb: e.valu(f"v_fma_f32 {r}, {r}, %[sc], -%[lse{rb}]", r, [r]))
                        g.add(st, 8, rel0, 40 + 16 * h, lambda r=r: e.valu(f"v_exp_f32 {r}, {r}", r, [r], kind="trans"))
                        if masked:
                            g.add(st, 8, rel0, 41 + 16 * h, lambda rb=rb, h=h, i=i: self.mask_elem(rb, h, i))
                rel1 = 50 + 16 * h
                for rb in range(2):
                    if self.dropout:  # this lane's keys start 4 hh into the word
                        w_ = QMW(par, rb, h)
                        g.add(f"d{h}{rb}", 4, -1, rel1,
                              lambda w_=w_: e.valu(f"v_lshrrev_b32 {w_}, %[msh], {w_}", w_, [w_]))
                    for i in range(16):
                        a_, b_ = QS(rb, h, i), QDP(rb, h, i)
                        st = f"d{h}{rb}"
                        if self.dropout:
                            # dS = P (dP M / (1 - p) - delta), M the forward's keep bit
                            t_, w_, k_ = QMT(h, rb), QMW(par, rb, h), (i & 3) + 8 * (i >> 2)
                            g.add(st, 4, rel1, 56 + 16 * h,
                                  lambda t_=t_, w_=w_, k_=k_: e.valu(f"v_bfe_i32 {t_}, {w_}, {k_}, 1", t_, [w_]))
                            g.add(st, 4, rel1, 57 + 16 * h,
                                  lambda t_=t_, b_=b_: e.valu(f"v_and_b32 {b_}, {t_}, {b_}", b_, [t_, b_]))
                            g.add(st, 4, rel1, 58 + 16 * h,
                                  lambda b_=b_, rb=rb: e.valu(f"v_fma_f32 {b_}, {b_}, %[dsc], -%[del{rb}]", b_, [b_]))
                        g.add(st, 4, rel1, 60 + 16 * h, lambda a_=a_, b_=b_: e.valu(f"v_mul_f32 {b_}, {a_}, {b_}", b_, [a_, b_]))
                        if i & 1:
                            kk, j = 2 * h + (i >> 3), (i & 7) >> 1
                            g.add(st, 4, rel1, 62 + 16 * h,
                                  lambda rb=rb, kk=kk, j=j, h=h, i=i: self.cvt(QDSP(rb, kk, j), QDP(rb, h, i - 1), QDP(rb, h, i)))
            for n, (c, f) in enumerate(dma):
                g.add("dma", c, 0, 40 + 4 * n, f)

            def mfma(gi):
                if gi < 32:
                    h, ks, rb = gi >> 4, (gi >> 1) & 7, gi & 1
                    d = QS(rb, h)
                    e.mfma(self.mop, d, QKR(8 * h + ks), f"%[q{rb * 8 + ks}]", "0" if ks == 0 else d)
                elif gi < 64:
                    x = gi - 32
                    h, ks, rb = x >> 4, (x >> 1) & 7, x & 1
                    d = QDP(rb, h)
                    c0 = QNDEL(rb) if self.seed else "0"
                    e.mfma(self.mop, d, QVR(8 * h + ks), f"%[o{rb * 8 + ks}]", c0 if ks == 0 else d)
                else:
                    f_, rb = (gi - 64) >> 1, gi & 1
                    kk, dt = f_ >> 2, f_ & 3
                    e.mfma(self.mop, QDQ(rb, dt), QTR(f_), QDSP(rb, kk), QDQ(rb, dt))

            g.run(mfma, pre_budget=48)
        e.salu(f"s_add_i32 {SI}, {SI}, 1")
        e.salu(f"s_add_i32 {Q_SN0}, {Q_SN0}, 64")
        e.salu(f"s_xor_b32 {Q_PAR}, {Q_PAR}, 1")
        e.drain_lds()
        if "dq_novm" not in ABL:
            e.raw("s_waitcnt vmcnt(0)")
        if "dq_nobar" not in ABL:
            e.raw("s_barrier")
        e.reset()

    def next_unit_loads(self):
        """The next unit's Q and dO fragments straight into the %[q*] / %[o*] accumulation
        registers (read-write operands; the caller waits before reading them).  Descriptor range
        0 without a next unit."""
        e = self.e
        for what, d in (("q", 68), ("o", 72)):
            e.salu(f"s_mov_b32 s{d}, %[n{what}lo]")
            e.salu(f"s_and_b32 s{d + 1}, %[n{what}hi], 0xffff")
            e.salu(f"s_mov_b32 s{d + 2}, %[n{what}bytes]")
            e.salu(f"s_mov_b32 s{d + 3}, 0x20000")
        for what, d in (("q", 68), ("o", 72)):
            for rb in range(2):
                for ks in range(8):
                    # row block 1: 32 rows further (%[n{what}rs] = 32 row strides, as soffset)
                    so = f"%[n{what}rs]" if rb else "0"
                    e.raw(f"buffer_load_dwordx4 %[{what}{rb * 8 + ks}], %[n{what}o0], s[{d}:{d + 3}], {so} offen offset:{32 * ks}")

    # -- one unit (256 query rows), persistent across units -------------------------------------
    def build(self):
        e = self.e
        e.raw("s_nop 7")
        e.raw("s_nop 7")
        e.salu(f"s_mov_b32 {SM0}, m0")
        for r in range(128):
            e.valu(f"v_accvgpr_write_b32 a{r}, 0", f"a{r}", kind="accw")
        if self.seed:  # -delta blocks (QNDEL): the dP chains' initial accumulators
            for rb in range(2):
                for r in _regs(QNDEL(rb)):
                    e.valu(f"v_sub_f32 {r}, 0, %[del{rb}]", r)
        # DMA cursors: period i requests K(i + 1), V(i + 1); the final period's requests are the
        # next unit's K(0), V(0) (cursors switched to its slices), into the buffer it starts on
        e.salu(f"s_mov_b32 {SKP[0]}, %[klo]")
        e.salu(f"s_mov_b32 {SKP[1]}, %[khi]")
        e.salu(f"s_mov_b32 {SVP[0]}, %[vlo]")
        e.salu(f"s_mov_b32 {SVP[1]}, %[vhi]")
        e.salu(f"s_mov_b32 {SKR}, %[kbytes]")
        e.salu(f"s_mov_b32 {SVR}, %[kbytes]")
        for p0, p1, rem in ((SKP[0], SKP[1], SKR), (SVP[0], SVP[1], SVR)):
            e.salu(f"s_add_u32 {p0}, {p0}, %[tileb]")
            e.salu(f"s_addc_u32 {p1}, {p1}, 0")
            e.salu(f"s_sub_i32 {rem}, {rem}, %[tileb]")
        e.salu(f"s_mov_b32 {SI}, 0")
        e.salu(f"s_mov_b32 {Q_SN0}, 0")
        e.salu(f"s_mov_b32 {Q_PAR}, %[boff]")
        e.salu(f"s_add_i32 {Q_FIN}, %[ntiles], -1")
        e.salu(f"s_min_i32 {Q_NA}, %[na], {Q_FIN}")  # A chain: class A tiles before the final one
        if self.dropout:
            # keep words: tile 0's in %[mw*] (from the previous unit or the caller) -> both sets;
            # period i requests tile i + 1's
            e.salu(f"s_mov_b32 {Q_MOFF[0]}, 256")
            e.salu(f"s_add_u32 {Q_MOFF[1]}, %[mrs], 256")
            e.valu(f"v_mov_b32 {QMO}, %[mo0]", QMO)
            for rb in range(2):
                for h in range(2):
                    for st in range(2):
                        e.valu(f"v_mov_b32 {QMW(st, rb, h)}, %[mw{2 * rb + h}]", QMW(st, rb, h))
        # this unit's K(0), V(0) (requested by the previous unit or before the statement), Q, dO
        e.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e.raw("s_barrier")
        e.reset()
        e.raw(f"s_cmp_lt_i32 {Q_FIN}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_loop")
        # no tile: the next unit's K(0), V(0) into buffer boff as a DMA-only period of parity 1-boff
        self.switch_cursors()
        e.salu(f"s_xor_b32 {Q_PAR}, {Q_PAR}, 1")
        e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_D0")
        e.raw("s_branch .Lhp%=_D1")
        e.raw(".balignl 64, 0xbf800000", 0)
        e.label(".Lhp%=_loop")
        e.raw(f"s_cmp_gt_i32 {SI}, {Q_FIN}")
        e.raw("s_cbranch_scc1 .Lhp%=_end")
        e.raw(f"s_cmp_eq_u32 {SI}, {Q_FIN}")
        e.raw("s_cbranch_scc0 .Lhp%=_cls")
        self.switch_cursors()
        e.label(".Lhp%=_cls")
        e.raw(f"s_cmp_lt_i32 {SI}, %[na]")
        e.raw("s_cbranch_scc1 .Lhp%=_clsA")
        e.raw(f"s_cmp_le_i32 {SI}, %[last]")
        e.raw("s_cbranch_scc1 .Lhp%=_clsB")
        e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_D0")
        e.raw("s_branch .Lhp%=_D1")
        # class A runs as a chain (the final tile excluded: its cursors switch first)
        e.label(".Lhp%=_clsA")
        e.raw(f"s_cmp_eq_u32 {SI}, {Q_FIN}")
        e.raw("s_cbranch_scc1 .Lhp%=_A1f")
        e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_A1")
        e.label(".Lhp%=_A0")
        self.period(0, "A")
        e.raw(f"s_cmp_ge_i32 {SI}, {Q_NA}")
        e.raw("s_cbranch_scc1 .Lhp%=_loop")
        e.label(".Lhp%=_A1")
        self.period(1, "A")
        e.raw(f"s_cmp_lt_i32 {SI}, {Q_NA}")
        e.raw("s_cbranch_scc1 .Lhp%=_A0")
        e.raw("s_branch .Lhp%=_loop")
        e.label(".Lhp%=_A1f")  # the final tile, class A: parity dispatch
        e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_A0")
        e.raw("s_branch .Lhp%=_A1")
        e.label(".Lhp%=_clsB")
        e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_B1")
        for par in (0, 1):
            e.label(f".Lhp%=_B{par}")
            self.period(par, "B")
            e.raw("s_branch .Lhp%=_loop")
        for par in (0, 1):
            e.label(f".Lhp%=_D{par}")
            self.period(par, "D")
            e.raw("s_branch .Lhp%=_loop")
        e.label(".Lhp%=_end")
        if self.dropout:
            # the final period requested the next unit's tile-0 words into set Q_PAR (flipped since)
            e.raw(f"s_cmp_eq_u32 {Q_PAR}, 0")
            e.raw("s_cbranch_scc0 .Lhp%=_mw1")
            for st in range(2):
                if st == 1:
                    e.label(".Lhp%=_mw1")
                for rb in range(2):
                    for h in range(2):
                        e.raw(f"v_mov_b32 %[mw{2 * rb + h}], {QMW(st, rb, h)}")
                if st == 0:
                    e.raw("s_branch .Lhp%=_mwd")
            e.label(".Lhp%=_mwd")
        else:
            # the next unit's Q / dO straight into the operand registers, left in flight across the
            # epilogue (the dropout variant loads them in its own statement after the epilogue:
            # gen_dq_load_next, nothing in flight between statements)
            self.next_unit_loads()
        e.drain_lds()
        e.salu(f"s_mov_b32 m0, {SM0}")
        e.raw("s_nop 15")
        e.raw("s_nop 15")
        return e.out

    def switch_cursors(self):
        e = self.e
        e.salu(f"s_mov_b32 {SKP[0]}, %[nklo]")
        e.salu(f"s_mov_b32 {SKP[1]}, %[nkhi]")
        e.salu(f"s_mov_b32 {SVP[0]}, %[nvlo]")
        e.salu(f"s_mov_b32 {SVP[1]}, %[nvhi]")
        e.salu(f"s_mov_b32 {SKR}, %[nkbytes]")
        e.salu(f"s_mov_b32 {SVR}, %[nkbytes]")
        if self.dropout:  # the final period's keep words: the next unit's tile 0
            e.valu(f"v_mov_b32 {QMO}, %[nmo0]", QMO)
            e.salu(f"s_mov_b32 {Q_MOFF[0]}, 0")
            e.salu(f"s_mov_b32 {Q_MOFF[1]}, %[mrs]")


def gen_dq_function(bf16, causal, dropout=False):
    g = DqGen(bf16, causal, dropout)
    lines = g.build()
    name = f"dq_hp_main_{'bf16' if bf16 else 'f16'}_{'causal' if causal else 'full'}{'_drop' if dropout else ''}"
    nv = DQ_NVGPR_DROP if dropout else DQ_NVGPR + 32
    clob = [f'"v{i}"' for i in range(nv)] + [f'"a{i}"' for i in range(128)] + \
           [f'"s{i}"' for i in _sgprs_used(lines)] + ['"vcc"', '"scc"', '"memory"']
    qops = ", ".join(f'[q{i}] "+a"(q[{i}])' for i in range(16))
    oops = ", ".join(f'[o{i}] "+a"(o[{i}])' for i in range(16))
    mops = (",\n        " + ", ".join(f'[mw{i}] "+v"(mw[{i}])' for i in range(4))) if dropout else ""
    nxt_v = [] if dropout else ["nqo0", "noo0"]
    nxt_s = [] if dropout else ["nqlo", "nqhi", "nqbytes", "nolo", "nohi", "nobytes", "nqrs", "nors"]
    vops = ["kb0", "kb1", "ta", "tb", "off0", "off1", "off2", "off3", "rel0", "rel1", "lse0", "lse1", "del0", "del1"] + \
        nxt_v + (["mo0", "nmo0", "msh"] if dropout else [])
    sops = ["na", "last", "ntiles", "tileb", "kbytes", "mlds", "klo", "khi", "vlo", "vhi", "sc",
            "boff", "nklo", "nkhi", "nvlo", "nvhi", "nkbytes"] + nxt_s + (["mdesc", "mrs", "dsc"] if dropout else [])
    marg = ", uint32_t (&mw)[4]" if dropout else ""
    inout = ("this unit's Q and dO fragments in (the next unit's: gen_dq_load_next)" if dropout else
             "this unit's Q and dO fragments in, the NEXT unit's out -- still in flight (wait before\n// reading them)")
    src = f"""// hand-placed dQ unit ({'bf16' if bf16 else 'fp16'}, {'causal' if causal else 'non-causal'}{', dropout' if dropout else ''}): {len(lines)} lines, {g.e.n_mfma} MFMAs
// q / o: {inout}{'; mw: the keep words of tile 0, in and (next unit) out' if dropout else ''}
FA2_DEV void {name}(u32x4 (&q)[16], u32x4 (&o)[16], const DqHpArgs& a{marg}) {{
  asm volatile(
{_asm_body(lines)}
      : {qops},
        {oops}{mops}
      : {", ".join(f'[{n}] "v"(a.{n})' for n in vops)},
        {", ".join(f'[{n}] "s"(a.{n})' for n in sops)}
      : {", ".join(clob)});
}}
"""
    return src


def gen_dq_load_next():
    """The dropout dQ's next-unit Q / dO fragments: loads and their wait in ONE statement (outputs
    early-clobber), so no load is in flight while compiler code runs (the compiler
    moved in-flight "+a" operands of the spilling dropout variant and read them early)."""
    g = DqGen(True, False, False)
    g.next_unit_loads()
    # s_nop 12: marker of tests/test_code_objects.py (end of the in-flight window: none here)
    lines = ["s_nop 12"] + g.e.out + ["s_waitcnt vmcnt(0)"]
    qops = ", ".join(f'[q{i}] "=&a"(q[{i}])' for i in range(16))
    oops = ", ".join(f'[o{i}] "=&a"(o[{i}])' for i in range(16))
    ins = ", ".join([f'[{n}] "v"(a.{n})' for n in ("nqo0", "noo0")] +
                    [f'[{n}] "s"(a.{n})' for n in ("nqlo", "nqhi", "nqbytes", "nolo", "nohi", "nobytes", "nqrs", "nors")])
    clob = ", ".join([f'"s{i}"' for i in _sgprs_used(lines)] + ['"memory"'])
    return f"""// the next unit's Q / dO fragments (dropout dQ), loaded and waited for in one statement
FA2_DEV void dq_hp_load_next(u32x4 (&q)[16], u32x4 (&o)[16], const DqHpArgs& a) {{
  asm volatile(
{_asm_body(lines)}
      : {qops},
        {oops}
      : {ins}
      : {clob});
}}
"""
