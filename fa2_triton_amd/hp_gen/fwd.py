"""The forward statements (fwd_hp_kernel): register map, `FwdGen`.

Same algorithm as the reference's compute_row_block (/root/reference/src/forward/
compute_row_blocks.py:38-103) and fwd_pipe_kernel: per 64-key tile, S^T = K Q^T (swapped so the
softmax row is one lane pair), online softmax in base 2 with defer-max (running max moved only
when a row grows by more than 8), O^T += V^T P^T.  Differences of arrangement only:
  * the scale is applied in fp32, one fma per score: z = s (scale log2 e) - m_ref, as the
    reference scales qk in fp32;
  * the row sums of P are added in the PV phase (where the VALU has room), the exponentials of a
    tile ride on the next tile's QK^T MFMAs.
"""
import re

from . import ABL
from .emitter import Emitter, GapScheduler, _asm_body, _sgprs_used, rng

NINF = "0xff800000"
# head dim 128 only (a D = 64 unit of this generator was measured no faster than fwd_pipe_kernel
# at D = 64, where the softmax VALU bounds both -- DESIGN.md section 6 -- so none is generated)
KS = 8        # 16-wide k-steps of QK^T
NDT = 4       # 32-wide d-tiles of O; also the 4 KiB LDS-DMA pieces of a tile
TILE = 16384  # bytes of a 64-row K / V tile


# ----------------------------------------------------------------------------------------------
# Register map of the forward (fixed registers owned by the asm statement)
#   v[0:127]    S[set][rb][t] scores / exponent arguments / probabilities (16 per key half)
#   v[128:159]  PF[rb][kk] packed P (B operand of O^T += V^T P^T), 4 dwords per 16-key step
#   v[160:191]  INIT[rb]: -m_ref in register 0 of each block; the rest hold the dropout masks
#   v[192:215]  row statistics and temporaries
#   a[0:127]    O^T[rb][dt] accumulators
#   a[128:191]  Q fragments (compiler-placed "a" operands %[q0]..%[q15])
#   a[192:207]  K fragment ring (4 slots), a[208:223] V^T fragment ring (4 slots)
#   s[64:91]    scalar state
def S(st, rb, t, i=None):
    base = ((st * 2 + rb) * 2 + t) * 16
    return rng("v", base, 16) if i is None else f"v{base + i}"


def PF(rb, kk, j=None):
    base = 128 + (rb * 4 + kk) * 4
    return rng("v", base, 4) if j is None else f"v{base + j}"


def INIT(rb, j=None):
    return rng("v", 160 + 16 * rb, 16) if j is None else f"v{160 + 16 * rb + j}"


MRUN = ["v192", "v193"]
LSUM = [["v194", "v195"], ["v196", "v197"]]
MREF = ["v198", "v199"]
THR = ["v200", "v201"]
MAH = [["v202", "v203"], ["v204", "v205"]]
MX = ["v206", "v207"]
REL = ["v208", "v209"]
VNINF = "v210"
TMP = ["v211", "v212", "v213", "v214", "v215"]
N_VGPR = 216
# dropout statement (INIT(rb, 1..15) are otherwise unused): keep words W[set][rb][t]
# of the lane's row (set = tile parity; t = 32-key half) in v[177:184], and per row block the byte
# masks MC[rb][c] (byte n = 0xFF iff element (i & 3 = c, i >> 2 = n) is kept) in v[161:168];
# s[92:95] the keep-mask descriptor, s96 the byte offset of the next tile's words
FW_MD = "s[92:95]"
FW_MT = "s96"
FW_SEL = "s97"              # v_perm_b32 selector of the byte masks (mask_prep_items)
FW_TMP = ["v169", "v170"]   # per row block: the S0 source of that v_perm_b32


def FW_W(s, rb, t):
    return f"v{177 + 4 * s + 2 * rb + t}"


def FW_MC(rb, c):
    return f"v{161 + 4 * rb + c}"


def O(rb, dt, i=None):
    base = (rb * 4 + dt) * 16
    return rng("a", base, 16) if i is None else f"a{base + i}"


def KR(slot):
    return rng("a", 192 + 4 * slot, 4)


def VR(slot, half=None):
    base = 208 + 4 * slot
    return rng("a", base, 4) if half is None else rng("a", base + 2 * half, 2)


AGPR_CLOBBER = list(range(0, 128)) + list(range(192, 256))

# scalar state
SI = "s64"        # period index i
SN1 = "s65"       # 64 (i + 1): first key of tile i + 1
SKD = "s[68:71]"  # K descriptor of the tile being requested
SVD = "s[72:75]"  # V descriptor
SKP = ("s76", "s77")  # next K tile to request: byte address
SVP = ("s78", "s79")
SKR = "s80"       # bytes of K from that tile to the end of the slice
SVR = "s81"
SM0 = "s82"       # saved m0
SVOTE = "s[84:85]"
SVOTE2 = "s[86:87]"
SMASK = ["s[88:89]", "s[90:91]"]
SPAR = "s66"      # buffer parity of the current period: (i + boff) & 1
N_NEXT = 12 + 16  # vector-memory ops of the next-unit requests (3 tiles x 4 pieces, 16 Q loads)

LEADK = 3  # K fragments in flight ahead of their MFMAs
LEADV = 3


def elem_order():
    """The 64 softmax elements (rb, t, i) of a lane in 16-key-step order: kk-major, then rb."""
    out = []
    for kk in range(4):
        for rb in range(2):
            for j in range(8):
                out.append((kk, rb, kk >> 1, (kk & 1) * 8 + j))
    return out


def descriptors(e):
    """K / V descriptors of the tile being requested; the cursors move one tile on (shared with
    the dQ statement, dq.py)."""
    for (p0, p1), rem, d in ((SKP, SKR, 68), (SVP, SVR, 72)):
        e.salu(f"s_mov_b32 s{d}, {p0}")
        e.salu(f"s_and_b32 s{d + 1}, {p1}, 0xffff")
        e.salu(f"s_max_i32 s{d + 2}, {rem}, 0")
        e.salu(f"s_mov_b32 s{d + 3}, 0x20000")
        e.salu(f"s_add_u32 {p0}, {p0}, %[tileb]")
        e.salu(f"s_addc_u32 {p1}, {p1}, 0")
        e.salu(f"s_sub_i32 {rem}, {rem}, %[tileb]")


class FwdGen:
    """Q enters unscaled and every score gets z = s (scale log2 e) - m_ref in fp32 (one
    v_fma_f32, in the PV phase beside the row max), as the reference scales qk in fp32."""

    def __init__(self, bf16, causal, stamp=False, dropout=False):
        self.bf16, self.causal, self.stamp = bf16, causal, stamp
        # dropout: P is multiplied by the keep bits a dropout_mask_kernel launch wrote just before
        # (misc.hip) -- the packed P halves of dropped elements zeroed after the row sums (which
        # are of the whole P, compute_row_blocks.py:76-79); 1 / (1 - p) in the epilogue
        self.dropout = dropout
        assert not (dropout and stamp)
        self.mop = "v_mfma_f32_32x32x16_bf16" if bf16 else "v_mfma_f32_32x32x16_f16"
        self.cvtop = "v_cvt_pk_bf16_f32" if bf16 else "v_cvt_pk_f16_f32"
        self.e = Emitter()

    # -- pieces ------------------------------------------------------------------------------
    def k_read(self, kbuf, m):
        """K fragment m (key half t = m // KS, k-step m % KS) of the buffer kbuf -> ring."""
        t, ks = m // KS, m % KS
        imm = kbuf * TILE + (ks >> 1) * 4096 + 32 * t * 64
        base = "%[kb1]" if ks & 1 else "%[kb0]"
        dst = KR(m % 4)
        self.e.ds_read(f"ds_read_b128 {dst}, {base} offset:{imm}", dst)

    def v_read(self, vbuf, m, half):
        """Half `half` of V^T fragment m (kk = m // NDT, dt = m % NDT) of V buffer vbuf -> ring."""
        kk, dt = m // NDT, m % NDT
        imm = 2 * TILE + vbuf * TILE + dt * 4096 + 16 * kk * 64
        base = "%[vb]" if half else "%[va]"
        dst = VR(m % 4, half)
        self.e.ds_read(f"ds_read_b64_tr_b16 {dst}, {base} offset:{imm}", dst)

    def exp(self, st, el):
        kk, rb, t, i = el
        r = S(st, rb, t, i)
        self.e.valu(f"v_exp_f32 {r}, {r}", r, [r], kind="trans")

    def cvt(self, st, rb, kk, j):
        t, i0 = kk >> 1, (kk & 1) * 8 + 2 * j
        a, b = S(st, rb, t, i0), S(st, rb, t, i0 + 1)
        d = PF(rb, kk, j)
        self.e.valu(f"{self.cvtop} {d}, {a}, {b}", d, [a, b])

    def add(self, st, el, c):
        kk, rb, t, i = el
        r = S(st, rb, t, i)
        l = LSUM[rb][c]
        self.e.valu(f"v_add_f32 {l}, {l}, {r}", l, [l, r])

    # -- dropout keep words ----------------------------------------------------------------------
    def word_load(self, s, rb, t):
        """Keep word of the lane's row in block rb, 32-key half t, of the tile at byte offset s96
        (tiled layout of fa2_amd.h: tile i at + 256 i, half t at + 128 t) -> W[s][rb][t]."""
        self.e.raw(f"buffer_load_dword {FW_W(s, rb, t)}, %[mvo{rb}], {FW_MD}, {FW_MT} offen offset:{128 * t}")

    def word_load_items(self, s):
        """The next tile's four words -> set s (issue cost 8 each), then s96 moves one tile on."""
        out = []
        for n, (rb, t) in enumerate((rb, t) for rb in range(2) for t in range(2)):
            def f(rb=rb, t=t, n=n):
                self.word_load(s, rb, t)
                if n == 3:
                    self.e.salu(f"s_add_u32 {FW_MT}, {FW_MT}, 256")
            out.append(f)
        return out

    def mask_prep_items(self, cur, rb, t):
        """W >>= 4 hh (this lane's 16 keys at bits (i & 3) + 8 (i >> 2)); MC[rb][c] = the byte mask
        whose byte n is 0xFF iff bit c + 8 n of W is set: v_perm_b32's sign selectors replicate
        bits 15 / 31 of either source into a byte, so with S1 = W << (15 - c) (bits c, c + 16 at
        15, 31) and S0 = W << (7 - c) (bits c + 8, c + 24 at 15, 31) the selector 0x0B090A08
        (s97) builds it in one instruction (bench_micro/sdwa_sext_test.hip pins it)."""
        e = self.e
        w_ = FW_W(cur, rb, t)
        tmp = FW_TMP[rb]
        out = [lambda: e.valu(f"v_lshrrev_b32 {w_}, %[hh4], {w_}", w_, [w_])]
        for c in range(4):
            mc = FW_MC(rb, c)
            out.append(lambda c=c, mc=mc: e.valu(f"v_lshlrev_b32 {mc}, {15 - c}, {w_}", mc, [w_]))
            out.append(lambda c=c: e.valu(f"v_lshlrev_b32 {tmp}, {7 - c}, {w_}", tmp, [w_]))
            out.append(lambda mc=mc: e.valu(f"v_perm_b32 {mc}, {tmp}, {mc}, {FW_SEL}", mc, [tmp, mc]))
        return out

    def mask_and(self, rb, kk, j, h):
        """Zero half h of the P pack PF[rb][kk][j] (element i = 8 (kk & 1) + 2 j + h) unless its keep
        bit is set: AND with the sign-extended byte i >> 2 (0x00 / 0xFF) of MC[rb][i & 3] (SDWA
        writes the low 16 bits of the result to the selected word: P's word is selected on the
        source too; a byte's sign extension keeps its low 7 bits, hence whole-byte masks)."""
        i = 8 * (kk & 1) + 2 * j + h
        pp, mc = PF(rb, kk, j), FW_MC(rb, i & 3)
        self.e.valu(f"v_and_b32_sdwa {pp}, sext({mc}), {pp} dst_sel:WORD_{h} dst_unused:UNUSED_PRESERVE "
                    f"src0_sel:BYTE_{i >> 2} src1_sel:WORD_{h}", pp, [mc, pp])

    def mask_and_items(self, rb, kk):
        return [lambda j=j, h=h: self.mask_and(rb, kk, j, h) for j in range(4) for h in range(2)]

    def mask_elem(self, st, rb, t, i):
        """z = key offset o < rel[rb] ? z : -inf  (o = 32 t + (i & 3) + 8 (i >> 2))."""
        o = 32 * t + (i & 3) + 8 * (i >> 2)
        r = S(st, rb, t, i)
        sm = SMASK[i & 1]
        e = self.e
        e.valu(f"v_cmp_gt_i32_e64 {sm}, {REL[rb]}, {o}", None, [REL[rb]])
        e.valu(f"v_cndmask_b32_e64 {r}, {VNINF}, {r}, {sm}", r, [r, VNINF])

    def fma_z(self, st, rb, t, i):
        """z = s (scale log2 e) - m_ref in place (-m_ref kept in INIT(rb, 0))."""
        r = S(st, rb, t, i)
        self.e.valu(f"v_fma_f32 {r}, {r}, %[uz], {INIT(rb, 0)}", r, [r, INIT(rb, 0)])

    def max_ops_z(self, st, rb, t):
        """The row-max chain of (rb, half t), 16 values -> 8 instructions, each value's fma right
        after the max op that read it: ("max", text, dst, srcs) and ("fma", rb, t, i) entries."""
        v = [S(st, rb, t, i) for i in range(16)]
        m = MAH[rb][t]
        ops = [(f"v_max3_f32 {m}, {v[0]}, {v[1]}, {v[2]}", m, v[0:3])]
        for k in range(3, 15, 2):
            ops.append((f"v_max3_f32 {m}, {m}, {v[k]}, {v[k + 1]}", m, [m, v[k], v[k + 1]]))
        ops.append((f"v_max_f32 {m}, {m}, {v[15]}", m, [m, v[15]]))
        covered = [[0, 1, 2]] + [[k, k + 1] for k in range(3, 15, 2)] + [[15]]
        out = []
        for op, els in zip(ops, covered):
            out.append(("max",) + op)
            for i in els:
                out.append(("fma", rb, t, i))
        return out

    def row_max_finish(self):
        """mx[rb] = max over the lane pair of max(MAH[rb][0], MAH[rb][1]), converted to the
        exponent-argument domain: mx s scale log2 e - m_ref."""
        for f in self.row_max_finish_items():
            f()

    def rescale(self, st, first=False):
        """Defer-max rescale: for each row block, m_new = max(m_run, mx + m_ref), m_use = m_new or
        0 when -inf; O, l *= exp2(m_run - m_use); z of set st -= m_use - m_ref; INIT = -m_use.
        first: the unit's first tile (O and l are still zero: nothing to scale)."""
        e = self.e
        t_new, t_use, t_alpha, t_shift = TMP[0], TMP[1], TMP[2], TMP[3]
        # free during a rescale: the row-max chains and the mask limits (MX is still read)
        scratch = [TMP[4], MAH[0][0], MAH[0][1], MAH[1][0], MAH[1][1], REL[0], REL[1]]
        for rb in range(2):
            e.valu(f"v_add_f32 {t_new}, {MX[rb]}, {MREF[rb]}", t_new, [MX[rb], MREF[rb]])
            e.valu(f"v_max_f32 {t_new}, {MRUN[rb]}, {t_new}", t_new, [MRUN[rb], t_new])
            e.valu(f"v_cmp_eq_f32_e32 vcc, {VNINF}, {t_new}", None, [VNINF, t_new])
            e.valu(f"v_cndmask_b32_e64 {t_use}, {t_new}, 0, vcc", t_use, [t_new])
            e.valu(f"v_sub_f32 {t_shift}, {t_use}, {MREF[rb]}", t_shift, [t_use, MREF[rb]])
            if not first:
                e.valu(f"v_sub_f32 {t_alpha}, {MRUN[rb]}, {t_use}", t_alpha, [MRUN[rb], t_use])
                e.valu(f"v_exp_f32 {t_alpha}, {t_alpha}", t_alpha, [t_alpha], kind="trans")
                for c in range(2):
                    e.valu(f"v_mul_f32 {LSUM[rb][c]}, {t_alpha}, {LSUM[rb][c]}", LSUM[rb][c], [t_alpha, LSUM[rb][c]])
            # O[rb] *= alpha, in groups of len(scratch)
            regs = [] if first else [O(rb, dt, i) for dt in range(NDT) for i in range(16)]
            g = len(scratch)
            for k in range(0, len(regs), g):
                grp = regs[k:k + g]
                for a_, v_ in zip(grp, scratch):
                    e.valu(f"v_accvgpr_read_b32 {v_}, {a_}", v_, [a_], kind="accr")
                for a_, v_ in zip(grp, scratch):
                    e.valu(f"v_mul_f32 {v_}, {t_alpha}, {v_}", v_, [t_alpha, v_])
                for a_, v_ in zip(grp, scratch):
                    e.valu(f"v_accvgpr_write_b32 {a_}, {v_}", a_, [v_], kind="accw")
            for t in range(2):
                for i in range(16):
                    r = S(st, rb, t, i)
                    e.valu(f"v_sub_f32 {r}, {r}, {t_shift}", r, [r, t_shift])
            e.valu(f"v_mov_b32 {MRUN[rb]}, {t_new}", MRUN[rb], [t_new])
            e.valu(f"v_mov_b32 {MREF[rb]}, {t_use}", MREF[rb], [t_use])
            e.valu(f"v_sub_f32 {THR[rb]}, {t_new}, {t_use}", THR[rb], [t_new, t_use])
            e.valu(f"v_add_f32_e32 {THR[rb]}, 0x41000000, {THR[rb]}", THR[rb], [THR[rb]])
            e.valu(f"v_sub_f32 {INIT(rb, 0)}, 0, {t_use}", INIT(rb, 0), [t_use])

    def vote_and_rescale(self, st, tag):
        """One wave vote: any row of either block whose max outgrew its threshold -> rescale."""
        e = self.e
        e.valu(f"v_cmp_gt_f32_e64 {SVOTE}, {MX[0]}, {THR[0]}", None, [MX[0], THR[0]])
        e.valu(f"v_cmp_gt_f32_e64 {SVOTE2}, {MX[1]}, {THR[1]}", None, [MX[1], THR[1]])
        e.salu(f"s_or_b64 {SVOTE}, {SVOTE}, {SVOTE2}")
        e.raw(f"s_cbranch_scc0 .Lhp%=_{tag}_nr")
        self.rescale(st)
        e.label(f".Lhp%=_{tag}_nr")

    # -- s_memtime stamps (FA2_HP_STAMPS development builds only) ---------------------------------
    # per period: s[96:97] = its start (after the previous barrier), s[92:93] = the start of phase
    # Y (PV), s[94:95] = its end before the period-end waits; sums: s98 = phase X cycles, s99 =
    # phase Y + tail, %[st2] = prologue wait + every period-end wait and barrier
    def stamp_end_pre(self):
        e = self.e
        e.raw("s_memtime s[94:95]")
        e.drain_lds()
        e.raw("s_waitcnt lgkmcnt(0)")
        e.raw("s_sub_u32 s93, s94, s92")
        e.raw("s_add_u32 s99, s99, s93")
        e.raw("s_sub_u32 s92, s92, s96")
        e.raw("s_add_u32 s98, s98, s92")

    def stamp_end_post(self):
        e = self.e
        e.raw("s_memtime s[96:97]")
        e.raw("s_waitcnt lgkmcnt(0)")
        e.raw("s_sub_u32 s92, s96, s94")
        e.raw("s_add_u32 %[st2], %[st2], s92")

    def barrier(self):
        e = self.e
        if self.stamp:
            self.stamp_end_pre()
        e.drain_lds()
        e.raw("s_waitcnt vmcnt(0)")
        e.raw("s_barrier")
        if self.stamp:
            self.stamp_end_post()
        e.reset()

    # -- phases --------------------------------------------------------------------------------
    def qk_prologue(self, st):
        """S(0) = K(0) Q^T into set st (K(0) in K buffer st), fragments read LEADK ahead; no
        fillers."""
        nk = 2 * KS
        for m in range(LEADK):
            self.k_read(st, m)
        for m in range(nk):
            if m + LEADK < nk:
                self.k_read(st, m + LEADK)
            for rb in range(2):
                self.qk_mfma(st, 2 * m + rb)

    def qk_mfma(self, st, g):
        """QK^T MFMA g of a tile: S[st][rb][t] += K fragment m = g >> 1 (ring slot m % 4) Q^T(rb, ks)."""
        m, rb = g >> 1, g & 1
        t, ks = m // KS, m % KS
        d = S(st, rb, t)
        self.e.mfma(self.mop, d, KR(m % 4), f"%[q{rb * KS + ks}]", "0" if ks == 0 else d)

    def pv_mfma(self, g):
        """PV MFMA g of a tile: O^T[rb][dt] += V^T fragment m = g >> 1 (ring slot m % 4) P(rb, kk)."""
        m, rb = g >> 1, g & 1
        kk, dt = m // NDT, m % NDT
        self.e.mfma(self.mop, O(rb, dt), VR(m % 4), PF(rb, kk), O(rb, dt))

    def max_mask_plain(self, st, masked):
        """Mask (masked tiles) and row max of set st, no MFMA cover (prologue)."""
        e = self.e
        if masked:
            for rb in range(2):
                e.valu(f"v_subrev_u32 {REL[rb]}, {SN1}, %[rel{rb}]", REL[rb], [])
        for rb in range(2):
            for t in range(2):
                if masked:
                    for i in range(16):
                        self.mask_elem(st, rb, t, i)
                for op in self.max_ops_z(st, rb, t):
                    if op[0] == "max":
                        e.valu(op[1], op[2], op[3])
                    else:
                        self.fma_z(st, *op[1:])
        self.row_max_finish()

    def period_end(self, final):
        e = self.e
        e.salu(f"s_add_i32 {SI}, {SI}, 1")
        e.salu(f"s_add_i32 {SN1}, {SN1}, 64")
        e.salu(f"s_xor_b32 {SPAR}, {SPAR}, 1")
        if final:
            if self.stamp:
                self.stamp_end_pre()
            # the next unit's loads stay in flight across the epilogue (its statement waits)
            e.drain_lds()
            e.raw(f"s_waitcnt vmcnt({N_NEXT})")
            e.raw("s_barrier")
            if self.stamp:
                self.stamp_end_post()
            e.reset()
        else:
            self.barrier()

    def next_unit_items(self, par):
        """The final period's requests: the NEXT unit's K(0) -> K buffer 1-par, V(0) -> V buffer
        1-par, K(1) -> K buffer par (all free in the final period), and its Q fragments straight
        into the Q accumulation registers (%[q*], read-write operands); N_NEXT vector-memory ops.
        Without a next unit the descriptors have range 0 (no memory access)."""
        e = self.e
        pieces = [(1 - par, "k0"), (1 - par, "v0"), (par, "k1")]

        def lds_of(buf, what, it):
            return (2 * TILE if what == "v0" else 0) + buf * TILE + it * 4096

        seq = [(buf, what, it) for buf, what in pieces for it in range(NDT)]
        out = []

        def desc(what):
            # s[68:71] next K tile 0 / 1, s[72:75] next V tile 0
            d = 72 if what == "v0" else 68
            return f"s[{d}:{d + 3}]"

        def build_desc():
            e.salu("s_mov_b32 s68, %[nklo]")
            e.salu("s_and_b32 s69, %[nkhi], 0xffff")
            e.salu("s_mov_b32 s70, %[nkbytes]")
            e.salu("s_mov_b32 s71, 0x20000")
            e.salu("s_mov_b32 s72, %[nvlo]")
            e.salu("s_and_b32 s73, %[nvhi], 0xffff")
            e.salu("s_mov_b32 s74, %[nkbytes]")
            e.salu("s_mov_b32 s75, 0x20000")
        out.append((8, build_desc))
        for n, (buf, what, it) in enumerate(seq):
            def f(n=n, buf=buf, what=what, it=it):
                if n == 0:
                    e.salu(f"s_add_u32 m0, %[mlds], {lds_of(buf, what, it)}", m0=True)
                if n == 2 * NDT:  # tile 1 of K: one tile further, range one tile shorter
                    e.salu("s_add_u32 s68, s68, %[tileb]")
                    e.salu("s_addc_u32 s69, s69, 0")
                    e.salu("s_sub_i32 s70, s70, %[tileb]")
                    e.salu("s_max_i32 s70, s70, 0")
                e.dma(f"buffer_load_dwordx4 %[off{it}], {desc(what)}, 0 offen lds")
                if n + 1 < len(seq):
                    e.salu(f"s_add_u32 m0, %[mlds], {lds_of(*seq[n + 1])}", m0=True)
            out.append((16, f))

        def qdesc():
            e.salu("s_mov_b32 s72, %[nqlo]")
            e.salu("s_and_b32 s73, %[nqhi], 0xffff")
            e.salu("s_mov_b32 s74, %[nqbytes]")
            e.salu("s_mov_b32 s75, 0x20000")
        out.append((8, qdesc))
        for rb in range(2):
            for ks in range(KS):
                def f(rb=rb, ks=ks):
                    e.raw(f"buffer_load_dwordx4 %[q{rb * KS + ks}], %[nqo{rb}], s[72:75], 0 offen offset:{32 * ks}")
                out.append((16, f))
        return out

    def period_c(self, par, final=False):
        """One period i (parity par) of class C (no tile i+1): the exponentials and packs of tile
        i with no MFMA to ride on, then the PV(i) MFMAs with the row sums of tile i as fillers
        (`GapScheduler`).  The classes A (tile i+1 live, unmasked) and B (live, masked) are
        period_xy_bal."""
        e = self.e
        cur, vbuf = par, par
        E = elem_order()
        if final:
            dma = self.next_unit_items(par)
        else:
            descriptors(e)
            dma = self.dma_stream(par)
        # ---------------- phase X (no QK^T: nothing to schedule around) ----------------
        for el in E:
            self.exp(cur, el)
        for _, f in dma:
            f()
        for kk in range(4):
            for rb in range(2):
                for j in range(4):
                    self.cvt(cur, rb, kk, j)
        if self.dropout:
            for rb in range(2):
                for t in range(2):
                    for f in self.mask_prep_items(cur, rb, t):
                        f()
                    for kk in (2 * t, 2 * t + 1):
                        for f in self.mask_and_items(rb, kk):
                            f()
        for m in range(LEADV):
            for h in range(2):
                self.v_read(vbuf, m, h)
        if self.stamp:
            e.raw("s_memtime s[92:93]")
        # ---------------- phase Y ----------------
        nv = 4 * NDT            # V^T fragments per tile (two MFMAs each)
        ny = 2 * nv             # phase Y MFMAs
        gy = GapScheduler(ny)
        for m in range(nv):
            if m + LEADV < nv:
                for h in range(2):
                    gy.add("v", 4, 2 * m, 2 * m + 1, lambda m=m, h=h: self.v_read(vbuf, m + LEADV, h))
        for n, el in enumerate(E):
            gy.add(f"add{n % 2}", 4, 0, ny - 1, lambda el=el, c=n % 2: self.add(cur, el, c))
        gy.run(self.pv_mfma, pre_budget=0)
        self.period_end(final)

    def row_max_finish_items(self):
        """row_max_finish as a list of emit functions (scheduled into the last PV gaps)."""
        e = self.e
        out = []
        for rb in range(2):
            out.append(lambda rb=rb: e.valu(f"v_max_f32 {MX[rb]}, {MAH[rb][0]}, {MAH[rb][1]}", MX[rb], MAH[rb]))
            out.append(lambda rb=rb: e.valu(f"v_mov_b32 {TMP[rb]}, {MX[rb]}", TMP[rb], [MX[rb]]))
        for rb in range(2):
            out.append(lambda rb=rb: e.valu(f"v_permlane32_swap_b32 {MX[rb]}, {TMP[rb]}", [MX[rb], TMP[rb]],
                                            [MX[rb], TMP[rb]], kind="perm"))
        for rb in range(2):
            out.append(lambda rb=rb: e.valu(f"v_max_f32 {MX[rb]}, {MX[rb]}, {TMP[rb]}", MX[rb], [MX[rb], TMP[rb]]))
        for rb in range(2):
            out.append(lambda rb=rb: e.valu(f"v_fma_f32 {MX[rb]}, {MX[rb]}, %[uz], {INIT(rb, 0)}", MX[rb],
                                            [MX[rb], INIT(rb, 0)]))
        return out

    def period_xy_bal(self, par, cls, tag):
        """One period i (parity par) of class A (tile i+1 live, unmasked) or B (live, masked):
        phase X = QK^T(i+1) MFMAs, phase Y = PV(i) MFMAs, with the fillers balanced over both
        phases (round 6).  The fillers of each MFMA gap come from `GapScheduler` (deadline-ordered,
        issue-cost budget per gap).

        The round-5 schedule put 56 of the 64 exponentials of tile i into phase X (two or three per
        MFMA gap, where one v_exp per gap hides) and left phase Y with every row sum and the whole
        mask / row max / exponent-argument pass of tile i+1 -- more than its 32 gaps hold, so ~60
        instructions ran after its last MFMA (s_memtime stamps, profiles/r06a_fwd_stamps_ablations.jsonl:
        X 1369 and Y 1400 cycles per period against 1024 of MFMAs).  Here:
          X: K fragment reads (issued first in the period, before the descriptor updates), the
             exponentials of E[0:40] (kk = 0, 1 and half of kk = 2), the packs of kk = 0 and 1, the row
             sums of kk = 0, the LDS-DMA pieces, and -- once the chains S(i+1)[rb][t = 0] are complete
             (MFMAs 14, 15) -- the t = 0 half of the mask / row max / exponent arguments of tile i+1;
          Y: the remaining 24 exponentials, the kk = 2, 3 packs, the other row sums, the t = 1 half of
             the next tile's pass, and the row-max finish in its last gaps (the vote after the last
             MFMA).
        Every cross-stream dependence is a release after the producer's deadline (a stream orders
        only itself)."""
        e = self.e
        cur, nxt = par, 1 - par
        kbuf, vbuf = 1 - par, par
        masked = cls == "B"
        E = elem_order()
        nk, nx, nv = 2 * KS, 4 * KS, 4 * NDT
        ny = 2 * nv
        # development timing ablations of the steady-state (class A) period: FA2_HPGEN_ABL=fw_*
        # (wrong outputs; cycles only, read with the stamp build)
        drops = {"fw_nodma": r"^buffer_load|^s_add_u32 m0", "fw_noexp": r"^v_exp",
                 "fw_novalu": r"^v_(?!mfma)", "fw_nolds": r"^ds_read", "fw_nosalu": r"^s_(?!waitcnt|barrier|cbranch|nop|branch)"}
        pat = "|".join(v for k, v in drops.items() if k in ABL) if cls == "A" else ""
        e.drop = re.compile(pat) if pat else None
        # the first K fragments first: their LDS latency runs under the scalar updates below
        for m in range(LEADK):
            self.k_read(kbuf, m)
        descriptors(e)
        dma = self.dma_stream(par)
        if masked:
            for rb in range(2):
                e.valu(f"v_subrev_u32 {REL[rb]}, {SN1}, %[rel{rb}]", REL[rb], [])

        def zprep(add, t, rb, release, deadline):
            st_ = f"mx{t}{rb}"
            if masked:
                for i in range(16):
                    add(st_, 8, release, deadline, lambda rb=rb, t=t, i=i: self.mask_elem(nxt, rb, t, i))
            for op in self.max_ops_z(nxt, rb, t):
                if op[0] == "max":
                    add(st_, 4, release, deadline, lambda op=op: e.valu(op[1], op[2], op[3]))
                else:
                    add(st_, 4, release, deadline, lambda op=op: self.fma_z(nxt, *op[1:]))

        # ---------------- phase X ----------------
        n_x = 40
        x_dl = {n: (n * 28) // n_x for n in range(n_x)}
        gx = GapScheduler(nx)
        for m in range(nk):
            if m + LEADK < nk:
                gx.add("k", 4, 2 * m, 2 * m, lambda m=m: self.k_read(kbuf, m + LEADK))
        # (released one gap before the deadline: about one exponential per gap instead of a burst of
        # three, MI355X_MICROARCH.md filler rule "at most one v_exp per MFMA gap")
        for n in range(n_x):
            gx.add("exp", 8, x_dl[n] - 1, x_dl[n], lambda el=E[n]: self.exp(cur, el))
        for n, f in enumerate(dma):
            gx.add("dma", f[0], -1, min(nx - 1, (4 * n + 3) * nx // 32), f[1])
        # dropout: the kk = 0 packs early enough for their keep masking in phase X (X_CVT0); the
        # next tile's keep words requested at the period start
        X_CVT0 = 20
        for kk in (0, 1):
            for rb in range(2):
                for j in range(4):
                    idx = [16 * kk + 8 * rb + 2 * j, 16 * kk + 8 * rb + 2 * j + 1]
                    gx.add(f"cvt{kk}", 4, max(x_dl[i] for i in idx) + 1, X_CVT0 if self.dropout and kk == 0 else nx - 1,
                        lambda c=(rb, kk, j): self.cvt(cur, *c))
        if self.dropout:
            for f in self.word_load_items(nxt):
                gx.add("wl", 8, -1, 6, f)
            for rb in range(2):
                for f in self.mask_prep_items(cur, rb, 0):
                    gx.add(f"dm{rb}", 4, -1, X_CVT0 - 2, f)
                for f in self.mask_and_items(rb, 0):
                    gx.add(f"dm{rb}", 4, X_CVT0 + 1, nx - 1, f)
        for n in range(16):
            gx.add(f"add{n % 2}", 4, x_dl[n] + 1, nx - 1, lambda el=E[n], c=n % 2: self.add(cur, el, c))
        for m in range(LEADV):
            for h in range(2):
                gx.add("vr", 4, max(0, nx - 12), nx - 1, lambda m=m, h=h: self.v_read(vbuf, m, h))
        # S(i+1)[rb][0] is complete after MFMA 14 + rb
        for rb in range(2):
            zprep(gx.add, 0, rb, 17 + rb, nx - 1)

        # (before the first MFMA the wave waits for its first K fragment anyway: room for fillers)
        gx.run(lambda g: self.qk_mfma(nxt, g), pre_budget=64)
        if self.stamp:
            e.raw("s_memtime s[92:93]")
        # ---------------- phase Y ----------------
        gy = GapScheduler(ny)
        for m in range(nv):
            if m + LEADV < nv:
                for h in range(2):
                    gy.add("v", 4, 2 * m, 2 * m + 1, lambda m=m, h=h: self.v_read(vbuf, m + LEADV, h))
        # (dropout: exponentials and packs earlier, so that the keep masking of a pack fits between
        # it and the first PV MFMA reading it, MFMA 8 kk)
        y_span = 16 if self.dropout else 20
        y_dl = {n: ((n - n_x) * y_span) // (64 - n_x) for n in range(n_x, 64)}
        for n in range(n_x, 64):
            gy.add("exp", 8, y_dl[n] - 1, y_dl[n], lambda el=E[n]: self.exp(cur, el))
        # packs of P(kk) before the first PV MFMA reading them (MFMA 8 kk; margin for VALU -> MFMA)
        y_cvt = (9, 17) if self.dropout else (13, 21)
        for kk in (2, 3):
            for rb in range(2):
                for j in range(4):
                    idx = [16 * kk + 8 * rb + 2 * j, 16 * kk + 8 * rb + 2 * j + 1]
                    rel = max([y_dl[i] for i in idx if i in y_dl] + [-2]) + 1
                    gy.add(f"cvt{kk}", 4, rel, y_cvt[kk - 2], lambda c=(rb, kk, j): self.cvt(cur, *c))
        if self.dropout:
            for rb in range(2):
                for f in self.mask_and_items(rb, 1):
                    gy.add(f"dm{rb}", 4, -1, 5, f)
                for f in self.mask_prep_items(cur, rb, 1):
                    gy.add(f"dm{rb}", 4, -1, 8, f)
                for kk in (2, 3):
                    for f in self.mask_and_items(rb, kk):
                        gy.add(f"dm{rb}", 4, y_cvt[kk - 2] + 1, 8 * kk - 2, f)
        for n in range(16, 64):
            rel = y_dl[n] + 1 if n in y_dl else -1
            gy.add(f"add{n % 2}", 4, rel, ny - 1, lambda el=E[n], c=n % 2: self.add(cur, el, c))
        for rb in range(2):
            zprep(gy.add, 1, rb, -1, ny - 4)
        for f in self.row_max_finish_items():
            gy.add("rmf", 4, ny - 3, ny - 1, f)
        gy.run(self.pv_mfma, pre_budget=0)
        self.vote_and_rescale(nxt, tag)
        e.drop = None
        self.period_end(False)

    def dma_stream(self, par):
        """The period's 8 LDS-DMA pieces as (cost, emit) items; each item issues its piece and
        already points m0 at the next one, so no piece waits on its own m0 write."""
        pieces = [("k", it) for it in range(NDT)] + [("v", it) for it in range(NDT)]

        def m0_of(w_, it):
            return par * TILE + it * 4096 if w_ == "k" else 2 * TILE + (1 - par) * TILE + it * 4096

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

    def period_d(self, par, final=False):
        if self.stamp:
            self.e.raw("s_memtime s[92:93]")
        if final:
            items = self.next_unit_items(par)
        else:
            descriptors(self.e)
            items = self.dma_stream(par)
        for _, f in items:
            f()
        self.period_end(final)

    # -- one work unit (256 query rows), persistent across units --------------------------------
    def build(self):
        e = self.e
        e.raw("s_nop 7")
        e.raw("s_nop 7")
        if self.stamp:
            e.raw("s_memtime s[100:101]")
            e.raw("s_mov_b32 s98, 0")
            e.raw("s_mov_b32 s99, 0")
        e.salu(f"s_mov_b32 {SM0}, m0")
        e.valu(f"v_mov_b32 {VNINF}, {NINF}", VNINF)
        for rb in range(2):
            e.valu(f"v_mov_b32 {MRUN[rb]}, {NINF}", MRUN[rb])
            e.valu(f"v_mov_b32 {THR[rb]}, {NINF}", THR[rb])
            e.valu(f"v_mov_b32 {MREF[rb]}, 0", MREF[rb])
            for c in range(2):
                e.valu(f"v_mov_b32 {LSUM[rb][c]}, 0", LSUM[rb][c])
            e.valu(f"v_mov_b32 {INIT(rb, 0)}, 0", INIT(rb, 0))
        for rb in range(2):
            for dt in range(NDT):
                for i in range(16):
                    e.valu(f"v_accvgpr_write_b32 {O(rb, dt, i)}, 0", O(rb, dt, i), kind="accw")
        # DMA cursors: period i requests K(i + 2) and V(i + 1)
        e.salu(f"s_mov_b32 {SKP[0]}, %[klo]")
        e.salu(f"s_mov_b32 {SKP[1]}, %[khi]")
        e.salu(f"s_mov_b32 {SVP[0]}, %[vlo]")
        e.salu(f"s_mov_b32 {SVP[1]}, %[vhi]")
        e.salu(f"s_mov_b32 {SKR}, %[kbytes]")
        e.salu(f"s_mov_b32 {SVR}, %[kbytes]")
        for k in range(2):
            e.salu(f"s_add_u32 {SKP[0]}, {SKP[0]}, %[tileb]")
            e.salu(f"s_addc_u32 {SKP[1]}, {SKP[1]}, 0")
            e.salu(f"s_sub_i32 {SKR}, {SKR}, %[tileb]")
        e.salu(f"s_add_u32 {SVP[0]}, {SVP[0]}, %[tileb]")
        e.salu(f"s_addc_u32 {SVP[1]}, {SVP[1]}, 0")
        e.salu(f"s_sub_i32 {SVR}, {SVR}, %[tileb]")
        e.salu(f"s_mov_b32 {SI}, 0")
        e.salu(f"s_mov_b32 {SN1}, 0")
        e.salu(f"s_mov_b32 {SPAR}, %[boff]")
        if self.dropout:
            # the keep-mask descriptor; tile 0's words into both sets (its period's parity is boff)
            e.salu("s_mov_b32 s92, %[mlo]")
            e.salu("s_mov_b32 s93, %[mhi]")
            e.salu("s_mov_b32 s94, %[mbytes]")
            e.salu("s_mov_b32 s95, 0x20000")
            e.salu(f"s_mov_b32 {FW_MT}, 0")
            e.salu(f"s_mov_b32 {FW_SEL}, 0x0b090a08")
            for s_ in range(2):
                for rb in range(2):
                    for t in range(2):
                        self.word_load(s_, rb, t)
            e.salu(f"s_mov_b32 {FW_MT}, 256")
        # this unit's K(0), V(0), K(1) and Q (requested during the previous unit's final period,
        # or before the statement) have landed
        e.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e.raw("s_barrier")
        if self.stamp:  # prologue wait (st2 then adds every period-end wait)
            e.raw("s_memtime s[92:93]")
            e.raw("s_waitcnt lgkmcnt(0)")
            e.raw("s_sub_u32 s92, s92, s100")
            e.raw("s_mov_b32 %[st2], s92")
        e.reset()
        # ---- prologue: S(0) in set boff (K(0) in K buffer boff) ----
        e.raw("s_cmp_lt_i32 %[last], 0")
        e.raw("s_cbranch_scc1 .Lhp%=_pro_end")
        for par in (0, 1):
            e.label(f".Lhp%=_pro{par}")
            if par == 0:
                e.raw(f"s_cmp_eq_u32 {SPAR}, 1")
                e.raw("s_cbranch_scc1 .Lhp%=_pro1")
            self.qk_prologue(par)
            e.drain_lds()
            e.drain_mfma()  # both paths below start with every S(0) result readable
            e.raw("s_cmp_eq_u32 %[mask0], 0")
            e.raw(f"s_cbranch_scc1 .Lhp%=_pro{par}_plain")
            self.max_mask_plain(par, True)
            self.rescale(par, first=True)
            e.raw("s_branch .Lhp%=_pro_end")
            e.label(f".Lhp%=_pro{par}_plain")
            self.max_mask_plain(par, False)
            self.rescale(par, first=True)
            e.raw("s_branch .Lhp%=_pro_end")
        e.label(".Lhp%=_pro_end")
        e.drain_mfma()
        e.raw("s_barrier")  # every wave is done with K(0) before K(2) lands in its buffer
        if self.stamp:  # the first period starts here
            e.raw("s_memtime s[96:97]")
            e.raw("s_waitcnt lgkmcnt(0)")
        e.reset()
        e.salu(f"s_mov_b32 {SN1}, 64")
        e.salu("s_add_i32 s67, %[ntiles], -1")  # s67: index of the final period
        e.raw("s_cmp_lt_i32 s67, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_noper")
        # ---- periods 0 .. ntiles-2: class by tile i+1, body by parity ----
        e.raw(".balignl 64, 0xbf800000", 0)  # loop head on a 64-byte boundary, padded with s_nop 0
        e.label(".Lhp%=_loop")
        e.raw(f"s_cmp_ge_i32 {SI}, s67")
        e.raw("s_cbranch_scc1 .Lhp%=_fin")
        e.raw(f"s_cmp_lt_i32 {SI}, %[na]")
        e.raw("s_cbranch_scc1 .Lhp%=_clsA")
        e.raw(f"s_cmp_lt_i32 {SI}, %[last]")
        e.raw("s_cbranch_scc1 .Lhp%=_clsB")
        e.raw(f"s_cmp_eq_u32 {SI}, %[last]")
        e.raw("s_cbranch_scc1 .Lhp%=_clsC")
        e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_D0")
        e.raw("s_branch .Lhp%=_D1")
        # class A runs as a chain: one compare and one (mostly not taken) branch per period
        e.label(".Lhp%=_clsA")
        e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_A1")
        e.label(".Lhp%=_A0")
        self.period_xy_bal(0, "A", "a0")
        e.raw(f"s_cmp_ge_i32 {SI}, %[na]")
        e.raw("s_cbranch_scc1 .Lhp%=_loop")
        e.label(".Lhp%=_A1")
        self.period_xy_bal(1, "A", "a1")
        e.raw(f"s_cmp_lt_i32 {SI}, %[na]")
        e.raw("s_cbranch_scc1 .Lhp%=_A0")
        e.raw("s_branch .Lhp%=_loop")
        for cls in ("B", "C"):
            e.label(f".Lhp%=_cls{cls}")
            e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
            e.raw(f"s_cbranch_scc0 .Lhp%=_{cls}1")
            for par in (0, 1):
                e.label(f".Lhp%=_{cls}{par}")
                if cls == "B":
                    self.period_xy_bal(par, "B", f"b{par}")
                else:
                    self.period_c(par)
                e.raw("s_branch .Lhp%=_loop")
        for par in (0, 1):
            e.label(f".Lhp%=_D{par}")
            self.period_d(par)
            e.raw("s_branch .Lhp%=_loop")
        # ---- the final period (i = ntiles - 1): class C or D, the next unit's requests ----
        e.label(".Lhp%=_fin")
        e.raw(f"s_cmp_eq_u32 {SI}, %[last]")
        e.raw("s_cbranch_scc0 .Lhp%=_finD")
        e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_finC1")
        for par in (0, 1):
            e.label(f".Lhp%=_finC{par}")
            self.period_c(par, final=True)
            e.raw("s_branch .Lhp%=_end")
        e.label(".Lhp%=_finD")
        e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
        e.raw("s_cbranch_scc0 .Lhp%=_finD1")
        for par in (0, 1):
            e.label(f".Lhp%=_finD{par}")
            self.period_d(par, final=True)
            e.raw("s_branch .Lhp%=_end")
        # ---- no period at all: the next unit's requests right away (every buffer is free) ----
        e.label(".Lhp%=_noper")
        e.raw(f"s_cmp_eq_u32 {SPAR}, 0")
        e.raw("s_cbranch_scc1 .Lhp%=_noper1")
        for par in (0, 1):
            # parity of a virtual final period: boff ^ 1
            if par == 1:
                e.label(".Lhp%=_noper1")
            for _, f in self.next_unit_items(par):
                f()
            e.raw("s_branch .Lhp%=_end")
        e.label(".Lhp%=_end")
        e.drain_lds()
        for rb in range(2):
            e.valu(f"v_mov_b32 %[mo{rb}], {MRUN[rb]}", None, [MRUN[rb]])
            e.valu(f"v_add_f32 %[lo{rb}], {LSUM[rb][0]}, {LSUM[rb][1]}", None, LSUM[rb])
        e.salu(f"s_mov_b32 m0, {SM0}")
        if self.stamp:
            e.raw("s_memtime s[92:93]")
            e.raw("s_waitcnt lgkmcnt(0)")
            e.raw("s_sub_u32 s92, s92, s100")
            e.raw("s_mov_b32 %[st0], s98")
            e.raw("s_mov_b32 %[st1], s99")
            e.raw("s_mov_b32 %[st3], s92")
        e.raw("s_nop 15")
        e.raw("s_nop 15")
        return e.out


def gen_fwd_function(bf16, causal, dropout=False):
    out = []
    nq = 2 * KS  # Q fragments (two row blocks x k-steps)
    for stamp in ((False,) if dropout else (False, True)):
        g = FwdGen(bf16, causal, stamp, dropout)
        lines = g.build()
        name = f"fwd_hp_main_{'bf16' if bf16 else 'f16'}_{'causal' if causal else 'full'}{'_drop' if dropout else ''}"
        # O^T a[0:127], K / V^T rings a[192:223]; every AGPR but the Q operands' (a[128:191])
        # clobbered, so the compiler has no room to move them
        clob = [f'"v{i}"' for i in range(N_VGPR)] + [f'"a{i}"' for i in AGPR_CLOBBER] + \
               [f'"s{i}"' for i in _sgprs_used(lines)] + ['"vcc"', '"scc"', '"memory"']
        qops = ", ".join(f'[q{i}] "+a"(q[{i}])' for i in range(nq))
        stops = ", " + ", ".join(f'[st{i}] "=&s"(st[{i}])' for i in range(4)) if stamp else ""
        starg = ", uint32_t (&st)[4]" if stamp else ""
        dops = ('\n        [mvo0] "v"(a.mvo[0]), [mvo1] "v"(a.mvo[1]), [hh4] "v"(a.hh4), [mlo] "s"(a.mlo), '
                '[mhi] "s"(a.mhi), [mbytes] "s"(a.mbytes),' if dropout else "")
        out.append(f"""{'#if FA2_HP_STAMPS' if stamp else '#if !FA2_HP_STAMPS'}
// hand-placed unit ({'bf16' if bf16 else 'fp16'}, {'causal' if causal else 'non-causal'}, exact scale{', dropout' if dropout else ''}{', stamped' if stamp else ''}): {len(lines)} lines, {g.e.n_mfma} MFMAs
// q: this unit's Q fragments in, the NEXT unit's Q fragments out -- still in flight (the next
// statement waits for them first; nothing may read q in between)
FA2_DEV void {name}(u32x4 (&q)[{nq}], const FwdHpArgs& a, float (&m_out)[2], float (&l_out)[2]{starg}) {{
  asm volatile(
{_asm_body(lines)}
      : [mo0] "=&v"(m_out[0]), [mo1] "=&v"(m_out[1]), [lo0] "=&v"(l_out[0]), [lo1] "=&v"(l_out[1]), {qops}{stops}
      : [kb0] "v"(a.kb0), [kb1] "v"(a.kb1), [va] "v"(a.va), [vb] "v"(a.vb),{dops}
        {", ".join(f'[off{i}] "v"(a.off[{i}])' for i in range(NDT))},
        [rel0] "v"(a.rel[0]), [rel1] "v"(a.rel[1]), [nqo0] "v"(a.nqo[0]), [nqo1] "v"(a.nqo[1]),
        [na] "s"(a.na), [last] "s"(a.last), [ntiles] "s"(a.ntiles), [mask0] "s"(a.mask0),
        [tileb] "s"(a.tileb), [kbytes] "s"(a.kbytes), [mlds] "s"(a.mlds),
        [klo] "s"(a.klo), [khi] "s"(a.khi), [vlo] "s"(a.vlo), [vhi] "s"(a.vhi), [uz] "s"(a.uz),
        [boff] "s"(a.boff), [nklo] "s"(a.nklo), [nkhi] "s"(a.nkhi), [nvlo] "s"(a.nvlo), [nvhi] "s"(a.nvhi),
        [nkbytes] "s"(a.nkbytes), [nqlo] "s"(a.nqlo), [nqhi] "s"(a.nqhi), [nqbytes] "s"(a.nqbytes)
      : {", ".join(clob)});
}}
#endif
""")
    return "".join(out)


# Each read statement clobbers every accumulator register: a value live across them (the next
# unit's Q / dO fragments, "+a" operands of the main statement) then cannot be placed in
# a[0:127] anywhere between the main statement and the last read -- the compiler moving one
# there early would overwrite accumulators not read yet (tests/test_code_objects.py checks the ISA).
ACC_CLOBBER = ", ".join(f'"a{i}"' for i in range(128))


def gen_read_o():
    parts = ["// O^T accumulators a[0:127] -> registers (after the main statement's final drain)",
             "FA2_DEV void fwd_hp_read_o(f32x16 (&o)[2][4]) {"]
    for rb in range(2):
        for dt in range(4):
            base = (rb * 4 + dt) * 16
            outs = ", ".join(f'"=v"(o[{rb}][{dt}][{i}])' for i in range(16))
            body = "".join(f"v_accvgpr_read_b32 %{i}, a{base + i}\\n" for i in range(16))
            parts.append(f'  asm volatile("{body}" : {outs} : : {ACC_CLOBBER});')
    parts.append("}")
    return "\n".join(parts) + "\n"
