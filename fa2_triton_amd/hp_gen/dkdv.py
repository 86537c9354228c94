"""The dK / dV statements (dkdv_hp_kernel): LDS layout, register map, `DkdvGen`."""
from . import ABL
from .emitter import Emitter, GapScheduler, _asm_body, _sgprs_used, rng

# ----------------------------------------------------------------------------------------------
# dK / dV (the backward's dominant kernel): dkdv_hp_kernel (csrc/dkdv_hp_kernel.h)
#
# Software-pipelined step (round 5): the step i of a wave runs, between two barriers,
#   M 0-7    the last 8 dK MFMAs of step i-1 (dK^T += Q^T dS for rows 16-31; operands read before
#            the barrier: the Q^T fragments in the row ring, the packed dS in registers), so the
#            step opens with MFMAs while its first LDS reads are in flight;
#   M 8-23   S(i+1) = Q(i+1) K^T into the other S register set (the NEXT step's scores);
#   M 24-39  dP(i) = dO(i) V^T, seeded with the -delta rows;
#   M 40-55  dV^T += dO(i)^T P(i);
#   M 56-63  dK^T += Q(i)^T dS(i), rows 0-15.
# so the exponentials of P(i) (whose S(i) the previous step computed) run beside M 0-47 and dS(i)
# beside M 41-63 (round 4 ran S(i) first and waited for it: the exponentials crowded 16 gaps).
#
# Register map of the statement:
#   v[0:63]     S[st][kb] (two sets by step parity): the next step's scores, then P = exp2(s scale
#               log2 e - LSE2) in place
#   v[64:95]    dP[kb] accumulators (start as -delta rows), then dS = P (dP - delta) in place, then
#               in place the packed dS DSP[kb][sp] (B operands of dK^T += Q^T dS)
#   v[96:111]   PP[kb][sp] packed P (B operand of dV^T += dO^T P)
#   v[112:127]  row-fragment ring, 4 slots: Q(i+1), dO(i), then the Q^T(i) fragments of rows 16-31
#               for the next step's first MFMAs
#   v[128:143]  V fragment ring (B operands of dP), 4 slots
#   v[144:159]  transposed fragment ring (dO^T, then Q^T of rows 0-15), 4 slots
#   v[160:167]  LSE2 of 8 of the lane's rows (rows of 16-row half sp, reloaded for sp = 1)
#   a[0:127]    dV^T[kb][dt], a[128:255] dK^T[kb][dt]
#   K fragments: compiler-placed "v" operands %[k0]..%[k15]
# LDS (bytes from the workgroup's base, DkLayout): a ring of nbuf = 5 step buffers -- step i
# reads buffers i and i + 1, its DMA fills buffer i + 3: Q tile of buffer b at 16384 b, dO tile at
# 16384 b + 8192 (Tile<128, 32>; buffer 4 through the "h" bases, 64 KiB up: a ds offset has 16
# bits), V rows of wave w at v0 + 16384 w (Tile<128, 64>), LSE2 / -delta rows of buffer b at
# rows + 256 b (+128).
# One barrier per TWO steps (after the odd ones): between the barriers after steps j - 2 and j
# (j odd) the steps j - 1 and j read buffers j - 1 .. j + 1 and request steps j + 2 and j + 3
# into the buffers of steps j - 3 and j - 2, which every wave finished reading before the
# barrier after step j - 2: five buffers.  At that barrier every request so far has landed
# (vmcnt(0): the odd step's own request is issued early in the step).  The S / P register set
# alternates per step, so the step bodies come in 10 phases (buffer ph % 5, set ph & 1).
# The dropout statement keeps four buffers and a barrier after every step (the "h" bases of
# buffer 4 would spill its VGPRs).
DK_NBUF_PLAIN = 5
DK_NBUF_DROP = 4


class DkLayout:
    """LDS layout of one dK/dV statement variant (bytes from the workgroup's base)."""

    def __init__(self, nbuf):
        self.nbuf = nbuf
        self.ph = nbuf if nbuf % 2 == 0 else 2 * nbuf  # step phases: buffer ph % nbuf, set ph & 1
        self.halfbar = nbuf == 5
        self.v0 = 16384 * nbuf
        self.rows = self.v0 + 65536
        self.lds = self.rows + 256 * nbuf
        self.w0 = self.lds  # dropout: keep words of buffer b, wave w at w0 + 1024 b + 256 w
        self.lds_drop = self.w0 + 1024 * nbuf


DK_AHEAD = 3  # a step's DMA fills the buffer of the step DK_AHEAD later
DK_VMEM = 4  # vector-memory ops of one step's DMA after its rows (the count each step end leaves)


def DS(st, kb, i=None):
    base = 32 * st + 16 * kb
    return rng("v", base, 16) if i is None else f"v{base + i}"


def DDP(kb, i=None):
    return rng("v", 64 + 16 * kb, 16) if i is None else f"v{64 + 16 * kb + i}"


def DDSP(kb, sp, j=None):
    """Packed dS of 16-row half sp, in place over dP[kb] (as QDSP): pack j of elements 8 sp ..
    8 sp + 7 reads 2j, 2j + 1 and writes element j."""
    base = 64 + 16 * kb + 8 * sp
    return rng("v", base, 4) if j is None else f"v{base + j}"


def DPP(kb, sp, j=None):
    base = 96 + (kb * 2 + sp) * 4
    return rng("v", base, 4) if j is None else f"v{base + j}"


def DRR(slot, half=None):
    base = 112 + 4 * (slot % 4)
    return rng("v", base, 4) if half is None else rng("v", base + 2 * half, 2)


DVF_SLOTS = 4


def DVF(n):
    return rng("v", 128 + 4 * (n % DVF_SLOTS), 4)


def DTR(slot, half=None):
    base = 144 + 4 * (slot % 4)
    return rng("v", base, 4) if half is None else rng("v", base + 2 * half, 2)


DLSE0 = 160


def DLSE(i):
    """LSE2 of the row of register i (rows (i & 3) + 8 (i >> 2) + 4 hh of the step's tile); the
    8 registers hold the rows of one half sp = i >> 3 at a time."""
    return f"v{DLSE0 + (i & 7)}"


DK_NVGPR = DLSE0 + 8
# dropout (the forward's saved keep words, DkdvGen(dropout=True)):
#   DKM[kb]   the lane's keep column of key block kb (bit (i & 3) + 8 (i >> 2) = register i's row)
#   DTM[kb]   temporary of key block kb: the P packs' masking, then the dS keep factors
#   -delta of row group g4 (rows 8 g4 + 4 hh ..) in V fragment ring slot g4 (the ring is free from
#   the dP MFMA that last reads a slot to the next step's first V fragment read)
DKM = [f"v{DK_NVGPR}", f"v{DK_NVGPR + 1}"]
DTM = [f"v{DK_NVGPR + 2}", f"v{DK_NVGPR + 3}"]
DK_NVGPR_DROP = DK_NVGPR + 4
D_MC = "s99"       # dropout: byte offset of the requested step's keep words from the wave's base


def _lds_hi(buf, imm, base):
    """(base operand, offset) of an LDS read at step-buffer offset imm: buffer 4 through the
    operand's "h" twin (64 KiB up)."""
    return (base[:-1] + "h]", imm - 65536) if imm >= 65536 else (base, imm)


def DDEL(g4, j=None):
    base = 128 + 4 * g4
    return rng("v", base, 4) if j is None else f"v{base + j}"



def DDV(kb, dt):
    return rng("a", (kb * 4 + dt) * 16, 16)


def DDK(kb, dt):
    return rng("a", 128 + (kb * 4 + dt) * 16, 16)


# scalar state of the dK/dV statement
D_G = "s64"        # q-head index in the group
D_IDX = "s65"      # step index within the head
D_CM = "s66"       # first query row of the current tile
# descriptors of the requested step's Q, dO, LSE2 and delta rows; their base words ARE the
# cursors (the requested tile's first byte; stride 0, and a 48-bit address leaves the high
# word's stride bits clear), word 2 the range of the step, word 3 constant
D_QD = "s[68:71]"
D_OD = "s[72:75]"
D_LD = "s[76:79]"
D_DD = "s[80:83]"
D_QP = ("s68", "s69")
D_OP = ("s72", "s73")
D_LP = ("s76", "s77")
D_DP = ("s80", "s81")
D_MD = "s[84:87]"  # dropout: keep-word descriptor (constant through the statement)
D_WL = "s88"       # dropout: LDS base of this wave's keep words in buffer 0
D_NM = "s89"       # requested step's first query row
D_LEFT = "s90"     # total steps - the requested step's index (> 0: it exists)
D_NMT = "s91"      # requested step's tile index within its head
D_M0 = "s92"
D_T = "s93"
D_EX = "s[94:95]"  # exec save of the rows DMA
D_MK = ["s[96:97]", "s[98:99]"]


class DkdvGen:
    """dK / dV: 4 waves x 64 keys (two 32-key blocks kb per wave, one wave per SIMD); per step
    (32 query rows of one q-head) 64 MFMAs: S(i+1)[kb] = Q K'^T (16), dP(i)[kb] = dO V^T (16),
    dV^T[kb] += dO^T P (16), dK^T[kb] += Q^T dS (16, 8 of them in the next step); every Q / dO /
    transposed fragment read from LDS feeds both key blocks.  Same math as the reference's dK/dV
    loop (/root/reference/src/backward/compute_dkdv.py:42-112) and dkdv_kernel."""

    def __init__(self, bf16, causal, dropout=False):
        self.bf16, self.causal, self.dropout = bf16, causal, dropout
        self.L = DkLayout(DK_NBUF_DROP if dropout else DK_NBUF_PLAIN)
        self.nvgpr = DK_NVGPR_DROP if dropout else DK_NVGPR
        self.mop = "v_mfma_f32_32x32x16_bf16" if bf16 else "v_mfma_f32_32x32x16_f16"
        self.cvtop = "v_cvt_pk_bf16_f32" if bf16 else "v_cvt_pk_f16_f32"
        self.e = Emitter()

    # -- pieces ----------------------------------------------------------------------------------
    def row_read(self, buf, dout, ks):
        """Row fragment ks (Q, or dO when dout) of buffer buf into ring slot ks % 4."""
        imm = buf * 16384 + (8192 if dout else 0) + (ks >> 1) * 2048
        base, imm = _lds_hi(buf, imm, "%[qb1]" if ks & 1 else "%[qb0]")
        d = DRR(ks)
        self.e.ds_read(f"ds_read_b128 {d}, {base} offset:{imm}", d)

    def v_frag(self, n):
        """V fragment n = 2 ks + kb (keys 32 kb .. of this wave, k-step ks)."""
        ks, kb = n >> 1, n & 1
        imm = (ks >> 1) * 4096 + 32 * kb * 64
        base = "%[vb1]" if ks & 1 else "%[vb0]"
        d = DVF(n)
        self.e.ds_read(f"ds_read_b128 {d}, {base} offset:{imm}", d)

    def tr_read(self, buf, dout, f, half, dst):
        """Half `half` of transposed fragment f (sp = f >> 2, dt = f & 3) of dO^T (dout) or Q^T of
        buffer buf into the 2 registers dst."""
        sp, dt = f >> 2, f & 3
        imm = buf * 16384 + (8192 if dout else 0) + dt * 2048 + 16 * sp * 64
        base, imm = _lds_hi(buf, imm, "%[tb]" if half else "%[ta]")
        self.e.ds_read(f"ds_read_b64_tr_b16 {dst}, {base} offset:{imm}", dst)

    def init_read(self, buf, what, kb, g4):
        """LSE2 (what 0; g4 in the half's pair) rows into the LSE registers, -delta (what 1) into
        dP[kb] (the dP chain's initial accumulator): register group g4."""
        imm = buf * 256 + what * 128 + 32 * g4
        d = rng("v", DLSE0 + 4 * (g4 & 1), 4) if what == 0 else rng("v", 64 + 16 * kb + 4 * g4, 4)
        self.e.ds_read(f"ds_read_b128 {d}, %[lb] offset:{imm}", d)

    def descriptors(self, part=None):
        """The ranges of the requested step's descriptors (range 0 when none): part 0 the rows
        (D_T) and the LSE2 / delta bytes below Lq, 1 the Q and dO bytes."""
        e = self.e
        if part in (None, 0):
            e.salu(f"s_sub_u32 {D_T}, %[lq], {D_NM}")
            e.salu(f"s_cmp_gt_i32 {D_LEFT}, 0")
            e.salu(f"s_cselect_b32 {D_T}, {D_T}, 0")
            e.salu(f"s_min_u32 s78, {D_T}, 32")
            e.salu("s_lshl_b32 s78, s78, 2")
            if self.dropout:  # lsoff = sb + w0 + 256 w + 4 lane (w = 0 here): the range
                # starts there (lbs = sb + rows)
                e.salu("s_add_u32 s78, s78, %[lbs]")
                e.salu(f"s_add_u32 s78, s78, {self.L.w0 - self.L.rows}")
            e.salu("s_mov_b32 s82, s78")
        if part in (None, 1):
            orb = "%[qrb]" if self.dropout else "%[orb]"  # (dropout: one row stride)
            e.salu(f"s_mul_i32 s70, {D_T}, %[qrb]")
            e.salu(f"s_mul_i32 s74, {D_T}, {orb}")

    def advance_cursors(self, tag):
        """Cursors to the step after the requested one: one tile down, or the next head's last
        tile; one request fewer left."""
        e = self.e
        e.salu(f"s_sub_i32 {D_LEFT}, {D_LEFT}, 1")
        e.salu(f"s_add_u32 {D_NMT}, {D_NMT}, 1")
        e.salu(f"s_cmp_eq_u32 {D_NMT}, %[nmt]")
        e.raw(f"s_cbranch_scc1 .Lhp%=_{tag}_wrap")
        e.salu(f"s_sub_u32 {D_NM}, {D_NM}, 32")
        # one tile = 32 rows (D_T: free once the step's descriptors are built)
        e.salu(f"s_lshl_b32 {D_T}, %[qrb], 5")
        e.salu(f"s_sub_u32 {D_QP[0]}, {D_QP[0]}, {D_T}")
        e.salu(f"s_subb_u32 {D_QP[1]}, {D_QP[1]}, 0")
        e.salu(f"s_lshl_b32 {D_T}, {'%[qrb]' if self.dropout else '%[orb]'}, 5")
        e.salu(f"s_sub_u32 {D_OP[0]}, {D_OP[0]}, {D_T}")
        e.salu(f"s_subb_u32 {D_OP[1]}, {D_OP[1]}, 0")
        for p0, p1 in (D_LP, D_DP):
            e.salu(f"s_sub_u32 {p0}, {p0}, 128")
            e.salu(f"s_subb_u32 {p1}, {p1}, 0")
        if self.dropout:
            e.salu(f"s_sub_u32 {D_MC}, {D_MC}, %[mstep]")
        e.raw(f"s_branch .Lhp%=_{tag}_adv")
        e.label(f".Lhp%=_{tag}_wrap")
        e.salu(f"s_mov_b32 {D_NMT}, 0")
        e.salu(f"s_mov_b32 {D_NM}, %[mlast]")
        e.salu(f"s_add_u32 {D_QP[0]}, {D_QP[0]}, %[qwrap]")
        e.salu(f"s_addc_u32 {D_QP[1]}, {D_QP[1]}, 0")
        e.salu(f"s_add_u32 {D_OP[0]}, {D_OP[0]}, %[owrap]")
        e.salu(f"s_addc_u32 {D_OP[1]}, {D_OP[1]}, 0")
        for p0, p1 in (D_LP, D_DP):
            e.salu(f"s_add_u32 {p0}, {p0}, %[lwrap]")
            e.salu(f"s_addc_u32 {p1}, {p1}, 0")
        if self.dropout:
            e.salu(f"s_add_u32 {D_MC}, {D_MC}, %[mwrap]")
        e.label(f".Lhp%=_{tag}_adv")

    def dma_items(self, nb, tag):
        """One step's request into buffer nb as (cost, emit) items: the descriptors, wave 0's
        LSE2 / delta rows, the Q, dO pieces (m0 set one item ahead), then the cursors.  Every
        wave's last DK_VMEM vector-memory ops are its pieces."""
        pieces = [("q", 0), ("q", 1), ("o", 0), ("o", 1)]

        def m0_of(w_, it):
            return nb * 16384 + (8192 if w_ == "o" else 0) + it * 4096

        # (issue costs of scalar instructions are taken as 2 cycles each)
        out = [(12, lambda: self.descriptors(0)), (4, lambda: self.descriptors(1))]

        def rows(tag=tag):
            e = self.e
            e.raw("s_cmp_eq_u32 %[w0], 0")
            e.raw(f"s_cbranch_scc0 .Lhp%=_{tag}_nl")
            # one row per lane (lanes 0-31): the range ends exactly at the last row below Lq
            e.salu(f"s_mov_b64 {D_EX}, exec")
            e.salu("s_mov_b32 exec_lo, -1")
            e.salu("s_mov_b32 exec_hi, 0")
            e.salu(f"s_add_u32 m0, %[lbs], {nb * 256}", m0=True)
            e.dma(f"buffer_load_dword %[lsoff], {D_LD}, 0 offen lds")
            e.salu(f"s_add_u32 m0, %[lbs], {nb * 256 + 128}", m0=True)
            e.dma(f"buffer_load_dword %[lsoff], {D_DD}, 0 offen lds")
            e.salu(f"s_mov_b64 exec, {D_EX}")
            e.label(f".Lhp%=_{tag}_nl")
        out.append((16, rows))
        if self.dropout:
            def words(nb=nb):
                # this wave's 64 keep words of the requested step (rows of the tile, key tiles
                # kt0, kt0 + 1: one word per lane)
                e = self.e
                e.salu(f"s_add_u32 m0, {D_WL}, {nb * 1024}", m0=True)
                e.dma(f"buffer_load_dword %[lsoff], {D_MD}, {D_MC} offen lds")
            out.append((8, words))
        for n, (w_, it) in enumerate(pieces):
            def f(n=n, w_=w_, it=it):
                if n == 0:
                    self.e.salu(f"s_add_u32 m0, %[mlds], {m0_of(w_, it)}", m0=True)
                off = f"%[{'q' if w_ == 'q' or self.dropout else 'o'}off{it}]"
                self.e.dma(f"buffer_load_dwordx4 {off}, {D_QD if w_ == 'q' else D_OD}, 0 offen lds")
                if n + 1 < len(pieces):
                    self.e.salu(f"s_add_u32 m0, %[mlds], {m0_of(*pieces[n + 1])}", m0=True)
            out.append((16, f))
        out.append((20, lambda: self.advance_cursors(tag)))
        return out

    def keep_items(self, par, g):
        """Dropout: this step's keep words (buffer par: lane (r32, hh) holds row r32 of key tile
        hh) -> DKM[kb] = the lane's column of key block kb (bit r = row r; the hh = 1 lanes shifted
        by 4 so bit (i & 3) + 8 (i >> 2) is register i's row), as dkdv_kernel's transpose32_lanes:
        five ds_swizzle xor stages within each 32-lane half (the lane-dependent halves of a stage
        under exec masks), then one v_permlane32_swap hands each half the other key block."""
        e = self.e
        m0_, m1_ = DKM
        g.add("tp", 4, -1, 0, lambda: e.ds_read(f"ds_read_b32 {m0_}, %[lsoff] offset:{1024 * par}", m0_),
              lds=1)
        masks = {16: 0x0000FFFF, 8: 0x00FF00FF, 4: 0x0F0F0F0F, 2: 0x33333333, 1: 0x55555555}
        for n, J in enumerate((16, 8, 4, 2, 1)):
            def sw(J=J):
                e._need_lgkm({m0_})
                e.ds_read(f"ds_swizzle_b32 {m1_}, {m0_} offset:{0x1F | (J << 10)}", m1_)

            def stage(J=J):
                e._need_lgkm({m1_})
                e.salu(f"s_mov_b32 s98, {hex(masks[J])}")
                # lanes with lane bit J clear: x = (x & m) | (y << J & ~m)
                e.salu("s_mov_b32 exec_lo, s98")
                e.salu("s_mov_b32 exec_hi, s98")
                e.valu(f"v_lshlrev_b32 {m1_}, {J}, {m1_}", m1_, [m1_])
                e.valu(f"v_bfi_b32 {m0_}, s98, {m0_}, {m1_}", m0_, [m0_, m1_])
                # lanes with it set: x = (y >> J & m) | (x & ~m)
                e.salu("s_not_b32 exec_lo, s98")
                e.salu("s_not_b32 exec_hi, s98")
                e.valu(f"v_lshrrev_b32 {m1_}, {J}, {m1_}", m1_, [m1_])
                e.valu(f"v_bfi_b32 {m0_}, s98, {m1_}, {m0_}", m0_, [m0_, m1_])
                e.salu("s_mov_b64 exec, -1")
            g.add("tp", 4, 2 * n, 2 * n + 2, sw, lds=1)
            g.add("tp", 20, 2 * n + 1, 2 * n + 3, stage)

        def fin():
            e.valu(f"v_mov_b32 {m1_}, {m0_}", m1_, [m0_])
            e.valu(f"v_permlane32_swap_b32 {m0_}, {m1_}", [m0_, m1_], [m0_, m1_], kind="perm")
            e.salu("s_mov_b32 exec_lo, 0")
            e.valu(f"v_lshrrev_b32 {m0_}, 4, {m0_}", m0_, [m0_])
            e.valu(f"v_lshrrev_b32 {m1_}, 4, {m1_}", m1_, [m1_])
            e.salu("s_mov_b64 exec, -1")
        g.add("tp", 20, 10, 12, fin)

    def pack_keep(self, kb, sp, j):
        """Dropout: zero the halves of the P pack PP[kb][sp][j] whose element the forward dropped
        (dV is scaled by 1 / (1 - p) once, in the epilogue)."""
        e = self.e
        pp, t = DPP(kb, sp, j), DTM[kb]
        for h, a in enumerate((8 * sp + 2 * j, 8 * sp + 2 * j + 1)):
            o = (a & 3) + 8 * (a >> 2)
            e.valu(f"v_bfe_i32 {t}, {DKM[kb]}, {o}, 1", t, [DKM[kb]])
            # (SDWA writes the low 16 bits of the result to the selected word: select the same word
            # of both sources; bench_micro/sdwa_test.hip pins this on the hardware)
            e.valu(f"v_and_b32_sdwa {pp}, {t}, {pp} dst_sel:WORD_{h} dst_unused:UNUSED_PRESERVE src0_sel:WORD_{h} "
                   f"src1_sel:WORD_{h}", pp, [t, pp])

    def mask_elem(self, st, kb, i):
        """Causal: P = row >= key - diag ? P : 0 for register i of key block kb, as
        CM + o - kd[kb] >= lr (o = the row offset of the register, kd[kb] = the block's first key
        - diag, lr = r32 - 4 hh).  No other mask: query rows past Lq read zero Q, dO, LSE2 and
        delta (the descriptors' ranges), so P = 1 there multiplies zeros; keys past Lk only reach
        their own dK / dV rows, which are not stored."""
        if not self.causal:
            return
        e = self.e
        o = (i & 3) + 8 * (i >> 2)
        r = DS(st, kb, i)
        # s96 + kb = CM - kd[kb] (mask_bases, at the step start)
        e.salu(f"s_add_u32 s98, s{96 + kb}, {o}")
        e.valu("v_cmp_ge_i32_e32 vcc, s98, %[lr]", None, [])
        e.valu(f"v_cndmask_b32_e32 {r}, 0, {r}, vcc", r, [r])

    def mask_bases(self):
        """s96 + kb = CM - kd[kb] of a masked step (kd[1] = kd[0] + 32)."""
        e = self.e
        e.salu(f"s_sub_u32 s96, {D_CM}, %[kd0]")
        e.salu("s_sub_u32 s97, s96, 32")

    def cvt(self, d, a, b):
        self.e.valu(f"{self.cvtop} {d}, {a}, {b}", d, [a, b])

    # -- MFMAs -----------------------------------------------------------------------------------
    def mf_dk_tail(self, g):
        """Straddled MFMA g (0-7): dK^T[kb][dt] += Q^T(rows 16-31, dt) dS[kb] rows 16-31 of the
        previous step (Q^T fragment in row-ring slot dt)."""
        dt, kb = g >> 1, g & 1
        self.e.mfma(self.mop, DDK(kb, dt), DRR(dt), DDSP(kb, 1), DDK(kb, dt))

    def mf_s(self, st, g):
        """S(next)[kb] (set st) += Q(ks) K[kb](ks), g = 2 ks + kb."""
        ks, kb = g >> 1, g & 1
        self.e.mfma(self.mop, DS(st, kb), DRR(ks), f"%[k{kb * 8 + ks}]", "0" if ks == 0 else DS(st, kb))

    # -- one step --------------------------------------------------------------------------------
    def step(self, ph, cls, tag):
        """Step i with i mod (the layout's phase count) = ph, class A (live, unmasked), B (live, masked) or D (no key
        of the wave visible: only the straddled MFMAs, S(i+1) and the request)."""
        e = self.e
        L = self.L
        par = ph % L.nbuf      # buffer of step i
        st = ph & 1            # S / P set of step i; S(i+1) goes to 1 - st
        nxt = (ph + 1) % L.nbuf
        # half barriers: the even step of a pair requests steps i + 3 and i + 4 (the buffers of
        # steps i - 2 and i - 1, both read before the barrier after step i - 1), the odd one none,
        # so every request has a whole step to land before the barrier; without half barriers
        # (dropout) one request per step
        if L.halfbar:
            reqs = [] if ph & 1 else [((par + DK_AHEAD) % L.nbuf, tag), ((par + DK_AHEAD + 1) % L.nbuf, tag + "x")]
        else:
            reqs = [((par + DK_AHEAD) % L.nbuf, tag)]
        live = cls in ("A", "B")
        masked = cls == "B"
        if masked and self.causal:
            self.mask_bases()
        # the MFMAs of the step (indices of `mfma` below): a live step all 64; a dead step (no key of
        # the wave visible) only what a neighbour needs (round 6; round 5 ran the straddled eight and
        # S(i+1) in every dead step: 3.9 % more MFMAs than the algorithm per launch) --
        #   D  (the head's first dead step, also its last): the straddled MFMAs that finish the last
        #      live step's dK, and S(i+1) for the next head's first step;
        #   Ds (first dead step, more follow): the straddled MFMAs only;
        #   E  (neither first nor last): none;
        #   F  (the head's last dead step after others): S(i+1) only
        mf = list(range(64)) if live else {"D": list(range(24)), "Ds": list(range(8)), "E": [],
                                           "F": list(range(8, 24))}[cls]
        pos = {m: n for n, m in enumerate(mf)}
        last = max(len(mf) - 1, -1)
        g = GapScheduler(len(mf), lds_cap=3)
        # Q(i+1) row fragments ks -> ring slot ks % 4 (after the slot's previous occupant's last
        # MFMA: the straddled MFMAs 2 dt + kb, then S MFMAs 8 + 2 ks + kb); none without S(i+1)
        if 8 in pos:
            for ks in range(8):
                if 0 in pos:
                    rel, dl = 2 * ks + 1, 2 * ks + 5
                else:
                    # F: no straddled MFMA reads the slots (the step before was Ds or E), so
                    # fragments 0-3 go at once; fragment ks >= 4 reuses slot ks % 4 only after
                    # both S MFMAs of fragment ks - 4 have read it
                    rel = -1 if ks < 4 else pos[8 + 2 * (ks - 4) + 1] + 1
                    dl = max(rel, pos[8 + 2 * ks] - 3)
                g.add("row", 4, rel, dl, lambda ks=ks: self.row_read(nxt, False, ks), lds=2)
        items = [it for nb, t in reqs for it in self.dma_items(nb, t)]
        for n, (c, f) in enumerate(items):
            if L.halfbar:
                dl = min(20 + 3 * n, 62) if live else min(6 + n, last)
            else:
                dl = 42 + 3 * n if live else min(14 + 3 * n, last)
            g.add("dma", c, 2 if live else 0, dl, f)
        if live:
            # dO(i) row fragments ks (slot ks % 4, after the S MFMAs 2 ks + 17), dP at 24 + 2 ks
            for ks in range(8):
                rel = 2 * ks + 17
                g.add("row", 4, rel, rel + 4, lambda ks=ks: self.row_read(par, True, ks), lds=2)
            # Q^T(i) fragments of rows 16-31 (f = 4 + dt) into row-ring slots dt, after the dP
            # MFMAs that read the slot's dO fragment (2 dt + 33): the next step's first MFMAs
            for dt in range(4):
                for h in range(2):
                    g.add("row", 4, 2 * dt + 33, 58,
                          lambda dt=dt, h=h: self.tr_read(par, False, 4 + dt, h, DRR(dt, h)), lds=1)
            # V fragments n (slot n % 4): dP MFMA 24 + n
            for n in range(16):
                rel = 8 if n < DVF_SLOTS else 24 + n - DVF_SLOTS
                g.add("vf", 4, rel, max(rel, 21 + n), lambda n=n: self.v_frag(n), lds=2)
            # dO^T fragments f (slot f % 4): dV MFMAs 40 + 2 f + kb; then Q^T rows 0-15 (slot f)
            for f in range(8):
                rel = 0 if f < 4 else 2 * f + 33
                for h in range(2):
                    g.add("tr", 4, rel, 2 * f + 37, lambda f=f, h=h: self.tr_read(par, True, f, h, DTR(f, h)), lds=1)
            for f in range(4):
                for h in range(2):
                    g.add("tr", 4, 2 * f + 49, 2 * f + 53, lambda f=f, h=h: self.tr_read(par, False, f, h, DTR(f, h)),
                          lds=1)
            # -delta rows into dP[1] only (register groups g4; g4 = 2 holds the packed dS of rows
            # 16-31 that the straddled MFMAs 2 dt + 1 read: after them); the first dP MFMA of block
            # 0 takes dP[1] as its C (before block 1's chain overwrites it), so both chains start
            # from the one copy of the rows
            if not self.dropout:
                for g4 in range(4):
                    g.add("init1", 4, 8 if g4 == 2 else 0, 20, lambda g4=g4: self.init_read(par, 1, 1, g4), lds=2)
            else:
                # -delta rows (group g4) for dS = P (dP kp - delta), into V ring slot g4 once the
                # dP MFMA 36 + g4 has read it
                for g4 in range(4):
                    d = DDEL(g4)
                    rel, dl = 36 + g4, 41 + g4
                    g.add("dl", 4, rel, dl, lambda g4=g4, d=d: self.e.ds_read(
                        f"ds_read_b128 {d}, %[lb] offset:{par * 256 + 128 + 32 * g4}", d), lds=2)
                self.keep_items(par, g)
            # LSE2 of this step's half sp = 1 once every sp = 0 exponent argument is done; half
            # sp = 0 of the NEXT step once every sp = 1 one is (its rows landed a step ago), so no
            # exponential waits for an LDS read at a step start (round 5: that wait cost ~8 %)
            for g4 in (2, 3):
                g.add("lse", 4, 14, 18, lambda g4=g4: self.init_read(par, 0, 0, g4), lds=2)
            for g4 in (0, 1):
                g.add("lse", 4, 40, 58, lambda g4=g4: self.init_read(nxt, 0, 0, g4), lds=2)
            # exponentials of P(i) (set st): P = exp2(s scale log2 e - LSE2), the scale in fp32;
            # mask; packs PP[kb][sp] (dV MFMAs 40 + 8 sp + 2 dt + kb)
            for sp in range(2):
                r0, r1 = (0, 18) if sp == 0 else (21, 44)
                for kb in range(2):
                    els = list(range(8 * sp, 8 * sp + 8))
                    for k, i in enumerate(els):
                        r = DS(st, kb, i)
                        dl = r0 + ((r1 - r0 - 6) * (k + 1)) // 8
                        g.add(f"exp{kb}", 4, r0, dl,
                              lambda r=r, i=i: e.valu(f"v_fma_f32 {r}, {r}, %[sc], -{DLSE(i)}", r, [r, DLSE(i)]))
                        g.add(f"exp{kb}", 8, r0, dl + 1, lambda r=r: e.valu(f"v_exp_f32 {r}, {r}", r, [r], kind="trans"))
                        if masked and self.causal:
                            g.add(f"exp{kb}", 12, r0, dl + 2, lambda kb=kb, i=i: self.mask_elem(st, kb, i))
                    for j in range(4):
                        g.add(f"exp{kb}", 4, r0, (38 if sp == 0 else (42 if self.dropout else 46)),
                              lambda kb=kb, sp=sp, j=j: self.cvt(DPP(kb, sp, j), DS(st, kb, 8 * sp + 2 * j),
                                                               DS(st, kb, 8 * sp + 2 * j + 1)))
                        if self.dropout:  # (the keep columns are ready after the transposition;
                            # DTM[kb] is the dS side's from MFMA 43 on)
                            g.add(f"exp{kb}", 16, max(r0, 13), (38 if sp == 0 else 42),
                                  lambda kb=kb, sp=sp, j=j: self.pack_keep(kb, sp, j))
            # dS(i) = P dP' after the dP chains (last MFMA 39; 4 MFMAs for the result), packs in place; DSP[kb][0] for the
            # MFMAs 56 + 2 dt + kb, DSP[kb][1] for the next step's first MFMAs
            for kb in range(2):
                if self.dropout:
                    # dS = P (dP kp - delta), kp = keep ? 1 / (1 - p) : 0 (bit for bit dkdv_kernel's
                    # pr * (dp * kp + d4)); by row group g4, packs j of the group right after it
                    for g4 in range(4):
                        sp, dl = g4 >> 1, (50, 53, 58, 61)[g4]
                        for i in range(4 * g4, 4 * g4 + 4):
                            a_, b_, t_, d_ = DS(st, kb, i), DDP(kb, i), DTM[kb], DDEL(g4, i & 3)
                            o = (i & 3) + 8 * (i >> 2)

                            def dsd(a_=a_, b_=b_, t_=t_, d_=d_, o=o, kb=kb):
                                e.valu(f"v_bfe_i32 {t_}, {DKM[kb]}, {o}, 1", t_, [DKM[kb]])
                                e.valu(f"v_and_b32 {t_}, %[dscb], {t_}", t_, [t_])
                                e.valu(f"v_fma_f32 {b_}, {b_}, {t_}, {d_}", b_, [b_, t_, d_])
                            g.add(f"ds{kb}", 12, 43, dl, dsd)
                            g.add(f"ds{kb}", 4, 43, dl,
                                  lambda a_=a_, b_=b_: e.valu(f"v_mul_f32 {b_}, {a_}, {b_}", b_, [a_, b_]))
                        for j in (2 * (g4 & 1), 2 * (g4 & 1) + 1):
                            g.add(f"ds{kb}", 4, 43, dl + 1,
                                  lambda kb=kb, sp=sp, j=j: self.cvt(DDSP(kb, sp, j), DDP(kb, 8 * sp + 2 * j),
                                                                   DDP(kb, 8 * sp + 2 * j + 1)))
                    continue
                for sp in range(2):
                    dl = 52 if sp == 0 else 61
                    for i in range(8 * sp, 8 * sp + 8):
                        a_, b_ = DS(st, kb, i), DDP(kb, i)
                        g.add(f"ds{kb}", 4, 43, dl, lambda a_=a_, b_=b_: e.valu(f"v_mul_f32 {b_}, {a_}, {b_}", b_, [a_, b_]))
                    for j in range(4):
                        g.add(f"ds{kb}", 4, 43, dl + 1,
                              lambda kb=kb, sp=sp, j=j: self.cvt(DDSP(kb, sp, j), DDP(kb, 8 * sp + 2 * j), DDP(kb, 8 * sp + 2 * j + 1)))
        else:
            # no dS of this step: the next step's straddled MFMAs add zeros (after this step's
            # straddled MFMAs, which read the packs)
            for kb in range(2):
                for j in range(4):
                    r = DDSP(kb, 1, j)
                    g.add("zero", 4, (7 + kb) if 0 in pos else -1, min(20, last), lambda r=r: e.valu(f"v_mov_b32 {r}, 0", r))
            for g4 in (0, 1):  # the next step's LSE2 of half sp = 0
                g.add("lse", 4, -1, min(20, last), lambda g4=g4: self.init_read(nxt, 0, 0, g4), lds=2)

        if "dk_novalu" in ABL:
            g.items = [it for it in g.items if not it["stream"].startswith(("exp", "ds"))]
        if "dk_nodma" in ABL:
            g.items = [it for it in g.items if it["stream"] != "dma"]
        if "dk_nolds" in ABL:
            g.items = [it for it in g.items if it["stream"] not in ("row", "vf", "tr", "init1", "lse")]
        if "dk_nolgkm" in ABL:
            e.ds = []
            e._need_lgkm = lambda regs: None

        def mfma(n):
            m = mf[n]
            if m < 8:
                self.mf_dk_tail(m)
            elif m < 24:
                self.mf_s(1 - st, m - 8)
            elif m < 40:  # dP[kb] += dO(ks) V[kb](ks), both chains seeded from dP[1]'s -delta rows
                ks, kb = (m - 24) >> 1, m & 1
                c = ("0" if self.dropout else DDP(1)) if ks == 0 else DDP(kb)
                e.mfma(self.mop, DDP(kb), DRR(ks), DVF(2 * ks + kb), c)
            elif m < 56:  # dV^T[kb][dt] += dO^T(sp, dt) P[kb](sp)
                f, kb = (m - 40) >> 1, m & 1
                e.mfma(self.mop, DDV(kb, f & 3), DTR(f), DPP(kb, f >> 2), DDV(kb, f & 3))
            else:  # dK^T[kb][dt] += Q^T(rows 0-15, dt) dS[kb](rows 0-15)
                f, kb = (m - 56) >> 1, m & 1
                e.mfma(self.mop, DDK(kb, f), DTR(f), DDSP(kb, 0), DDK(kb, f))

        g.run(mfma, pre_budget=24)
        if "dk_nolgkm" in ABL:
            e._need_lgkm = Emitter._need_lgkm.__get__(e)
        e.salu(f"s_sub_u32 {D_CM}, {D_CM}, 32")
        e.drain_lds()
        if L.halfbar:
            if ph & 1:
                # every request so far (up to step i + 3) has landed
                e.raw("s_waitcnt vmcnt(0)")
                e.raw("s_barrier")
            else:
                return  # (no reset: the odd step starts from this end state, DkdvGen.build)
        else:
            if "dk_novm" not in ABL:
                # the next step's tiles (requested two steps ago) have landed; this step's stay in
                # flight
                e.raw(f"s_waitcnt vmcnt({DK_VMEM})")
            if "dk_nobar" not in ABL:
                e.raw("s_barrier")
        e.reset()

    def build(self):
        e = self.e
        e.raw("s_nop 7")
        e.raw("s_nop 7")
        e.salu(f"s_mov_b32 {D_M0}, m0")
        for r in range(256):
            e.valu(f"v_accvgpr_write_b32 a{r}, 0", f"a{r}", kind="accw")
        # the first step's straddled MFMAs add zeros
        for kb in range(2):
            for j in range(4):
                e.valu(f"v_mov_b32 {DDSP(kb, 1, j)}, 0", DDSP(kb, 1, j))
        # cursors: step 0's tiles were requested before the statement (and waited for by the
        # compiler's wait for the K fragments); steps 1 and 2 here, then the loop requests step
        # i + 3 during step i
        e.salu(f"s_mov_b32 {D_QP[0]}, %[qlo]")
        e.salu(f"s_mov_b32 {D_QP[1]}, %[qhi]")
        e.salu(f"s_mov_b32 {D_OP[0]}, %[olo]")
        e.salu(f"s_mov_b32 {D_OP[1]}, %[ohi]")
        for (p0, p1), b in ((D_LP, "lse"), (D_DP, "dl")):
            e.salu(f"s_add_u32 {p0}, %[{b}lo], %[lc0]")
            e.salu(f"s_addc_u32 {p1}, %[{b}hi], 0")
        for d in (71, 75, 79, 83):
            e.salu(f"s_mov_b32 s{d}, 0x20000")
        if self.dropout:
            e.salu("s_mov_b32 s84, %[mlo]")
            e.salu("s_mov_b32 s85, %[mhi]")
            e.salu("s_mov_b32 s86, %[mrange]")  # the mask's bytes from the base: reads past it give 0
            e.salu("s_mov_b32 s87, 0x20000")
            # sb + w0 + 256 w (lbs = sb + rows)
            e.salu(f"s_lshl_b32 {D_WL}, %[w0], 8")
            e.salu(f"s_add_u32 {D_WL}, {D_WL}, %[lbs]")
            e.salu(f"s_add_u32 {D_WL}, {D_WL}, {self.L.w0 - self.L.rows}")
        e.salu(f"s_mov_b32 {D_NM}, %[mlast]")
        e.salu(f"s_mov_b32 {D_NMT}, 0")
        e.salu(f"s_mul_i32 {D_LEFT}, %[ng], %[nmt]")  # the block's steps
        if self.dropout:  # step 0's keep words: mstep (nmt - 1)
            e.salu(f"s_sub_u32 {D_MC}, %[nmt], 1")
            e.salu(f"s_mul_i32 {D_MC}, {D_MC}, %[mstep]")
        self.advance_cursors("init")  # -> step 1 (D_LEFT = total - 1)
        # this block's V rows, step-0 tiles and K fragments (requested before the statement, during
        # the previous block's epilogue) have landed; every wave is past that epilogue, whose
        # staging images sit in step buffers 2-3
        e.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e.raw("s_barrier")
        e.reset()
        for nb in (1, 2):
            for _, f in self.dma_items(nb, f"pro{nb}"):
                f()
        e.salu(f"s_mov_b32 {D_G}, 0")
        # no step at all (ng nmt = 0; D_G = 0 here)
        e.raw(f"s_cmp_eq_u32 {D_G}, %[ng]")
        e.raw("s_cbranch_scc1 .Lhp%=_end")
        e.raw("s_cmp_eq_u32 %[nmt], 0")
        e.raw("s_cbranch_scc1 .Lhp%=_end")
        # S(0) into set 0 from buffer 0
        for ks in range(3):
            self.row_read(0, False, ks)
        for m in range(16):
            ks = m >> 1
            if m & 1 and ks + 3 < 8:
                self.row_read(0, False, ks + 3)
            self.mf_s(0, m)
        for g4 in (0, 1):  # step 0's LSE2 of half sp = 0 (each step loads the next one's)
            self.init_read(0, 0, 0, g4)
        e.drain_lds()
        e.drain_mfma()
        # step 1's tiles (half barriers: step 2's too; steps 0 and 1 run before the next barrier)
        e.raw(f"s_waitcnt vmcnt({0 if self.L.halfbar else DK_VMEM})")
        e.raw("s_barrier")
        e.reset()
        e.salu(f"s_mov_b32 {D_IDX}, 0")
        e.salu(f"s_mov_b32 {D_CM}, %[mlast]")
        # one entry per step phase ph: the class of step IDX ([0, c0) B, [c0, c01) A, [c01, c012)
        # B, then D) -> the body (class, ph); each body continues at the entry of phase ph + 1 (the
        # phase is static: no dispatch on it)
        for ph in range(self.L.ph):
            e.raw(".balignl 64, 0xbf800000", 0)
            e.label(f".Lhp%=_step{ph}")
            e.raw(f"s_cmp_lt_u32 {D_IDX}, %[c0]")
            e.raw(f"s_cbranch_scc1 .Lhp%=_B{ph}")
            e.raw(f"s_cmp_lt_u32 {D_IDX}, %[c01]")
            e.raw(f"s_cbranch_scc1 .Lhp%=_A{ph}")
            e.raw(f"s_cmp_lt_u32 {D_IDX}, %[c012]")
            e.raw(f"s_cbranch_scc1 .Lhp%=_B{ph}")
            # dead steps: D / Ds at IDX == c012 (with / without more after it), E between, F last
            e.salu(f"s_add_u32 {D_T}, {D_IDX}, 1")
            e.raw(f"s_cmp_eq_u32 {D_IDX}, %[c012]")
            e.raw(f"s_cbranch_scc0 .Lhp%=_nd{ph}")
            e.raw(f"s_cmp_lt_u32 {D_T}, %[nmt]")
            e.raw(f"s_cbranch_scc1 .Lhp%=_Ds{ph}")
            e.raw(f"s_branch .Lhp%=_D{ph}")
            e.label(f".Lhp%=_nd{ph}")
            e.raw(f"s_cmp_lt_u32 {D_T}, %[nmt]")
            e.raw(f"s_cbranch_scc1 .Lhp%=_E{ph}")
            e.raw(f"s_branch .Lhp%=_F{ph}")
        snaps = []
        for ph in range(self.L.ph):
            ends = []
            for cls in ("A", "B", "D", "Ds", "E", "F"):
                nph = (ph + 1) % self.L.ph
                e.label(f".Lhp%=_{cls}{ph}")
                # half barriers: an odd step follows any of the previous phase's bodies with no
                # barrier between (their merged end states); an even one follows a barrier
                if self.L.halfbar and ph & 1:
                    e.restore(snaps)
                else:
                    e.reset()
                self.step(ph, cls, f"{cls.lower()}{ph}")
                if self.L.halfbar and not ph & 1:
                    if cls not in ("A", "B"):  # (rare: a head's dead steps)
                        e.close_windows()
                    ends.append(e.snapshot())
                # next step: within the head, else the next head's first (IDX 0, CM = mlast)
                e.salu(f"s_add_u32 {D_IDX}, {D_IDX}, 1")
                e.raw(f"s_cmp_lt_u32 {D_IDX}, %[nmt]")
                e.raw(f"s_cbranch_scc1 .Lhp%=_step{nph}")
                e.salu(f"s_add_u32 {D_G}, {D_G}, 1")
                e.salu(f"s_mov_b32 {D_IDX}, 0")
                e.salu(f"s_mov_b32 {D_CM}, %[mlast]")
                e.raw(f"s_cmp_lt_u32 {D_G}, %[ng]")
                e.raw(f"s_cbranch_scc1 .Lhp%=_step{nph}")
                e.raw("s_branch .Lhp%=_last")
            snaps = ends
        e.label(".Lhp%=_last")
        # (after any body: every window closed)
        e.ds = []
        e._pad(max(Emitter.MFMA_RESULT, Emitter.MFMA_C_WAR))
        e.reset()
        # the last step's straddled MFMAs
        for m in range(8):
            self.mf_dk_tail(m)
        e.label(".Lhp%=_end")
        # every wave's (range-0) requests of the last steps have landed before any wave stages
        # its epilogue in the step buffers
        e.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e.raw("s_barrier")
        e.salu(f"s_mov_b32 m0, {D_M0}")
        e.raw("s_nop 15")
        e.raw("s_nop 15")
        return e.out


def gen_dkdv_function(bf16, causal, dropout=False):
    g = DkdvGen(bf16, causal, dropout)
    lines = g.build()
    name = f"dkdv_hp_main_{'bf16' if bf16 else 'f16'}_{'causal' if causal else 'full'}{'_drop' if dropout else ''}"
    clob = [f'"v{i}"' for i in range(g.nvgpr)] + [f'"a{i}"' for i in range(256)] + \
           [f'"s{i}"' for i in _sgprs_used(lines)] + ['"vcc"', '"scc"', '"memory"']
    kops = ", ".join(f'[k{i}] "v"(kf[{i}])' for i in range(16))
    sops = ["ng", "nmt", "c0", "c01", "c012", "mlast", "lq", "qrb"] + ([] if dropout else ["orb"]) + ["qwrap",
            "owrap", "lwrap", "lc0", "qlo", "qhi", "olo", "ohi", "lselo", "lsehi", "dllo", "dlhi", "mlds", "lbs", "w0",
            "sc"] + (["kd0"] if causal else []) + (["mlo", "mhi", "mrange", "mstep", "mwrap"] if dropout else [])
    vops = ["qb0", "qb1", "vb0", "vb1", "ta", "tb"] + (["qb0h", "qb1h", "tah", "tbh"] if g.L.nbuf > 4 else []) + ["lb", "qoff0", "qoff1"] + ([] if dropout else ["ooff0", "ooff1"]) + \
        ["lsoff"] + (["lr"] if causal else []) + (["dscb"] if dropout else [])
    src = f"""// hand-placed dK/dV statement ({'bf16' if bf16 else 'fp16'}, {'causal' if causal else 'non-causal'}): {len(lines)} lines, {g.e.n_mfma} MFMAs
FA2_DEV void {name}(const u32x4 (&kf)[16], const DkdvHpArgs& a) {{
  asm volatile(
{_asm_body(lines)}
      :
      : {kops},
        {", ".join(f'[{n}] "v"(a.{n})' for n in vops)},
        {", ".join(f'[{n}] "s"(a.{n})' for n in sops)}
      : {", ".join(clob)});
}}
"""
    return src


def gen_read_dkdv():
    parts = ["// dV^T a[0:127], dK^T a[128:255] of key block KB -> registers (after the statement's final",
             "// drain); one key block at a time keeps the epilogue within the register file; tok: a",
             "// value of the next block's requests (kept ahead of these reads by the data dependence)",
             "template <int KB>",
             "FA2_DEV void dkdv_hp_read(f32x16 (&dv)[4], f32x16 (&dk)[4], uint32_t tok);"]
    for kb in range(2):
        parts.append("template <>")
        parts.append(f"FA2_DEV void dkdv_hp_read<{kb}>(f32x16 (&dv)[4], f32x16 (&dk)[4], uint32_t tok) {{")
        for which, base0 in (("dv", 0), ("dk", 128)):
            for dt in range(4):
                base = base0 + (kb * 4 + dt) * 16
                outs = ", ".join(f'"=v"({which}[{dt}][{i}])' for i in range(16))
                body = "".join(f"v_accvgpr_read_b32 %{i}, a{base + i}\\n" for i in range(16))
                clob = ", ".join(f'"a{r}"' for r in range(256))
                parts.append(f'  asm volatile("{body}" : {outs} : "s"(tok) : {clob});')
        parts.append("}")
    return "\n".join(parts) + "\n"
