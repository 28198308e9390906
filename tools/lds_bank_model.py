#!/usr/bin/env python3
"""Host-side LDS bank model for the fused Winograd kernels (csrc/conv_wino.hip).  No GPU, no compiler: it enumerates the byte
addresses of every LDS access of the slab loop, per lane group, and counts the extra cycles of each wave instruction under the
rules of gfx950's LDS (64 banks of 4 bytes; an access is serviced in fixed lane groups, one LDS cycle per group, and each extra
distinct address on a busy bank within a group adds one cycle):

    instruction     lane groups                                                   bank of byte address a
    ds_read_b32     2 x 32: {0-31}, {32-63}                                       (a / 4) mod 32
    ds_write_b32    2 x 32: {0-31}, {32-63}                                       (a / 4) mod 32
    ds_read_b64     2 x 32: {0-31}, {32-63}                                       (a / 4) mod 64
    ds_read_b128    4 x 16: {0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32  (a / 4) mod 64
    ds_write_b64    4 x 16 contiguous                                             (a / 4) mod 32
    ds_write_b128   8 x 8 contiguous                                              (a / 4) mod 32

usage: python tools/lds_bank_model.py            the report kept as profiles/r13_lds_bank_model.txt
       python tools/lds_bank_model.py --search   every conflict-free pixel-pair layout of the 3x3 halo, smallest first
       python tools/lds_bank_model.py --wino15   the layouts of the F(4, 5) kernels' transformed tile, kept as
                                                 profiles/r19_wino15_lds_bank_model.txt
       python tools/lds_bank_model.py --wino44   the F(4x4, 3x3) kernel: operands from the halo against the row transform staged
                                                 in LDS, kept as profiles/r22_wino44_rowstage_lds_bank_model.txt
       python tools/lds_bank_model.py --wino44-exchange   the F(4x4, 3x3) kernel's output exchange by lane mapping, kept as
                                                 profiles/r32_wino44_epilogue_lds_bank_model.txt
"""
import sys

R128 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS = {
    "ds_read_b64": ([list(range(0, 32)), list(range(32, 64))], 64, 2),
    "ds_read_b128": (R128 + [[l + 32 for l in g] for g in R128], 64, 4),
    "ds_read_b32": ([list(range(0, 32)), list(range(32, 64))], 32, 1),
    "ds_write_b32": ([list(range(0, 32)), list(range(32, 64))], 32, 1),
    "ds_write_b64": ([list(range(16 * g, 16 * g + 16)) for g in range(4)], 32, 2),
    "ds_write_b128": ([list(range(8 * g, 8 * g + 8)) for g in range(8)], 32, 4),
}


def cycles(instr, addr):
    """(LDS cycles, conflict cycles) of one wave instruction; addr(lane) -> float index of the lane's first dword, or None when the
    lane is masked off."""
    groups, banks, dwords = GROUPS[instr]
    total = extra = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            a = addr(lane)
            if a is None:
                continue
            for d in range(dwords):
                per_bank.setdefault((a + d) % banks, set()).add(a + d)
        ways = max((len(v) for v in per_bank.values()), default=1)
        total += ways
        extra += ways - 1
    return total, extra


class Tally:
    def __init__(self):
        self.rows = []

    def add(self, name, instr, addrs):
        """addrs: one address function per wave instruction of a workgroup and slab"""
        t = e = 0
        for f in addrs:
            c, x = cycles(instr, f)
            t += c
            e += x
        self.rows.append((name, instr, len(addrs), t, e))

    def show(self, what="per workgroup and slab"):
        T = E = 0
        for name, instr, n, t, e in self.rows:
            print(f"  {name:<44} {instr:<14} {n:>4} wave instr  {t:>5} LDS cycles  {e:>5} conflict cycles  ({(t / (t - e)):.2f}-way)")
            T += t
            E += e
        print(f"  {what:<44} {'':<14} {'':>4}             {T:>5} LDS cycles  {E:>5} conflict cycles  = {100.0 * E / T:.1f} %")
        return T, E


def stage_writes(at, W, H):
    """halo staging, both kernels: item i = tid + 256 k = (pixel i / 4, float4 slot i % 4), pixels row-major"""
    items = W * H * 4
    out = []
    for k in range((items + 255) // 256):
        for wave in range(4):
            def f(lane, k=k, wave=wave):
                i = wave * 64 + lane + 256 * k
                if i >= items:
                    return None
                pix = i >> 2
                return at(pix // W, pix % W) + 4 * (i & 3)
            out.append(f)
    return out


kLDV = 20


def staged_3x3(t, at):
    """the parent's F(2x2, 3x3) slab: transform through Vs"""
    t.add("halo staging (10 x 18 pixels)", "ds_write_b128", stage_writes(at, 18, 10))
    rd, wr = [], []
    for wave in range(4):
        for r in range(4):
            for c in range(4):
                rd.append(lambda lane, wave=wave, r=r, c=c: at(2 * wave + r, 2 * (lane >> 3) + c) + 2 * (lane & 7))
        for pt in range(16):
            wr.append(lambda lane, wave=wave, pt=pt: (pt * 32 + wave * 8 + (lane >> 3)) * kLDV + 2 * (lane & 7))
    t.add("transform reads of the halo", "ds_read_b64", rd)
    t.add("transform writes of Vs (row stride 20)", "ds_write_b64", wr)
    fr = []
    for wave in range(4):
        for q in range(4):
            for ks in range(2):
                fr.append(lambda lane, wave=wave, q=q, ks=ks: ((4 * wave + q) * 32 + (lane & 31)) * kLDV + 4 * (lane >> 5) + 8 * ks)
    t.add("A fragments from Vs", "ds_read_b128", fr)


ROWS = [(0, 2), (1, 2), (2, 1), (1, 3)]   # the two window rows of wave i's row of B^T d


def rows_3x3(t, at):
    """this kernel: the operands come from the halo, lane = (tile lane & 31, channel group lane >> 5)"""
    t.add("halo staging (10 x 18 pixels)", "ds_write_b128", stage_writes(at, 18, 10))
    rd = []
    for wave in range(4):
        for ks in range(2):
            for r in ROWS[wave]:
                for c in range(4):
                    def f(lane, r=r, c=c, ks=ks):
                        tile = lane & 31
                        return at(2 * (tile >> 3) + r, 2 * (tile & 7) + c) + 8 * ks + 4 * (lane >> 5)
                    rd.append(f)
    t.add("operand reads of the halo (2 rows x 4 columns)", "ds_read_b128", rd)


def staged_15(t, vert, vs_at):
    """vs_at(point, tile, channel) -> float index in Vs of a transformed value (channel a multiple of 2 or 4)"""
    W, H, ldh = (16, 12, 16) if vert else (20, 8, 20)
    at = lambda y, x: (y * W + x) * ldh
    t.add(f"halo staging ({H} x {W} pixels)", "ds_write_b128", stage_writes(at, W, H))
    base = (lambda tl: (4 * (tl >> 4)) * W + (tl & 15)) if vert else (lambda tl: (tl >> 2) * W + 4 * (tl & 3))
    tap = (W if vert else 1) * ldh
    rd, wr, fr = [], [], []
    for wave in range(4):
        for j in range(8):
            rd.append(lambda lane, wave=wave, j=j: base(wave * 8 + (lane >> 3)) * ldh + 2 * (lane & 7) + j * tap)
            wr.append(lambda lane, wave=wave, j=j: vs_at(j, wave * 8 + (lane >> 3), 2 * (lane & 7)))
        for q in range(8):
            for ks in range(2):
                fr.append(lambda lane, q=q, ks=ks: vs_at(q, lane & 31, 4 * (lane >> 5) + 8 * ks))
    t.add("transform reads of the halo", "ds_read_b64", rd)
    t.add("transform writes of Vs", "ds_write_b64", wr)
    t.add("A fragments from Vs", "ds_read_b128", fr)


def vs_rows(ldv, pts=None):
    """[point][tile][channel] at row stride ldv, points pts floats apart (32 rows by default)"""
    pts = 32 * ldv if pts is None else pts
    return lambda q, tile, c: q * pts + tile * ldv + c


def vs_swizzled(q, tile, c):
    """tools/experiments/wino15_vs_swizzle.diff: rows of 16 floats, the row's four channel quads permuted by (tile / 4) % 4"""
    return (q * 32 + tile) * 16 + 4 * ((c >> 2) ^ ((tile >> 2) & 3)) + (c & 3)


def wino15():
    print("# tools/lds_bank_model.py --wino15: LDS cycles of one workgroup and slab of the F(4, 5) kernels, by the layout of Vs")
    tot = {}
    for name, vs in (("row stride 20 (kLDV of csrc/conv_wino.hip)", vs_rows(20)),
                     ("row stride 16, channel quad ^ (tile / 4) % 4 (tools/experiments/wino15_vs_swizzle.diff)", vs_swizzled)):
        for vert, o in ((False, "1x5"), (True, "5x1")):
            print(f"\n## F(4, 5) {o}: Vs at {name}")
            t = Tally()
            staged_15(t, vert, vs)
            tot[name, o] = t.show()
    print("\n## every plain row stride (a multiple of 4 floats, whole float4 reads) up to 80 KB of LDS, points 32 rows (+ pad) apart:")
    print("## modelled conflict cycles of (Vs writes, A fragments), the same in both orientations")
    best = None
    for ldv in range(16, 68, 4):
        for pad in range(0, 36, 4):
            t = Tally()
            staged_15(t, False, vs_rows(ldv, 32 * ldv + pad))
            w, f = t.rows[2][4], t.rows[3][4]
            if best is None or w + f < best[0]:
                best = (w + f, ldv, pad)
            if pad == 0:
                print(f"  row stride {ldv:>2}: writes {w:>4}  fragments {f:>4}")
    print(f"  the best plain layout: row stride {best[1]}, point pad {best[2]}: {best[0]} conflict cycles -- no plain stride serves both:")
    print("  the ds_write_b64 wants two neighbouring tiles' 16 floats in disjoint halves of 32 banks (stride = 16 mod 32), the")
    print("  ds_read_b128 wants 16 tiles' float4 in 16 different bank quads (stride = 4 mod 8, not 0 mod 16).  The swizzle gives both.")


def wino44():
    """F(4x4, 3x3): twelve waves, wave = (point row i, channel half nt), lane = (tile lane & 31, channel group lane >> 5); halo
    18 x 34 pixels of 8 channels, quads of four pixels 34 floats apart, rows 308 (Halo44 of csrc/conv_wino.hip)"""
    W, lq, lrow, ltrow = 34, 34, 308, 336
    at = lambda y, x: y * lrow + (x >> 2) * lq + (x & 3) * 8

    def staging(t):
        wr = []
        for k in range(2):
            for wave in range(12):
                def f(lane, k=k, wave=wave):
                    i = wave * 64 + lane + 768 * k
                    return None if i >= W * 18 * 2 else at((i >> 1) // W, (i >> 1) % W) + 4 * (i & 1)
                wr.append(f)
                wr.append(lambda lane, f=f: None if f(lane) is None else f(lane) + 2)
        t.add("halo staging (18 x 34 pixels, two float2 per item)", "ds_write_b64", wr)

    print("# tools/lds_bank_model.py --wino44: LDS cycles of one workgroup (twelve waves) and 8-channel slab of the F(4x4, 3x3) kernel")
    print("# (single ds_read_b64 / ds_write_b64; the compiler pairs neighbouring ones into ds_read2_b64 / ds_write2_b64)")
    print("\n## operands from the halo: every wave reads the three or four window rows of its point row, per column and half-step")
    t = Tally()
    staging(t)
    rd = []
    for wi in range(6):
        rows = (0, 2, 4) if wi == 0 else (1, 3, 5) if wi == 5 else (1, 2, 3, 4)
        for nt in range(2):
            for s in range(2):
                for c in range(6):
                    for r in rows:
                        rd.append(lambda lane, s=s, c=c, r=r: at(4 * ((lane & 31) >> 3) + r, 4 * (lane & 7) + c) + 4 * (lane >> 5) + 2 * s)
    t.add("operand reads of the halo", "ds_read_b64", rd)
    t.show()
    print(f"\n## the row transform staged: T[point row][tile row][x][8 channels], rows {ltrow} floats apart; thread < 544 = (tile row, x, channel pair)")
    t = Tally()
    staging(t)

    def item(i):
        if i >= 4 * W * 4:
            return None
        ty, x = (i >> 2) // W, (i >> 2) % W
        return ty, (x >> 2) * lq + (x & 3) * 8 + (i & 3) * 2
    rd, wr = [], []
    for wave in range(9):
        for k in range(6):
            rd.append(lambda lane, wave=wave, k=k: None if item(wave * 64 + lane) is None else
                      (4 * item(wave * 64 + lane)[0] + k) * lrow + item(wave * 64 + lane)[1])
            wr.append(lambda lane, wave=wave, k=k: None if item(wave * 64 + lane) is None else
                      (4 * k + item(wave * 64 + lane)[0]) * ltrow + item(wave * 64 + lane)[1])
    t.add("row pass: reads of the halo", "ds_read_b64", rd)
    t.add("row pass: writes of T", "ds_write_b64", wr)
    rd = []
    for wi in range(6):
        for nt in range(2):
            for s in range(2):
                for c in range(6):
                    rd.append(lambda lane, wi=wi, s=s, c=c: (4 * wi + ((lane & 31) >> 3)) * ltrow + (lane & 7) * lq + at(0, c) + 4 * (lane >> 5) + 2 * s)
    t.add("operand reads of T (the wave's own row)", "ds_read_b64", rd)
    t.show()


def wino44_exchange():
    """F(4x4, 3x3), the output exchange X[wave = (point row i, half nt)][column b][16 tiles][32 channels at kLDX4], one half of
    the patch: the accumulator side's writes, and the row side's reads before and after the four-channels-per-lane mapping"""
    ldx = 40
    xat = lambda i, nt, b, tl, ch: (((i * 2 + nt) * 4 + b) * 16 + tl) * ldx + ch
    print("# tools/lds_bank_model.py --wino44-exchange: LDS cycles of one workgroup (twelve waves) and half patch of the F(4x4, 3x3)")
    print(f"# kernel's output exchange, X[wave][b][tile][channel] at {ldx} floats per (b, tile) row")

    def writes():
        wr = []
        for wave in range(12):
            for e in range(8):
                for b in range(4):
                    wr.append(lambda lane, wave=wave, e=e, b=b:
                              xat(wave >> 1, wave & 1, b, (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), lane & 31))
        return wr

    print("\n## one channel of four pixels per lane: unit = (half, tile, row pair) per half-wave, 64 units over 24 half-waves")
    t = Tally()
    t.add("column side: writes of X", "ds_write_b32", writes())
    rd = []
    for p in range(3):
        for wave in range(12):
            for b in range(4):
                for k in range(5):
                    def f(lane, p=p, wave=wave, b=b, k=k):
                        un = 2 * wave + (lane >> 5) + 24 * p
                        if un >= 64:
                            return None
                        ap, rest = (un >> 1) & 1, un >> 2
                        return xat(ap + k, rest >> 3, b, (rest & 7) * 2 + (un & 1), lane & 31)
                    rd.append(f)
    t.add("row side: reads of X", "ds_read_b32", rd)
    t.show("per workgroup and half patch")

    print("\n## four channels of one pixel per lane: unit = (half, row pair, tiles t and t + 4) per wave, 32 units over 12 waves;")
    print("## lane = (channel quad lane & 7, b & 1 at bit 3, tile & 4 at bit 4, b >> 1 at bit 5)")
    t = Tally()
    t.add("column side: writes of X", "ds_write_b32", writes())

    def reads(lane_of):
        rd = []
        for p in range(3):
            for wave in range(12):
                ts = (wave >> 2) + 3 * p
                if ts >= 8:
                    continue
                for k in range(5):
                    def f(lane, wave=wave, ts=ts, k=k):
                        b, t2 = lane_of(lane)
                        return xat(((wave >> 1) & 1) + k, wave & 1, b, (ts & 3) + 4 * t2 + 8 * (ts >> 2), 4 * (lane & 7))
                    rd.append(f)
        return rd
    t.add("row side: reads of X", "ds_read_b128", reads(lambda lane: (((lane >> 3) & 1) + 2 * (lane >> 5), (lane >> 4) & 1)))
    t.show("per workgroup and half patch")
    print("\n## the same, had the lane's bits 3 .. 5 been (b, tile & 4) in order")
    t = Tally()
    t.add("row side: reads of X", "ds_read_b128", reads(lambda lane: ((lane >> 3) & 3, lane >> 5)))
    t.show("per workgroup and half patch")


def plain(ldh, W=18):
    return lambda y, x: (y * W + x) * ldh


def paired(rs, ps):
    """pixel pairs: (x, x + 1), x even, are 32 contiguous floats; pairs `ps` floats apart, rows `rs` floats apart"""
    return lambda y, x: y * rs + (x >> 1) * ps + (x & 1) * 16


def search():
    found = []
    for ps in range(32, 68, 4):
        for rs in range(9 * ps, 16 * ps + 4, 4):
            t = Tally()
            rows_3x3(t, paired(rs, ps))
            if sum(r[4] for r in t.rows) == 0:
                found.append((rs, ps))
    for rs, ps in sorted(found)[:12]:
        print(f"  pair stride {ps:>3} floats, row stride {rs:>4} floats: {10 * rs:>5} floats per buffer ({40 * rs} bytes)")


def main():
    if "--wino15" in sys.argv:
        wino15()
        return
    if "--wino44-exchange" in sys.argv:
        wino44_exchange()
        return
    if "--wino44" in sys.argv:
        wino44()
        return
    if "--search" in sys.argv:
        print("# conflict-free pixel-pair layouts of the 10 x 18 halo (staging ds_write_b128 and operand ds_read_b128), smallest first")
        search()
        return
    print("# tools/lds_bank_model.py: LDS cycles of one workgroup and slab (four waves), modelled from the byte addresses per lane group")
    print("\n## F(2x2, 3x3), parent: halo at pixel stride 24, transform through Vs")
    t = Tally()
    staged_3x3(t, plain(24))
    t.show()
    print("\n## F(2x2, 3x3), operands from the halo, had the halo kept its pixel stride of 24")
    t = Tally()
    rows_3x3(t, plain(24))
    t.show()
    print("\n## F(2x2, 3x3), operands from the halo, pixel pairs 36 floats apart, rows 336 floats apart (Halo3x3 of csrc/conv_wino.hip)")
    t = Tally()
    rows_3x3(t, paired(336, 36))
    t.show()
    for vert, name in ((False, "1x5"), (True, "5x1")):
        print(f"\n## F(4, 5) {name}: transform through Vs at row stride 20")
        t = Tally()
        staged_15(t, vert, vs_rows(kLDV))
        t.show()


if __name__ == "__main__":
    main()
