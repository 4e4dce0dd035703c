#!/usr/bin/env python3
"""LDS bank-conflict model of k_me's accesses (lane groups and bank rules of
MI355X_MICROARCH.md §LDS): prints modelled LDS cycles per MB for candidate row strides
(box-sum rows S, window rows WW, block rows BS)."""
# LDS bank model of MI355X_MICROARCH.md §LDS: per instruction lane groups, bank = dword mod nb
G32 = [list(range(0,32)), list(range(32,64))]
G128 = [[0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27],[4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31]]
G128 += [[x+32 for x in g] for g in G128]
W128 = [list(range(i,i+8)) for i in range(0,64,8)]
def cycles(addrs, groups, nb, width):
    tot = 0
    for g in groups:
        banks = {}
        for ln in g:
            a = addrs.get(ln)
            if a is None: continue
            for k in range(width):
                banks.setdefault((a+k) % nb, set()).add(a+k)
        tot += max([len(v) for v in banks.values()] or [0])
    return tot
def ideal(groups): return len(groups)
kFsWin, R2 = 48, 32
def analyse(S, WW, BS):
    out = {}
    # (a) int4 store of row box sums: lane l<48 stores sq[l*S + x], x=0,4,..,28
    c = sum(cycles({l: l*S + x for l in range(48)}, W128, 32, 4) for x in range(0, R2, 4)); out['sq_store_b128'] = (c, 8*8)
    # (b) column reads sq[r*S + l], l < 32
    c = sum(cycles({l: r*S + l for l in range(32)}, G32, 32, 1) for r in range(kFsWin)); out['sq_col_read'] = (c, 2*kFsWin)
    # (c) fs_key reads as b32: dyw*S + dxw
    c = 0
    for mt in range(2):
        for nt in range(2):
            for reg in range(4):
                ad = {l: (16*nt + (l & 15))*S + 16*mt + 4*(l >> 4) + reg for l in range(64)}
                c += cycles(ad, G32, 32, 1)
    out['fs_read_b32'] = (c, 16*2)
    # (c') as b128
    c = 0
    for mt in range(2):
        for nt in range(2):
            ad = {l: (16*nt + (l & 15))*S + 16*mt + 4*(l >> 4) for l in range(64)}
            c += cycles(ad, G128, 64, 4)
    out['fs_read_b128'] = (c, 4*4)
    # (d) window row loads (box sums): lane l<48 reads win[l*WW + q]
    c = sum(cycles({l: l*WW + q for l in range(48)}, G32, 32, 1) for q in range(12)); out['win_row_read'] = (c, 24)
    # (e) A fragments: rows 4ks+g, dword 4mt + (i16>>2) + q
    c = 0
    for ks in range(12):
        for mt in range(2):
            for q in range(5):
                ad = {l: (4*ks + (l >> 4))*WW + 4*mt + ((l & 15) >> 2) + q for l in range(64)}
                c += cycles(ad, G32, 32, 1)
    out['A_frag'] = (c, 12*2*5*2)
    # (f) B fragments: blk[src*BS + q], src = 4ks+g-16nt-i16 (in range)
    c = 0
    for ks in range(12):
        for nt in range(2):
            for q in range(4):
                ad = {}
                for l in range(64):
                    src = 4*ks + (l >> 4) - (16*nt + (l & 15))
                    ad[l] = (src if 0 <= src < 16 else 0)*BS + q
                c += cycles(ad, G32, 32, 1)
    out['B_frag'] = (c, 12*2*4*2)
    # (g) one search SAD read from the window (win_sad_lane: lane -> row l>>2, dword l&3 of the
    # 16x16 block at offset (ox, oy), aligned pair w[0], w[1]), averaged over offsets: x 10
    offs = [(ox, oy) for ox in range(-16, 17) for oy in (-16, 0, 5, 16)]
    c = 0
    for ox, oy in offs:
        for k in range(2):
            ad = {l: ((l >> 2) + oy + 16)*WW + (((l & 3)*4 + ox + 16) >> 2) + k for l in range(64)}
            c += cycles(ad, G32, 32, 1)
    out['sad_read_x10'] = (round(10*c/len(offs)), 10*2*2)
    return out
def analyse_shared(S, WW):
    """k_me with one 48 x 96 window (rows of WW dwords) and one 48 x 80 box-sum table (rows of S
    ints) per workgroup of four macroblocks, block rows of 4 dwords between zero rows. Every entry
    is (modelled, conflict-free) LDS cycles of the whole workgroup; the total is divided by 4."""
    out = {}
    W4 = range(4)
    # (a) window fill: thread i + 256 k stores win[wy*WW + q], wy = i / 24, q = i % 24
    c = n = 0
    for k in range(5):
        for w in W4:
            ad = {l: ((i // 24)*WW + i % 24) for l in range(64) for i in [256*k + 64*w + l] if i < 48*24}
            c += cycles(ad, G32, 32, 1); n += 2 if ad else 0
    out['win_fill_store'] = (c, n)
    # (b) row loads of the box sums: wave w, lane l < 48 reads win[l*WW + 5w + q], q < 9
    c = sum(cycles({l: l*WW + 5*w + q for l in range(48)}, G32, 32, 1) for w in W4 for q in range(9)); out['win_row_read'] = (c, 4*9*2)
    # (c) int4 stores of the row sums: sq[l*S + 20w + x], x = 0, 4, .., 16
    c = sum(cycles({l: l*S + 20*w + x for l in range(48)}, W128, 32, 4) for w in W4 for x in range(0, 20, 4)); out['sq_store_b128'] = (c, 4*5*6)
    # (d) column sums: thread t < 160 (h = t / 80, c = t % 80) reads rows 16h + r, r < 31, writes rows 32h + dy, dy < 16
    c = 0
    for w in range(3):
        th = [t for t in range(64*w, 64*w + 64) if t < 160]
        c += sum(cycles({t % 64: (16*(t // 80) + r)*S + t % 80 for t in th}, G32, 32, 1) for r in range(31))
        c += sum(cycles({t % 64: (32*(t // 80) + dy)*S + t % 80 for t in th}, G32, 32, 1) for dy in range(16))
    out['sq_col_read_write'] = (c, 5*(31 + 16))
    # (e) fs_key reads (b128): wave w, (32nt + i16)*S + 16w + 16mt + 4g
    c = 0
    for w in W4:
        for mt in range(2):
            for nt in range(2):
                c += cycles({l: (32*nt + (l & 15))*S + 16*w + 16*mt + 4*(l >> 4) for l in range(64)}, G128, 64, 4)
    out['fs_read_b128'] = (c, 4*4*4)
    # (f) A fragments: rows 4ks + g, dwords 4w + (i16 >> 2) + q, q < 9 (both dx tiles)
    c = 0
    for w in W4:
        for ks in range(12):
            for q in range(9):
                c += cycles({l: (4*ks + (l >> 4))*WW + 4*w + ((l & 15) >> 2) + q for l in range(64)}, G32, 32, 1)
    out['A_frag'] = (c, 4*12*9*2)
    # (g) B fragments (b128): padded block row 4k + g - i16 + 15, rows of 4 dwords
    c = 4*sum(cycles({l: (4*k + (l >> 4) - (l & 15) + 15)*4 for l in range(64)}, G128, 64, 4) for k in range(8))
    out['B_frag_b128'] = (c, 4*8*4)
    # (h) one search SAD read of wave w (win_sad_lane), averaged over offsets: x 10 per MB
    offs = [(ox, oy) for ox in range(-16, 17) for oy in (-16, 0, 5, 16)]
    c = 0
    for w in W4:
        for ox, oy in offs:
            for k in range(2):
                ad = {l: ((l >> 2) + oy + 16)*WW + 4*w + (((l & 3)*4 + ox + 16) >> 2) + k for l in range(64)}
                c += cycles(ad, G32, 32, 1)
    out['sad_read_x10'] = (round(10*c/len(offs)), 4*10*2*2)
    return out
if __name__ == '__main__':
    print('one window per wave (S, WW, BS):')
    for S, WW, BS in [(32,12,4),(36,12,4),(36,13,5),(44,13,5),(33,13,5),(40,13,5),(52,13,5),(36,12,5)]:
        o = analyse(S, WW, BS)
        print(S, WW, BS, {k: f"{v[0]}/{v[1]}" for k, v in o.items()}, 'total', sum(v[0] for v in o.values()))
    print('one window per workgroup (S, WW), cycles per MB = total / 4:')
    for S, WW in [(80,24),(84,24),(84,25),(88,25),(92,25),(84,27),(84,28),(100,25)]:
        o = analyse_shared(S, WW)
        print(S, WW, {k: f"{v[0]}/{v[1]}" for k, v in o.items()}, 'per MB', sum(v[0] for v in o.values()) / 4)
