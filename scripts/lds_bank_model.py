#!/usr/bin/env python3
"""LDS bank model of k_pnet's split conv2 operand reads (host only, no GPU).

Restates the per-lane byte addresses of conv2's operand reads for one tile and one split plane and
counts LDS-array cycles per read kind under the CDNA4 bank rules:

  ds_read_b32    lane groups {0-31}, {32-63};              bank = (a / 4) mod 32
  ds_read_b64    lane groups {0-31}, {32-63};              bank = (a / 4) mod 64
  ds_read_b128   lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32 for the upper half);
                 bank = (a / 4) mod 64

A group takes one cycle; every further distinct dword on a bank that is already busy in the group
adds one (equal addresses broadcast).  The figures are modelled, not measured: they say where
the replays are, the counters (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE) say how many there are.

  python scripts/lds_bank_model.py                 # the parent's layout and the packed layout
  python scripts/lds_bank_model.py --frag linear --read01 h8 --pitch-a 22 --pitch-c 21
"""
import argparse

PC = 18            # conv2 output rows / columns per tile
PP = 20            # pooled rows / columns per tile
NPOS = PC * PC     # 324 positions, 16 per fragment

G32 = [list(range(0, 32)), list(range(32, 64))]
_g128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
         [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = _g128 + [[l + 32 for l in g] for g in _g128]


def cycles(addrs, nbytes, groups, nbanks):
    """LDS cycles of one wave instruction: addrs[lane] = byte address, nbytes per lane."""
    total = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            for d in range(addrs[lane] // 4, (addrs[lane] + nbytes + 3) // 4):
                per_bank.setdefault(d % nbanks, set()).add(d)
        total += max(len(s) for s in per_bank.values())
    return total


def read_b32(addrs):
    return cycles(addrs, 4, G32, 32)


def read_b64(addrs):
    return cycles(addrs, 8, G32, 64)


def read_b128(addrs):
    assert all(a % 16 == 0 for a in addrs), 'ds_read_b128 wants 16-byte aligned addresses'
    return cycles(addrs, 16, G128, 64)


def read_h8(addrs):
    """ld_h8: 16 bytes as two ds_read_b64"""
    assert all(a % 8 == 0 for a in addrs), 'ds_read_b64 wants 8-byte aligned addresses'
    return read_b64(addrs) + read_b64([a + 8 for a in addrs])


def fragments(kind, row0=0):
    """The tile's fragments as lists of 16 (row, col) positions, rows row0..17 (row0 = 2: a
    vertical-reuse continuing tile).  'linear': position p = 16 f + lane of the row-major 18-wide
    order (the last fragment repeats the last position).  'rows': one fragment per row for columns
    0..15, then columns 16, 17 in strips of 8 rows (lane = 2 row + col - 16)."""
    if kind == 'linear':
        pos = [(p // PC, p % PC) for p in range(row0 * PC, NPOS)]
        pos += [pos[-1]] * (-len(pos) % 16)
        return [pos[i:i + 16] for i in range(0, len(pos), 16)]
    assert kind == 'rows'
    fr = [[(r, c) for c in range(16)] for r in range(row0, PC)]
    strip = [(r, c) for r in range(row0, PC) for c in (16, 17)]
    strip += [strip[-1]] * (-len(strip) % 16)
    return fr + [strip[i:i + 16] for i in range(0, len(strip), 16)]


def tap(t):
    return t // 3, t % 3


def parent_reads(frag):
    """[cell][12 halves] at pitch 20: steps 0, 1 as ld_h8, step 2 as four ds_read_b32 per lane."""
    cell = lambda r, c: (r * PP + c) * 24
    s01 = 0
    for s in range(2):
        a = [cell(r + tap(4 * s + g)[0], c + tap(4 * s + g)[1]) for g in range(4) for (r, c) in frag]
        s01 += read_h8(a)
    s2 = 0
    for jj in range(4):
        a = []
        for g in range(4):
            for (r, c) in frag:
                if g == 0:
                    a.append(cell(r + 2, c + 2) + 4 * jj)
                elif g == 3:
                    a.append(cell(r + 2, c + 2) + 16)
                else:
                    t = tap(4 * (g - 1) + jj)
                    a.append(cell(r + t[0], c + t[1]) + 16)
        s2 += read_b32(a)
    return s01, s2


def packed_reads(frag, pitch_a, pitch_c, off_a, off_c, read01):
    """Sub-planes A[cell][ch 0..7] (16 B cells) and C[cell] = [c8 c9 of the cell | c8 c9 of the next
    column] (8 B cells): steps 0, 1 read A at taps g / 4 + g; step 2 reads A at tap 8 (group 0) and
    the 16 bytes at C[(r + g - 1, c)] (groups 1..3), all lanes as ld_h8."""
    A = lambda r, c: off_a + (r * pitch_a + c) * 16
    C = lambda r, c: off_c + (r * pitch_c + c) * 8
    rd = read_b128 if read01 == 'b128' else read_h8
    s01 = 0
    for s in range(2):
        s01 += rd([A(r + tap(4 * s + g)[0], c + tap(4 * s + g)[1]) for g in range(4) for (r, c) in frag])
    a = [A(r + 2, c + 2) if g == 0 else C(r + g - 1, c) for g in range(4) for (r, c) in frag]
    return s01, read_h8(a)


def model(layout, frag_kind, row0=0, **kw):
    s01 = s2 = 0
    frs = fragments(frag_kind, row0)
    for fr in frs:
        a, b = parent_reads(fr) if layout == 'parent' else packed_reads(fr, **kw)
        s01 += a
        s2 += b
    # conflict-free: 4 cycles per 16-byte read (steps 0, 1: two of them), 2 per ds_read_b32 (four)
    return {'fragments': len(frs), 'steps01': s01, 'step2': s2, 'free01': 8 * len(frs),
            'free2': (8 if layout == 'parent' else 4) * len(frs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frag', choices=['linear', 'rows'], default='rows', help='fragment -> position map')
    ap.add_argument('--read01', choices=['b128', 'h8'], default='b128', help='read kind of k-steps 0 and 1')
    ap.add_argument('--pitch-a', type=int, default=20, help='row pitch of sub-plane A (16-byte cells)')
    ap.add_argument('--pitch-c', type=int, default=20, help='row pitch of sub-plane C (8-byte cells)')
    ap.add_argument('--off-a', type=int, nargs=2, default=[3216, 12832], help='byte offset of A, planes 0 and 1')
    ap.add_argument('--off-c', type=int, nargs=2, default=[16, 9632], help='byte offset of C, planes 0 and 1')
    ap.add_argument('--row0', type=int, default=0, help='first conv2 row (2: vertical-reuse continuing tile)')
    a = ap.parse_args()
    p = model('parent', 'linear', a.row0)
    print('LDS cycles per tile and plane (conflict-free in brackets)')
    print(f"parent  [cell][12] pitch 20, linear fragments ({p['fragments']}):")
    print(f"  k-steps 0, 1 (two 16-byte reads)   {p['steps01']} ({p['free01']})")
    print(f"  k-step 2 (eight ds_read_b32)       {p['step2']} ({p['free2']})")
    print(f"  total {p['steps01'] + p['step2']}, replays {p['steps01'] + p['step2'] - p['free01'] - p['free2']}")
    tot = rep = 0
    for pl in range(2):
        q = model('packed', a.frag, a.row0, pitch_a=a.pitch_a, pitch_c=a.pitch_c, off_a=a.off_a[pl],
                  off_c=a.off_c[pl], read01=a.read01)
        print(f"packed  A pitch {a.pitch_a}, C pitch {a.pitch_c}, {a.frag} fragments ({q['fragments']}), plane {pl}:")
        print(f"  k-steps 0, 1 ({a.read01})              {q['steps01']} ({q['free01']})")
        print(f"  k-step 2 (one 16-byte read, h8)    {q['step2']} ({q['free2']})")
        t = q['steps01'] + q['step2']
        print(f"  total {t}, replays {t - q['free01'] - q['free2']}")
        tot += t
        rep += t - q['free01'] - q['free2']
    print(f"packed, mean of the planes: total {tot / 2:g}, replays {rep / 2:g}")


if __name__ == '__main__':
    main()
