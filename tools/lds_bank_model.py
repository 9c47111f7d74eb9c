#!/usr/bin/env python3
"""LDS bank model of the attention tiles (csrc/attn_frag.h): cycles per wave of the score-fragment read (ds_read_b128, served in four
groups of 16 lanes) and of the transposing V read (ds_read_b64_tr_b16, two halves of 32 lanes) for the head-64 tile (128-byte rows,
chunk ^ (row & 7)) and for three candidate swizzles of the head-32 tile (64-byte rows): none, chunk ^ ((row >> 2) & 3), and the one
built, chunk ^ ((row >> 1) & 2); and for the head-128 tile (256-byte rows = one bank row each): none, chunk ^ (row & 15), and the one
built, chunk ^ ((row & 7) << 1), with the staging writes (ds_write_b128, groups of 8 consecutive lanes); and for the head-16 tile (32-byte rows, eight keys per bank row), whose score fragment is a ds_read_b64 (two
halves of 32 lanes: piece fq & 1 of chunk fq >> 1 of row fr): none, chunk ^ (row & 1), and the one built, chunk ^ ((row >> 3) & 1), with the staging writes on their 32 banks.  bank = (byte address / 4) % 64; a group costs as many cycles as its busiest bank has distinct
addresses.  Pure arithmetic: runs anywhere.  The device's own reading is the SQ_LDS_BANK_CONFLICT counter."""
from collections import Counter
G128 = [[0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27],[4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31]]
G128 += [[l+32 for l in g] for g in G128]
G64 = [list(range(32)), list(range(32,64))]
def cycles(groups, addr, nbytes, banks=64):
    tot = 0
    for g in groups:
        per_bank = {}
        for l in g:
            a = addr(l)
            for b in range(a//4, (a+nbytes)//4):
                per_bank.setdefault(b % banks, set()).add(b)
        tot += max(len(v) for v in per_bank.values())
    return tot
def swz(HD, row, chunk, kind):
    if HD == 64: return chunk ^ (row & 7)
    if HD == 16: return {'none': chunk, 'r1': chunk ^ (row & 1), 'built': chunk ^ ((row >> 3) & 1)}[kind]
    if HD == 128: return {'none': chunk, 'r15': chunk ^ (row & 15), 'built': chunk ^ ((row & 7) << 1)}[kind]
    return {'none': chunk, 'q2': chunk ^ ((row>>2)&3), 'built': chunk ^ ((row>>1)&2)}[kind]
G8 = [list(range(g*8, g*8+8)) for g in range(8)]
for HD, kinds in ((64, ['built']), (32, ['none','q2','built']), (128, ['none','r15','built']), (16, ['none','r1','built'])):
    for kind in kinds:
        if HD == 16:
            kc = [cycles(G64, lambda l: (kb*16+(l&15))*32 + 16*swz(16, kb*16+(l&15), (l>>4)>>1, kind) + ((l>>4)&1)*8, 8) for kb in range(4)]
        else:
          kc = [cycles(G128, lambda l: (kb*16+(l&15))*HD*2 + 16*swz(HD, kb*16+(l&15), kk*4+(l>>4), kind), 16) for kb in range(4) for kk in range(HD//32)]
        def va(l, key0, db):
            fr, fq = l&15, l>>4
            krow = key0 + fq*4 + (fr>>2); dcol = db*16 + (fr&3)*4
            return krow*HD*2 + 16*swz(HD, krow, dcol>>3, kind) + ((dcol>>2)&1)*8
        vc = [cycles(G64, lambda l: va(l, key0, db), 8) for key0 in (0,16,32,48) for db in range(HD//16)]
        if HD == 16:
            print("HD", HD, kind, "b64 cycles per read (2 = conflict-free):", set(kc), " tr_b16 cycles (2 = conflict-free):", set(vc))
            # staging: item i = lane + 64 * it is chunk i & 1 of tile row i >> 1; a store's banks are (address / 4) % 32
            wc = [cycles(G8, lambda l: ((l+64*it)>>1)*32 + 16*swz(16, (l+64*it)>>1, (l+64*it)&1, kind), 16, 32) for it in range(8)]
            print("HD", HD, kind, "b128 staging-write cycles per 64 lanes (8 = conflict-free):", set(wc))
            continue
        print("HD", HD, kind, "b128 cycles per read (4 = conflict-free):", set(kc), " tr_b16 cycles (2 = conflict-free):", set(vc))
        if HD == 128:      # staging: item i = lane + 64 * it is chunk i & 15 of tile row i >> 4 (tile_store / stage_kv)
            wc = [cycles(G8, lambda l: ((l+64*it)>>4)*256 + 16*swz(HD, (l+64*it)>>4, (l+64*it)&15, kind), 16) for it in range(8)]
            print("HD", HD, kind, "b128 staging-write cycles per 64 lanes (8 = conflict-free):", set(wc))
