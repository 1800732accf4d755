#!/usr/bin/env python3
"""Static instruction counts by class of the two lz_fast12_split_kernel instantiations in a gfx950 assembly listing
(profiles/producer_chain_isa_before.txt / _after.txt §1).  The listing is the device side of lizard_gpu.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-inline-asm -gline-tables-only --cuda-device-only \
          -S lizard_amd/csrc/lizard_gpu.hip -o kernels.s
    python scripts/isa_class_counts.py kernels.s [other.s ...]
    python scripts/isa_class_counts.py --blocks kernels.s     block table of the level-10 kernel (label, counts by class, loop nest,
                                                              source lines of lz_*.h, branches with their targets)

Classes: branch = s_branch / s_cbranch_*, wait = s_waitcnt, readlane = v_readlane / v_readfirstlane, smem = s_load / s_buffer_load,
salu = every other s_*, lds = ds_*, vmem = global / flat / buffer / scratch, valu = every other v_*.  Every line of the kernel's
function that starts with a tab and a lower-case mnemonic is counted, from the function's label to its .Lfunc_end."""
import re, sys, collections
def cls(op):
    if op.startswith('s_cbranch') or op=='s_branch': return 'branch'
    if op=='s_waitcnt': return 'wait'
    if op in('s_nop','s_barrier','s_sleep','s_endpgm','s_setprio'): return 'misc'
    if op.startswith('v_readlane') or op.startswith('v_readfirstlane'): return 'readlane'
    if op.startswith('s_load') or op.startswith('s_buffer_load'): return 'smem'
    if op.startswith('s_'): return 'salu'
    if op.startswith('ds_'): return 'lds'
    if op.startswith(('global_','flat_','buffer_','scratch_')): return 'vmem'
    if op.startswith('v_'): return 'valu'
    return 'misc'
for f in ([] if len(sys.argv) > 1 and sys.argv[1] == '--blocks' else sys.argv[1:]):
    cur=None; cnt={}
    for line in open(f):
        m=re.match(r'^(_ZN\S*lz_fast12_split_kernel\S*):',line)
        if m: cur=m.group(1); cnt[cur]=collections.Counter(); continue
        if line.startswith('.Lfunc_end'): cur=None
        if cur and re.match(r'^\t[a-z]',line):
            op=line.split()[0]
            cnt[cur][cls(op)]+=1
    for k,v in cnt.items(): print(f, 'true' if 'Lb1' in k else 'false', sum(v.values()), dict(sorted(v.items())))


def block_table(f):
    lines = open(f).read().split('\n')
    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m: files[int(m.group(1))] = (m.group(3) or m.group(2)).split('/')[-1]
    start = [i for i, l in enumerate(lines) if re.match(r'^_ZN\S*lz_fast12_split_kernelILb0', l)][0]
    end = [i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end')][0]
    cur, order, info = '(entry)', ['(entry)'], {'(entry)': dict(cnt=collections.Counter(), loop='', src=[], br=[])}
    for l in lines[start + 1:end]:
        m = re.match(r'^(\.LBB\d+_\d+):\s*(;.*)?', l)
        if m:
            cur = m.group(1); order.append(cur)
            info[cur] = dict(cnt=collections.Counter(), loop=(m.group(2) or '').strip('; '), src=[], br=[])
            continue
        m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
        if m:
            tag = '%s:%s' % (files.get(int(m.group(1)), '?'), m.group(2))
            if tag not in info[cur]['src'] and tag.startswith('lz_'): info[cur]['src'].append(tag)
            continue
        if l.startswith(';') and 'Loop' in l and not info[cur]['cnt']:
            info[cur]['loop'] += ' ' + l.strip('; ')
            continue
        if re.match(r'^\t[a-z]', l):
            op = l.split()[0]
            info[cur]['cnt'][cls(op)] += 1
            if cls(op) == 'branch': info[cur]['br'].append((op, l.split()[1]))
    for b in order:
        i = info[b]
        c = ' '.join('%s=%d' % kv for kv in sorted(i['cnt'].items()))
        print('%-12s n=%-3d %s | %s' % (b, sum(i['cnt'].values()), c, ' '.join(i['loop'].split())[:150]))
        print('      lines: ' + ' '.join(i['src'][:24]))
        print('      br: ' + str(i['br']))


if len(sys.argv) > 2 and sys.argv[1] == '--blocks':
    block_table(sys.argv[2])
    sys.exit(0)
