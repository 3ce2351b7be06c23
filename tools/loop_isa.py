"""VALU instructions of a kernel's main loop in a .s file, per basic block and in total, split by issue class
(profiles/r04_microbench.txt): fast = add / sub / mul / fma / fmac f32, and / or / xor / not / mov, add / sub / shift u32 with vector
operands only (2.4-3.1 cycles), transcendental, slow = everything else and anything that reads a scalar register, VCC or EXEC
(4.2-4.7 cycles).  The main loop is the loop of the function with the most instructions; its blocks carry the compiler's
"in Loop: Header=" comments.  Importable: loop_counts(text, key) -> {"valu", "slow", "trans", "blocks": [(label, valu, slow, ds, salu, vmem)]}.
usage: python tools/loop_isa.py file.s mangled_kernel_substring [min_valu_to_list]"""
import collections
import re
import sys

FAST = {'v_add_f32', 'v_sub_f32', 'v_subrev_f32', 'v_mul_f32', 'v_fma_f32', 'v_fmac_f32', 'v_add_u32', 'v_sub_u32', 'v_subrev_u32',
        'v_and_b32', 'v_or_b32', 'v_xor_b32', 'v_not_b32', 'v_mov_b32', 'v_lshlrev_b32', 'v_lshrrev_b32', 'v_ashrrev_i32'}
TRANS = {'v_sqrt_f32', 'v_rcp_f32', 'v_rsq_f32', 'v_rcp_iflag_f32', 'v_exp_f32', 'v_log_f32'}
SCALAR_OPERAND = re.compile(r'(?<![\w.])(s\d+|s\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?)(?![\w])')


def base(op):
    return re.sub(r'_(e32|e64|dpp|sdwa)$', '', op)


def classify(line):
    """'fast', 'slow', 'trans' for a VALU instruction line, None otherwise"""
    op = line.split()[0]
    if not op.startswith('v_'):
        return None
    b = base(op)
    if b in TRANS:
        return 'trans'
    operands = line[len(op):].split(';')[0]
    if b not in FAST or op.endswith(('_dpp', '_sdwa')) or SCALAR_OPERAND.search(operands):
        return 'slow'
    return 'fast'


def function_lines(text, key):
    lines = text.split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\w*' + re.escape(key) + r'\w*:', l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[start:end]


def loop_counts(text, key):
    lines = function_lines(text, key)
    # blocks: (label, header of the loop it belongs to or None, instruction lines)
    blocks, cur = [], ['entry', None, []]
    for raw in lines[1:]:
        l = raw.strip()
        m = re.match(r'^(\.LBB\d+_\d+):\s*(;.*)?$', l) or re.match(r'^; %bb\.(\d+):\s*(;.*)?$', l)
        if m:
            blocks.append(cur)
            label = m.group(1) if m.group(1).startswith('.') else 'bb.' + m.group(1)
            note = m.group(2) or ''
            h = re.search(r'in Loop: Header=(BB\d+_\d+)', note)
            own = re.search(r'Loop Header', note) and not h
            cur = [label, h.group(1) if h else (label.lstrip('.L') if own else None), []]
            continue
        if l and not l.startswith((';', '.')):
            cur[2].append(l)
    blocks.append(cur)
    size = collections.Counter()
    for _, h, ins in blocks:
        if h:
            size[h] += len(ins)
    main = size.most_common(1)[0][0]
    out = {"header": main, "valu": 0, "slow": 0, "trans": 0, "blocks": []}
    for label, h, ins in blocks:
        if h != main:
            continue
        cl = collections.Counter(classify(i) for i in ins)
        valu = cl['fast'] + cl['slow'] + cl['trans']
        out["valu"] += valu
        out["slow"] += cl['slow']
        out["trans"] += cl['trans']
        out["blocks"].append((label, valu, cl['slow'], sum(i.startswith('ds_') for i in ins), sum(i.startswith('s_') for i in ins),
                              sum(i.startswith(('global_', 'buffer_', 'flat_', 'scratch_')) for i in ins)))
    return out


def main():
    text = open(sys.argv[1]).read()
    minv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    r = loop_counts(text, sys.argv[2])
    print(function_lines(text, sys.argv[2])[0].split(':')[0])
    print(f"main loop {r['header']}: valu {r['valu']} slow {r['slow']} trans {r['trans']} in {len(r['blocks'])} blocks")
    for label, valu, slow, ds, salu, vmem in r["blocks"]:
        if valu >= minv:
            print(f"  {label:12s} valu {valu:4d} slow {slow:3d} ds {ds:3d} salu {salu:3d} vmem {vmem:2d}")


if __name__ == "__main__":
    main()
