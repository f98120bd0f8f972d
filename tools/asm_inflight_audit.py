#!/usr/bin/env python3
"""Audit of the asm column loads of a resident kernel in the compiler's assembly
(hipcc -save-temps, the gfx950 .s file).

The pipelined pass of k_mgs_wres loads its ring buffers with asm statements, which
the compiler does not count: it treats a destination as written at the statement
and may copy, move to an AGPR or reuse the register before the data has landed.
This walks every path of one kernel's control-flow graph with the queue of vector
memory operations in flight (loads return in issue order; every `s_waitcnt
vmcnt(N)` retires all but the youngest N) and reports each instruction that names
a destination register of an asm load still in flight -- a v_mov, a v_accvgpr_*,
a second load into it, anything.  It also reports the kernel's scratch size.

The two arms of `if (t < 64)` in the all-gather are laid out one after the other as
masked blocks, so the graph holds a path through both, which no wave takes (the
test is the same for all lanes of a wave).  The kernel marks them with asm comments
`; gk-audit: arm NAME` ... `; gk-audit: arms end`; a path that reaches the marker
of a second arm before the end marker is dropped.

  python tools/asm_inflight_audit.py gk_resident-hip-amdgcn-amd-amdhsa-gfx950.s 'k_mgs_wresILi89ELi39ELi0ELi8ELb1ELi6E'

Exit status 0: no such instruction on any path and no scratch.
"""
import re
import sys

VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
REG1 = re.compile(r"\b([va])(\d+)\b")
REGN = re.compile(r"\b([va])\[(\d+):(\d+)\]")
ANON_CAP = 64  # vmcnt holds 6 bits: a longer run of unnamed operations behaves the same


def regs_of(text):
    out = set()
    for f, a, b in REGN.findall(text):
        out.update((f, k) for k in range(int(a), int(b) + 1))
    for f, a in REG1.findall(text):
        out.add((f, int(a)))
    return out


def parse(path, name):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l.split(":")[0] and l.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ins, labels, in_asm = [], {}, False
    for no in range(start + 1, end):
        l = lines[no]
        code = l.split(";;#")[0] if ";;#" in l else l
        m = re.search(r";\s*gk-audit:\s*(arm \S+|arms end)", l)
        if m and in_asm:
            ins.append((no + 1, "gk-audit " + m.group(1), True))
            continue
        if ";;#ASMSTART" in l:
            in_asm = True
            continue
        if ";;#ASMEND" in l:
            in_asm = False
            continue
        code = code.split(";")[0].rstrip()
        if not code.strip():
            continue
        if not code[0].isspace():
            if code.endswith(":"):
                labels[code[:-1]] = len(ins)
            continue
        s = code.strip()
        if s.startswith("."):
            continue
        ins.append((no + 1, s, in_asm))
    scratch = None
    for l in lines[end:end + 400]:
        m = re.search(r"\.private_segment_fixed_size\s+(\d+)", l) or re.search(r"ScratchSize:\s*(\d+)", l)
        if m:
            scratch = int(m.group(1))
            break
    return ins, labels, scratch


def squeeze(q):
    out, run = [], 0
    for e in q:
        if e is None:
            run += 1
            if run > ANON_CAP:
                continue
        else:
            run = 0
        out.append(e)
    return tuple(out)


def main():
    path, name = sys.argv[1], sys.argv[2]
    ins, labels, scratch = parse(path, name)
    label_at = {v for v in labels.values()}
    bad, seen, work = {}, set(), [(0, (), None)]
    nasm = sum(1 for _, s, a in ins if a and s.startswith("global_load"))
    while work:
        pc, q, arm = work.pop()
        while pc < len(ins):
            if pc in label_at or pc == 0:
                if (pc, q, arm) in seen:
                    break
                seen.add((pc, q, arm))
            no, s, in_asm = ins[pc]
            op = s.split()[0]
            if op == "gk-audit":
                new = None if s.endswith("arms end") else s.split()[-1]
                if new is not None and arm is not None and new != arm:
                    break  # a second arm of a wave-uniform branch: no wave takes this path
                arm = new
                pc += 1
                continue
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", s)
                if m:
                    n = int(m.group(1))
                    q = q[len(q) - n:] if n < len(q) else q
                    if n == 0:
                        q = ()
                pc += 1
                continue
            live = set().union(*[e[1] for e in q if e is not None]) if any(e is not None for e in q) else set()
            if live:
                hit = regs_of(s.split(None, 1)[1] if " " in s else "") & live
                if hit:
                    src = sorted({e[0] for e in q if e is not None and e[1] & hit})
                    bad.setdefault(no, (s, src))
            if VMEM.match(op):
                if in_asm and "_load" in op:
                    dst = s.split(None, 1)[1].split(",")[0]
                    q = squeeze(q + ((no, frozenset(regs_of(dst))),))
                else:
                    q = squeeze(q + (None,))
            if op == "s_endpgm":
                break
            if op == "s_branch":
                pc = labels[s.split()[1]]
                continue
            if op.startswith("s_cbranch"):
                work.append((labels[s.split()[1]], q, arm))
            pc += 1
    print(f"{name}: {len(ins)} instructions, {nasm} asm loads, {len(seen)} (block, queue) states, scratch {scratch} B/lane")
    for no in sorted(bad):
        s, src = bad[no]
        print(f"  line {no}: {s}    <- names a register of the asm load(s) at line(s) {src}, still in flight")
    print("clean" if not bad and not scratch else "NOT clean")
    sys.exit(0 if not bad and not scratch else 1)


if __name__ == "__main__":
    main()
