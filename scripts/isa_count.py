#!/usr/bin/env python3
"""Static instruction counts of one kernel in a device assembly file
(`make -C emqx_amd/csrc asm` writes gm_match.gfx950.s).

  scripts/isa_count.py FILE.s [SYMBOL-SUBSTRING ...]

Counts the instructions of the first function whose symbol contains every
given substring (default: the shipped k_match_fused instantiation), classified
by mnemonic prefix (v_ = VALU, s_ = SALU and scalar memory, buffer_/global_/
flat_/scratch_ = vector memory, ds_ = LDS) and a few named mnemonics, and the
number of waterfall loops: a v_readfirstlane_b32 run followed within a few
instructions by s_and_saveexec_b64 and a buffer op (the compiler's loop around
a buffer op whose descriptor it could not prove wave-uniform).  Nothing here
runs on a GPU.
"""
import re
import sys
from collections import Counter

NAMED = ["v_mov_b32", "s_and_saveexec_b64", "s_cbranch_execz", "v_readlane_b32", "v_writelane_b32", "s_nop",
         "v_mul_lo_u32", "v_mul_hi_u32", "v_lshl_add_u64", "v_lshlrev_b64", "v_cndmask_b32", "s_waitcnt",
         "v_readfirstlane_b32", "s_load_dword"]
VMEM = ("buffer_", "global_", "flat_", "scratch_")


def function_body(lines, subs):
    start = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and all(s in m.group(1) for s in subs):
            start = i
            name = m.group(1)
            break
    if start is None:
        raise SystemExit("no function matches %r" % (subs,))
    body = []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        body.append(ln)
    return name, body


def main():
    path = sys.argv[1]
    # k_match_fused<EXACT, NT, TOKPRIO, CMP, AB = false, FLAT = false>
    subs = sys.argv[2:] or ["13k_match_fusedILb1ELb1ELb1ELb1ELb0ELb0EE"]
    name, body = function_body(open(path).read().splitlines(), subs)
    ins = []
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        ins.append(t.split()[0])
    c = Counter(ins)
    tot = len(ins)
    valu = sum(n for m, n in c.items() if m.startswith("v_"))
    salu = sum(n for m, n in c.items() if m.startswith("s_"))
    vmem = sum(n for m, n in c.items() if m.startswith(VMEM))
    lds = sum(n for m, n in c.items() if m.startswith("ds_"))
    print("function", name)
    print("total %d  VALU %d  SALU %d  vector-memory %d  LDS %d  other %d" %
          (tot, valu, salu, vmem, lds, tot - valu - salu - vmem - lds))
    for pre in VMEM:
        n = sum(k for m, k in c.items() if m.startswith(pre))
        if n:
            print("  %-22s %d" % (pre + "*", n))
    for m in NAMED:
        n = sum(k for mm, k in c.items() if mm == m or mm.startswith(m + "_") or (m == "s_load_dword" and mm.startswith(m)))
        print("  %-22s %d" % (m, n))
    # waterfall loops: >= 4 v_readfirstlane_b32 then s_and_saveexec_b64 then a buffer op, all within 12 instructions
    wf = 0
    i = 0
    while i < len(ins):
        if ins[i] == "v_readfirstlane_b32":
            win = ins[i:i + 12]
            if win.count("v_readfirstlane_b32") >= 4 and "s_and_saveexec_b64" in win:
                k = win.index("s_and_saveexec_b64")
                if any(m.startswith("buffer_") for m in win[k:k + 4]):
                    wf += 1
                    i += 12
                    continue
        i += 1
    print("waterfall loops around buffer ops: %d" % wf)


if __name__ == "__main__":
    main()
