"""dev helper: does a build overwrite the data registers of a 96- or 128-bit store in the very next instruction?
usage: python tools/store_hazard_scan.py FILE.s [...]        (assembly as tools/asm_compare.py --keep DIR leaves it)

Why: on gfx950 a `buffer_store_dwordx4 v[a:a+3], ..., sN offen` followed DIRECTLY by a vector instruction that writes v[a] stores
that instruction's result in alternate groups of four lanes instead of the pixel (seen on an MI355X with a scratch variant of
k_embed_signs_multi whose copies were stored without the wave-uniform branch between them).  The compiler
pads this pair only when the store's scalar offset is an immediate; store4's (wm_device.hpp) is a register.  One instruction of any
kind in between is enough.  Per file: the wide stores, those whose data a vector instruction writes in the next instruction, and
within the next two.  Exit code 1 when any file has a store of the first kind."""
import re
import sys


def scan(path, depth):
    ins = []
    for ln in open(path, errors="replace"):
        t = ln.split(";")[0].strip()
        if t and not t.endswith(":") and not t.startswith("."):
            ins.append(t)
    stores = hits = 0
    for n, t in enumerate(ins):
        m = re.match(r"(buffer|global|flat)_store_dwordx[34] v\[(\d+):(\d+)\]", t)
        if not m:
            continue
        stores += 1
        lo, hi = int(m.group(2)), int(m.group(3))
        for t2 in ins[n + 1:n + 1 + depth]:
            if t2.startswith(("s_cbranch", "s_branch", "s_endpgm")):
                break
            w = re.match(r"v_\w+ v\[(\d+):(\d+)\]", t2) or re.match(r"v_\w+ v(\d+),", t2)
            if w and int(w.group(1)) <= hi and int(w.group(w.lastindex)) >= lo:
                hits += 1
                break
    return stores, hits


bad = 0
for p in sys.argv[1:]:
    stores, next1 = scan(p, 1)
    print(f"{p}: {stores} wide stores, data written by the next instruction: {next1}, within two: {scan(p, 2)[1]}")
    bad += next1
sys.exit(1 if bad else 0)
