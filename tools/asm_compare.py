"""dev helper: do two builds give the same gfx950 assembly, kernel by kernel?  (the proof a refactor of device code owes)
usage: python tools/asm_compare.py A B [--files wm_k_embed.hip,wm_k_bits.hip] [--must-match wm_k_embed.hip ...] [--jobs 4] [--keep DIR]

A and B are each a source tree (its watermarking-gpu_amd/csrc/*.hip are compiled to assembly with the CXXFLAGS of its own csrc/Makefile,
`--cuda-device-only -S`, into a temporary directory or --keep DIR/a, DIR/b), a directory of .s files, or one .s file.  Files pair up
by stem (wm_k_embed.hip ~ wm_k_embed.s).  A kernel is the text between its `.type SYMBOL,@function` and its end label, compared line
by line after dropping comments, blank lines, `__hip_cuid_` lines and the function index in local labels (.LBB12_3 -> .LBB_3).  Per
file: how many kernels are identical; per kernel that differs or exists on one side only: instructions, VGPRs, SGPRs, scratch and LDS
from the kernel descriptor and the compiler's waves per SIMD, A -> B, and which opcodes occur more or less often.
Exit code 1 when a file named with --must-match has any difference, 0 otherwise.  It compares the two builds and nothing else."""
import argparse
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("watermarking-gpu_amd", "csrc")
DESC = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "scratch": "private_segment_fixed_size", "lds": "group_segment_fixed_size"}


def makefile_flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, mk, re.M).group(1).strip()
    return var("HIPCC"), var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


def compile_tree(root, stems, outdir, jobs):
    csrc = os.path.join(root, CSRC)
    hipcc, flags = makefile_flags(csrc)
    os.makedirs(outdir, exist_ok=True)
    stems = stems or sorted(f[:-4] for f in os.listdir(csrc) if f.startswith("wm_k_") and f.endswith(".hip"))

    def one(stem):
        out = os.path.join(outdir, stem + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, stem + ".hip"), "-o", out], check=True)
        return stem, out

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, stems))


def side(path, stems, outdir, jobs):
    """{stem: path of its .s}"""
    if os.path.isfile(path):
        return {os.path.basename(path)[:-2]: path}
    if os.path.isdir(os.path.join(path, CSRC)):
        return compile_tree(path, stems, outdir, jobs)
    found = {f[:-2]: os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".s")}
    return {k: v for k, v in found.items() if not stems or k in stems}


def kernels(spath):
    """{symbol: {"text": [normalised lines], "ops": [opcodes], descriptor fields, "occ"}} of every .amdhsa_kernel of the file"""
    funcs, cur, last = {}, None, None
    for ln in open(spath, errors="replace"):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            cur = last = funcs.setdefault(m.group(1), {"text": [], "ops": []})
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
        if m and m.group(1) == "kernel":
            last = funcs.setdefault(m.group(2), {"text": [], "ops": []})
            last["kernel"] = True
        elif m and last is not None:
            for key, name in DESC.items():
                if m.group(1) == name:
                    last[key] = int(m.group(2))
        m = re.match(r";\s*Occupancy:\s*(\d+)", ln)
        if m and last is not None:
            last["occ"] = int(m.group(1))
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", ln):
            cur = None
            continue
        t = ln.split(";")[0].rstrip()
        if not t.strip() or "__hip_cuid_" in t or re.match(r"\s*\.(amdhsa_|end_amdhsa|section|p2align)", t):
            continue
        t = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", t)
        cur["text"].append(t)
        s = t.strip()
        if not s.endswith(":") and not s.startswith("."):
            cur["ops"].append(s.split()[0])
    return {k: v for k, v in funcs.items() if v.get("kernel")}


def demangle(sym):
    out = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip() or sym
    return out.split("(")[0].replace("void wmk::", "")


def opcode_note(a, b):
    """how the opcode sequences of the two sides relate"""
    if a == b:
        return "same opcode sequence, other registers / operands"
    ca, cb = collections.Counter(a), collections.Counter(b)
    if ca == cb:
        return "same opcodes in another order"
    return "opcode counts A -> B: " + ", ".join(f"{cb[o] - ca[o]:+d} {o}" for o in sorted(set(ca) | set(cb)) if ca[o] != cb[o])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--files", default="", help="comma-separated .hip / .s names (default: every wm_k_*.hip of a tree, every .s of a directory)")
    ap.add_argument("--must-match", action="append", default=[], help="file whose kernels must all be identical (repeatable)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", default=None, help="directory for the .s files compiled from source trees")
    a = ap.parse_args()
    stem = lambda f: os.path.splitext(os.path.basename(f))[0]
    stems = [stem(f) for f in a.files.split(",") if f]
    must = {stem(f) for f in a.must_match}
    tmp = a.keep or tempfile.mkdtemp(prefix="asm_compare_")
    sa, sb = side(a.a, stems, os.path.join(tmp, "a"), a.jobs), side(a.b, stems, os.path.join(tmp, "b"), a.jobs)
    failed = sorted(must - (set(sa) & set(sb)))
    for f in failed:
        print(f"{f}: --must-match, but not on both sides")
    fmt = lambda k: "-" if k is None else (f"insns {len(k['ops'])} vgpr {k.get('vgpr', 0)} sgpr {k.get('sgpr', 0)} scratch {k.get('scratch', 0)} "
                                           f"lds {k.get('lds', 0)} waves/SIMD {k.get('occ', 0)}")
    for f in sorted(set(sa) & set(sb)):
        ka, kb = kernels(sa[f]), kernels(sb[f])
        diff = [s for s in sorted(set(ka) | set(kb)) if s not in ka or s not in kb or ka[s]["text"] != kb[s]["text"]]
        print(f"{f}: {len(set(ka) | set(kb)) - len(diff)} of {len(set(ka) | set(kb))} kernels identical" + (", MUST MATCH" if diff and f in must else ""))
        for s in diff:
            x, y = ka.get(s), kb.get(s)
            note = "on one side only" if x is None or y is None else opcode_note(x["ops"], y["ops"])
            print(f"  differs  {demangle(s)}\n           A {fmt(x)}\n           B {fmt(y)}\n           {note}")
        if diff and f in must:
            failed.append(f)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
