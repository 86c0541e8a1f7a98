"""Builds oracle/_ref/libwm_ref.so: the reference's own three OpenCL C kernels compiled for the CPU (test infrastructure).

Reads a reference checkout (kar-dim/Watermarking-GPU) at build time; nothing of it is committed here.
    python oracle/build_ref.py            # reference beside the repository: ../reference
    REF=/path/to/Watermarking-GPU python oracle/build_ref.py

Steps:
  1. extract the R"CLC(...)CLC" bodies of Watermark_GPU/kernels/{nvf,me_p3,scaled_neighbors_p3}.hpp and the RxMappings[64]
     initialiser (Watermark.hpp:29-39) into oracle/_ref/src/;
  2. compile each kernel as OpenCL C 1.2 for x86-64 in two variants:
       mad    -- the reference's build options (main.cpp:106-108): OpenCL defaults + -cl-mad-enable, on an FMA target;
       strict -- -ffp-contract=off (no contraction at all);
     nvf once per p in 3, 5, 7, 9 (-Dp=N, as main.cpp:106 passes it);
  3. rename every defined symbol to wmref_<name>_<variant> (llvm-objcopy --redefine-sym) so that the builds coexist;
  4. link them with oracle/clrt.c (the work-item runtime) and record oracle/_ref/MANIFEST.json: sha256 of each extracted
     source, the clang version, the flags.

Without a reference tree the script reports it and exits 0, leaving any existing oracle/_ref/ untouched (the GPU
machines receive a _ref built elsewhere).  The build is skipped when MANIFEST.json already records the same inputs.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLANG = os.environ.get("REF_CLANG", os.path.join(ROCM, "llvm", "bin", "clang"))
OBJCOPY = os.environ.get("REF_OBJCOPY", os.path.join(ROCM, "llvm", "bin", "llvm-objcopy"))
NM = os.environ.get("REF_NM", "nm")

KERNELS = {"nvf": "nvf.hpp", "me_p3": "me_p3.hpp", "scaled_neighbors_p3": "scaled_neighbors_p3.hpp"}
TARGET = ["-target", "x86_64-unknown-linux-gnu", "-mavx2", "-mfma", "-mf16c"]
CL_FLAGS = ["-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-O2", "-fPIC"] + TARGET
VARIANTS = {"mad": ["-cl-mad-enable"], "strict": ["-ffp-contract=off"]}
CC = os.environ.get("REF_CC", "gcc")  # the runtime: OpenMP from the same libgomp the oracle uses
RT_FLAGS = ["-O2", "-fPIC", "-fopenmp", "-Wall", "-Wextra", "-mavx2", "-mfma", "-mf16c"]
NVF_P = (3, 5, 7, 9)


def default_ref():
    return os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference")


def ref_files(ref):
    return [os.path.join(ref, "Watermark_GPU", "kernels", h) for h in KERNELS.values()] + \
        [os.path.join(ref, "Watermark_GPU", "Watermark.hpp")]


def ref_present(ref):
    """every file the build reads exists and is readable"""
    return all(os.path.isfile(f) and os.access(f, os.R_OK) for f in ref_files(ref))


def sha256(data):
    return hashlib.sha256(data if isinstance(data, bytes) else data.encode()).hexdigest()


def extract(ref):
    """returns {file name: text} for the kernel bodies and rx_mappings.inc"""
    src = {}
    kdir = os.path.join(ref, "Watermark_GPU", "kernels")
    for name, hpp in KERNELS.items():
        with open(os.path.join(kdir, hpp)) as f:
            bodies = re.findall(r'R"CLC\((.*?)\)CLC"', f.read(), re.S)
        if len(bodies) != 1:
            raise RuntimeError(f"{hpp}: expected one OpenCL raw string, found {len(bodies)}")
        src[name + ".cl"] = bodies[0]
    with open(os.path.join(ref, "Watermark_GPU", "Watermark.hpp")) as f:
        m = re.search(r"RxMappings\s*\[\s*64\s*\]\s*\{([^}]*)\}", f.read())
    if not m:
        raise RuntimeError("Watermark.hpp: RxMappings[64] initialiser not found")
    vals = [int(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()]
    if len(vals) != 64 or not all(0 <= v < 36 for v in vals):
        raise RuntimeError("Watermark.hpp: RxMappings is not 64 indices into the 36 Rx sums")
    src["rx_mappings.inc"] = "{" + ", ".join(map(str, vals)) + "}\n"
    return src


def run(cmd, **kw):
    subprocess.check_call(cmd, **kw)


def units():
    """(object name, source, kernel name, extra flags) for every kernel build; the kernel becomes wmref_<object name>"""
    out = []
    for var, vflags in VARIANTS.items():
        for p in NVF_P:
            out.append((f"nvf{p}_{var}", "nvf.cl", "nvf", vflags + [f"-Dp={p}"]))
        out.append((f"me_{var}", "me_p3.cl", "me", vflags))
        out.append((f"scaled_neighbors_p3_{var}", "scaled_neighbors_p3.cl", "scaled_neighbors_p3", vflags))
    return out


def build(ref):
    src = extract(ref)
    clang_version = subprocess.check_output([CLANG, "--version"], text=True).splitlines()[0]
    with open(os.path.join(HERE, "clrt.c"), "rb") as f:
        rt = f.read()
    manifest = {
        "reference": os.path.abspath(ref),
        "sources": {k: sha256(v) for k, v in sorted(src.items())},
        "runtime_sha256": sha256(rt),
        "clang": clang_version,
        "cl_flags": CL_FLAGS,
        "variants": VARIANTS,
        "nvf_p": list(NVF_P),
        "runtime_flags": RT_FLAGS,
        "builder_sha256": sha256(open(os.path.abspath(__file__), "rb").read()),
    }
    man_path = os.path.join(OUT, "MANIFEST.json")
    if os.path.exists(man_path) and os.path.exists(os.path.join(OUT, "libwm_ref.so")):
        with open(man_path) as f:
            old = json.load(f)
        if {k: v for k, v in old.items() if k != "symbols"} == manifest:
            return False
    tmp = tempfile.mkdtemp(prefix="wm_ref.")
    try:
        sdir = os.path.join(tmp, "src")
        os.makedirs(sdir)
        for name, text in src.items():
            with open(os.path.join(sdir, name), "w") as f:
                f.write(text)
        objs, symbols = [], {}
        for unit, cl, kname, flags in units():
            obj = os.path.join(tmp, unit + ".o")
            run([CLANG] + CL_FLAGS + flags + ["-c", os.path.join(sdir, cl), "-o", obj])
            defined = [ln.split()[0] for ln in
                       subprocess.check_output([NM, "-g", "--defined-only", "-P", obj], text=True).splitlines() if ln]
            if kname not in defined:
                raise RuntimeError(f"{unit}: kernel symbol {kname} not defined")
            ren = []
            for s in defined:
                new = f"wmref_{unit}" if s == kname else f"wmref_{unit}__{s}"
                ren += ["--redefine-sym", f"{s}={new}"]
            run([OBJCOPY] + ren + [obj])
            symbols[unit] = f"wmref_{unit}"
            objs.append(obj)
        rt_obj = os.path.join(tmp, "clrt.o")
        run([CC] + RT_FLAGS + ["-I", sdir, "-c", os.path.join(HERE, "clrt.c"), "-o", rt_obj])
        run([CC, "-shared", "-fopenmp", "-o", os.path.join(tmp, "libwm_ref.so"), rt_obj] + objs)
        for o in objs + [rt_obj]:
            os.remove(o)
        manifest["symbols"] = symbols
        with open(os.path.join(tmp, "MANIFEST.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        if os.path.exists(OUT):
            shutil.rmtree(OUT)
        shutil.move(tmp, OUT)
    finally:
        if os.path.exists(tmp):
            shutil.rmtree(tmp)
    return True


def main():
    ref = os.environ.get("REF") or default_ref()
    if not ref_present(ref):
        state = "kept" if os.path.exists(os.path.join(OUT, "libwm_ref.so")) else "absent"
        print(f"build_ref: no reference tree at {ref}; oracle/_ref {state}", file=sys.stderr)
        return 0
    built = build(ref)
    print(f"build_ref: oracle/_ref {'built' if built else 'up to date'}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
