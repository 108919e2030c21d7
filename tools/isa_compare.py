#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel.

  hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S unit.hip -o dir/unit.s      (every unit that holds a kernel, both trees)
  tools/isa_compare.py BEFORE_DIR AFTER_DIR [--brief] [--allow REGEX] [--gone REGEX] [--rename 'OLD NAME=NEW NAME'] > report.txt

A kernel's text is everything from its label to .end_amdhsa_kernel (instructions and the descriptor block); block labels are renumbered per
kernel, the kernel's own symbol is masked and comments are dropped, so only code can differ.  Kernels are matched by demangled name with
namespaces dropped (a parameter type that moves between namespaces renames the symbol, not the code); --rename pairs a kernel whose signature
changed.  A kernel that differs is "offsets only" when every differing line is the same instruction with another immediate (a kernarg offset in
a scalar load or in the s_add_u32 / s_addc_u32 that forms a kernarg address) or the kernarg size.  Exit status 1 when the kernel sets differ,
when a kernel differs that --allow does not name, or when an allowed one grew in registers, scratch or instructions or changed its LDS size.
--gone names kernels removed on purpose: each is listed as GONE and does not fail the run.  --brief prints differing kernels only.
"""
import glob, os, re, shutil, subprocess, sys

FILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
RES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
IMM = re.compile(r"\b(0x[0-9a-f]+|\d+)$")

def kernels(d):
    out = {}
    for f in sorted(glob.glob(d + "/*.s")):
        lines = open(f).read().split("\n")
        for i, l in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
            if not m: continue
            sym = m.group(1)
            a = next(j for j, x in enumerate(lines) if x.startswith(sym + ":")); b = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
            labels = {}
            def ren(mm): return labels.setdefault(mm.group(0), ".L%d" % len(labels))
            body = [re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", ren, re.sub(r"\s*;.*$", "", x).replace(sym, "KERNEL")) for x in lines[a:b + 1]
                    if not re.match(r"\s*(;|\.file|\.loc|\.ident|\.cfi|\.section|\.text|\.p2align)", x) and x.strip()]
            name = re.sub(r"\(anonymous namespace\)::|t4k::", "", subprocess.check_output([FILT, sym], text=True).strip())
            res = {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", "\n".join(body)).group(1)) for k in RES}
            res["instructions"] = sum(1 for x in body if re.match(r"\s+[sv]_|\s+(ds|global|buffer|flat|scratch)_", x))
            out[name] = (os.path.basename(f), body, res)
    return out

def offsets_only(ba, bb):
    same_but_imm = lambda x, y: re.match(r"\s+(s_load_dword|s_add_u32|s_addc_u32)", x) and IMM.sub("", x) == IMM.sub("", y)
    return len(ba) == len(bb) and all(x == y or same_but_imm(x, y) or ".amdhsa_kernarg_size" in x for x, y in zip(ba, bb))

def main():
    opt = lambda o: [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == o]
    allow, gone, brief = opt("--allow"), opt("--gone"), "--brief" in sys.argv
    A, B = kernels(sys.argv[1]), kernels(sys.argv[2])
    for pair in opt("--rename"):
        old, new = pair.split("=")
        A[new] = A.pop(old); print("renamed    %s  ->  %s" % (old, new))
    bad = n_same = 0
    fmt = lambda r: "vgpr %d acc %d sgpr %d scratch %d lds %d instr %d" % tuple(r[k] for k in RES + ("instructions",))
    print("kernels before: %d   after: %d   per unit after: %s" % (len(A), len(B), ", ".join("%s %d" % (u, sum(1 for v in B.values() if v[0] == u)) for u in sorted({v[0] for v in B.values()}))))
    for n in sorted(set(A) - set(B)):
        if any(re.search(p, n) for p in gone): print("GONE         " + n)
        else: print("ONLY BEFORE  " + n); bad += 1
    for n in sorted(set(B) - set(A)): print("ONLY AFTER   " + n); bad += 1
    for n in sorted(set(A) & set(B)):
        (fa, ba, ra), (fb, bb, rb) = A[n], B[n]
        if ba == bb:
            n_same += 1
            if not brief: print("identical  %-18s %s" % (fb, n))
            continue
        grew = [k for k in ra if rb[k] > ra[k]] + (["lds changed"] if rb["group_segment_fixed_size"] != ra["group_segment_fixed_size"] else [])
        ok = any(re.search(p, n) for p in allow) and not grew
        print("%s  %-18s %s | %s%s | before %s | after %s" % ("changed  " if ok else "DIFFERENT", fb, n, "offsets only" if offsets_only(ba, bb) else "code differs",
                                                                      "; GREW: " + ", ".join(grew) if grew else "", fmt(ra), fmt(rb)))
        bad += 0 if ok else 1
    print("identical: %d of %d   not accepted: %d" % (n_same, len(set(A) & set(B)), bad))
    sys.exit(1 if bad else 0)

if __name__ == "__main__":
    main()
