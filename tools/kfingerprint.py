#!/usr/bin/env python3
"""One line per device symbol of every .hip file under a csrc directory: file, normalised name, a hash of the
instruction text, and (for kernels) vgpr/sgpr/agpr counts, LDS, scratch and kernarg sizes.

    tools/kfingerprint.py <tree>/instance-segmentation-attention_amd/csrc > a.txt     (once per tree, then `diff a.txt b.txt`)

A host-only change must leave the output identical.  Each file is compiled for the device alone with the Makefile's
own flags; addresses and encodings are stripped from the disassembly and the literal of a pc-relative address is replaced
by the symbol it points at (the linker's relocation, kept with --emit-relocs); lines are sorted by name, so the order in which
a file instantiates its kernels does not matter.  `View` moving between an anonymous namespace and the global one is
folded out of the mangled names.  The tool hashes text and reads nothing out of it."""
import concurrent.futures, hashlib, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/llvm/bin/"
META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size")


def norm(s):
    return re.sub(r"N12_GLOBAL__N_14ViewE|NS_4ViewE", "4View", s)


def flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    return re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def fingerprint(csrc, name, tmp, cxxflags):
    obj = os.path.join(tmp, name + ".o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *cxxflags, "--offload-device-only", "--no-gpu-bundle-output",
                           "-Xoffload-linker", "--emit-relocs", "-c", name, "-o", obj], cwd=csrc)
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "-r", obj], capture_output=True, text=True, check=True).stdout
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", obj], capture_output=True, text=True, check=True).stdout
    meta = {}
    for chunk in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        f = dict(re.findall(r"^(?:    )?\.(\w+):\s*(\S+)", chunk, re.M))
        meta[norm(f["name"])] = " ".join("%s=%s" % (k.split("_")[0], f[k]) for k in META)
    rows, cur = [], None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        rel = re.match(r"^\s+[0-9a-f]+:\s+R_AMDGPU_\S+\s+(\S+)$", line)
        if m:
            cur = [norm(m.group(1)), []]
            rows.append(cur)
        elif rel and cur and cur[1]:          # pc-relative literal: depends on where the kernel sits, so name its target
            cur[1][-1] = re.sub(r"0x[0-9a-f]+$|-?\d+$", norm(rel.group(1)), cur[1][-1])
        elif cur and line.strip():
            cur[1].append(norm(re.sub(r"\s*//.*$", "", line)).strip())
    return sorted("%s %s %s %s" % (name, sym, hashlib.sha256("\n".join(text).encode()).hexdigest()[:16], meta.get(sym, "-"))
                  for sym, text in rows)


def main():
    csrc = os.path.abspath(sys.argv[1])
    jobs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    cxxflags = flags(csrc)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for rows in ex.map(lambda n: fingerprint(csrc, n, tmp, cxxflags), names):
            print("\n".join(rows))


if __name__ == "__main__":
    main()
