#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same code?  Splits each side into kernels, drops comments and directives that carry no
code, renumbers function-local labels per kernel, blanks the kernel's own symbol, then compares whole bodies and resource lines.
Usage: tools/kdiff.py <before> <after>    two .s files (hipcc ... --cuda-device-only -S), or two objects / .so;  exit 1 if they differ"""
import glob, os, re, shutil, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin/"
run = lambda *cmd, **kw: subprocess.run(cmd, capture_output=True, text=True, check=True, **kw).stdout
def asm_of(path, tmp):     # an object's code objects are disassembled and their metadata notes rewritten as .amdhsa_ lines
    if path.endswith(".s"):
        return open(path).read()
    local = os.path.join(tmp, "%d_%s" % (len(os.listdir(tmp)), os.path.basename(path)))
    shutil.copy(path, local)
    run(LLVM + "llvm-objdump", "--offloading", local)
    text = ""
    for co in sorted(glob.glob(local + ".*gfx950*")):
        text += run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands", co)
        for blk in run(LLVM + "llvm-readelf", "--notes", co).split("- .agpr_count:")[1:]:
            kv = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
            text += "\n%s:\n" % kv["name"] + "".join(".amdhsa_%s %s\n" % (k, kv.get(k)) for k in (
                "vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    return text
def kernels(text):         # name -> (body, {resource: value}): what stands between a global label `name:` and the next one
    out, name, labels = {}, None, {}
    for raw in text.splitlines():
        line = re.sub(r"\s+", " ", re.split(r";|//", raw)[0]).strip()
        m = re.match(r"(?:[0-9a-f]+ )?<?([A-Za-z_$][\w$.]*)>?:$", line)
        if line.startswith(".amdgpu_metadata") or "file format elf64-amdgpu" in line:   # (a library's next code object: its
            name = None                                                                  # path line is nobody's code)
        elif m and not re.match(r"L\d+$", m.group(1)):
            name, labels = m.group(1), {}
            out.setdefault(name, [[], {}])
        elif name and line.startswith(".amdhsa_") and not line.startswith(".amdhsa_kernel"):
            out[name][1][line.split(" ")[0]] = line.partition(" ")[2]
        elif name and line and (not line.startswith(".") or re.match(r"\.L\w+:$", line)):
            line = line.replace(name, "@self")
            out[name][0].append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?|<L\d+>|\bL\d+\b", lambda l: labels.setdefault(l.group(0).strip("<>"), "L%d" % len(labels)), line))
    for b, _ in out.values():      # a disassembled object shows the padding up to the next function's alignment as part of this one
        while b and b[-1] == "s_nop 0":
            b.pop()
    return {n: ("\n".join(b), r) for n, (b, r) in out.items() if r}      # kernels only: they have resource lines
with tempfile.TemporaryDirectory() as tmp:
    A, B = kernels(asm_of(sys.argv[1], tmp)), kernels(asm_of(sys.argv[2], tmp))
names = sorted(set(A) | set(B))
dem = dict(zip(names, run("c++filt", input="\n".join(names)).splitlines()))
by_body, used, bad = {}, {}, 0
for n, (body, _) in B.items():
    by_body.setdefault(body, []).append(n)
for n, (body, res) in A.items():
    mates = by_body.get(body, [])
    mate = n if n in B and (n in mates or not mates) else (mates[0] if mates else None)
    if not mates:
        bad += 1
        print("before only%s: %s" % (" (same name after, another body)" if n in B else "", dem[n]))
    if mate is not None:
        used.setdefault(mate, []).append(n)
        for k in sorted(set(res) | set(B[mate][1])):
            if res.get(k) != B[mate][1].get(k):
                bad += 1
                print("resources: %s\n    %s %s -> %s" % (dem[n], k, res.get(k), B[mate][1].get(k)))
for n in sorted(set(B) - set(used)):
    bad += 1
    print("after only: %s" % dem[n])
for mate, ns in used.items():
    if len(ns) > 1:
        print("collapsed: %d kernels before are one after: %s" % (len(ns), dem[mate]))
print("%d kernels before, %d after; %d identical under another name; %d differences" % (
    len(A), len(B), sum(n != m for m, ns in used.items() for n in ns), bad))
sys.exit(1 if bad else 0)
