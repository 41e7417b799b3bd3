#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.

  tools/kernel_code_diff.py <old> <new> [name filter]

<old> and <new> are each a directory of object files (quantize_amd/_ext/obj of a build: compared object by object, by file
name), one object file, or one assembly file written by `hipcc --offload-arch=gfx950 --cuda-device-only -S` with
quantize_amd/build.py's flags.  An object's code object is unbundled as tools/kernel_resources.sh does and disassembled with
llvm-objdump -d.

Of each kernel only the instruction lines count: no directives, no comments (an object's addresses and encodings are
comments), no __hip_cuid_ symbol, none of the zero padding or no-op fill behind a function's last instruction.  Kernels are keyed by their
demangled name without the parameter list, so a renamed argument type is no difference.  The filter keeps the kernels whose key contains it.  The comparison is of text: no
instruction is known by name.  Prints the kernels that only one side has, the kernels whose instructions differ (with the
first differing line) and the counts; the exit status is 1 if there is any of either.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def disassemble(obj):
    """llvm-objdump -d of the gfx950 code object bundled in a host object file; "" for an object that has none."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        if subprocess.call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET,
                            "--input=" + fat, "--output=" + co, "--unbundle"], stderr=subprocess.DEVNULL) != 0:
            return ""
        return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)


def split_objdump(text):
    """{mangled name: [instruction lines]}: a function starts at `<address> <name>:`; what follows `//` is dropped.  The zero
    bytes that align the NEXT function (an elided `...`, or a line whose encoding is all zero words) and the `s_nop 0` fill
    behind a function's last instruction (the section's long end fill lands behind whichever function is emitted last) are
    no part of this one: how many there are follows from the order in which the functions were emitted, so they go from the
    function's end.  A fill inside a function is followed by an instruction and stays."""
    out, pad, cur = {}, {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = " ".join(line.split("//")[0].split())
        if cur is not None and ins and not ins.startswith(("Disassembly of", "<")):
            cur.append(ins)
            words = line.split("//")[1].split(":")[-1].split() if "//" in line else []
            zero = ins in ("...", "s_nop 0") or (bool(words) and all(set(w) == {"0"} for w in words))
            pad[id(cur)] = pad.get(id(cur), 0) + 1 if zero else 0
    for cur in out.values():
        if pad.get(id(cur)):
            del cur[-pad[id(cur)]:]
    return out


def split_asm(text):
    """{mangled name: [instruction lines]} of a .s file: a function runs from its label to .Lfunc_end; block labels stay,
    numbered within the function (.LBB<function>_<n> -> .LBB_<n>), directives and `;` comments go."""
    out, cur = {}, None
    for line in text.splitlines():
        line = line.split(";")[0].strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and not line.startswith("."):
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line and (not line.startswith(".") or line.startswith(".LBB")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))
    return out


def kernels(path, flt):
    """{key: [instruction lines]} of one object or assembly file."""
    if path.endswith(".s"):
        funcs = split_asm(open(path).read())
    else:
        funcs = split_objdump(disassemble(path))
    names = [n for n in funcs if not n.startswith("__hip_cuid_")]
    plain = subprocess.check_output(["c++filt"] + names, text=True).splitlines() if names else []
    out = {}
    for mangled, name in zip(names, plain):
        if name.endswith(")"):                      # drop the parameter list: the last balanced (...) of the name
            depth, i = 0, len(name)
            while True:
                i -= 1
                depth += (name[i] == ")") - (name[i] == "(")
                if depth == 0:
                    break
            name = name[:i]
        if flt in name:
            assert name not in out, "two kernels named %s in %s" % (name, path)
            out[name] = funcs[mangled]
    return out


def pairs(old, new):
    """[(label, old file, new file)]: two files, or the objects of two directories by file name (None: one side lacks it)."""
    if not os.path.isdir(old) and not os.path.isdir(new):
        return [(os.path.basename(new), old, new)]
    ls = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    return [(f, os.path.join(old, f) if f in ls(old) else None, os.path.join(new, f) if f in ls(new) else None)
            for f in sorted(ls(old) | ls(new))]


def main(argv):
    if len(argv) not in (3, 4):
        sys.exit(__doc__)
    flt = argv[3] if len(argv) == 4 else ""
    total = only = differ = 0
    for label, old, new in pairs(argv[1], argv[2]):
        a = kernels(old, flt) if old else {}
        b = kernels(new, flt) if new else {}
        if not a and not b:
            continue
        gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        changed = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
        for k in gone:
            print("%s: only in old: %s" % (label, k))
        for k in added:
            print("%s: only in new: %s" % (label, k))
        for k in changed:
            i = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print("%s: differs: %s (%d -> %d instructions; line %d: %r -> %r)"
                  % (label, k, len(a[k]), len(b[k]), i, a[k][i] if i < len(a[k]) else None, b[k][i] if i < len(b[k]) else None))
        print("%s: %d kernels in old, %d in new, %d only in old, %d only in new, %d differ"
              % (label, len(a), len(b), len(gone), len(added), len(changed)))
        total += len(set(a) | set(b))
        only += len(gone) + len(added)
        differ += len(changed)
    print("kernels: %d, only in one side: %d, different: %d" % (total, only, differ))
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
