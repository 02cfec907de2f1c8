#!/usr/bin/env python3
"""kernel_diff.py OLD.o NEW.o [--rename REGEX=REPL ...]: what changed in the gfx950 machine code of one object
between two builds (no GPU needed).  Takes each object's gfx950 code object out of its offload bundle,
disassembles both with ROCm's llvm-objdump, pairs the kernels by demangled name (--rename rewrites OLD's names
first, for a template that lost or gained an argument) and prints the kernels only one build has and, for the
common ones, every instruction whose encoding differs.  Exit status 1 if anything was printed."""
import argparse
import difflib
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
INSN = re.compile(r"^\t(.*?)\s*// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)")


def code_object(path, arch):
    """The bundle's entry table: u64 count, then (u64 offset, u64 size, u64 triple length, triple) each."""
    blob = open(path, "rb").read()
    at = blob.index(MAGIC)
    (count,), pos = struct.unpack_from("<Q", blob, at + len(MAGIC)), at + len(MAGIC) + 8
    for _ in range(count):
        off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24:pos + 24 + tlen].decode()
        pos += 24 + tlen
        if triple.endswith(arch):
            return blob[at + off:at + off + size]
    sys.exit("%s: no %s code object in its offload bundle" % (path, arch))


def kernels(path, arch, renames=()):
    """{demangled name: [(encoding, text), ...]} of every function of the code object"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(path, arch))
        f.flush()
        asm = subprocess.run([OBJDUMP, "-d", "--demangle", f.name], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        if line.endswith(">:") and " <" in line:
            name = line[line.index(" <") + 2:-2]
            for pat, repl in renames:
                name = re.sub(pat, repl, name)
            cur = out.setdefault(name, [])
        elif cur is not None and (m := INSN.match(line)):
            cur.append((m.group(2).strip(), m.group(1)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="rewrite OLD's kernel names")
    args = ap.parse_args()
    old = kernels(args.old, args.arch, [r.split("=", 1) for r in args.rename])
    new = kernels(args.new, args.arch)
    changed = 0
    for tag, names in (("only in OLD", sorted(set(old) - set(new))), ("only in NEW", sorted(set(new) - set(old)))):
        print("%s: %d" % (tag, len(names)))
        for n in names:
            print("  " + n)
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        ops = [o for o in difflib.SequenceMatcher(None, [e for e, _ in a], [e for e, _ in b], autojunk=False).get_opcodes()
               if o[0] != "equal"]
        if ops:
            changed += 1
            print("%s: %d -> %d instructions" % (name, len(a), len(b)))
            for _, i0, i1, j0, j1 in ops:
                print("".join("  - [%d] %s  // %s\n" % (i, a[i][1], a[i][0]) for i in range(i0, i1)) +
                      "".join("  + [%d] %s  // %s\n" % (j, b[j][1], b[j][0]) for j in range(j0, j1)), end="")
    print("common: %d kernels, %d with a differing encoding" % (len(set(old) & set(new)), changed))
    return 1 if changed or set(old) ^ set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
