"""Are the kernels of two builds of libart.so the same machine code?  The comparison DESIGN.md §4.7 describes, for a
change that should not move the kernels (a refactor, a new kernel beside the old ones):

    python tools/kernel_identity.py OLD.so NEW.so [--objdump /opt/rocm/llvm/bin/llvm-objdump]

Kernels are paired by name: the mangled name up to the end of its template-argument list, a leading scalar-type
argument (`d`, `f`) dropped and the parameter list ignored, so k_accum<double>(PassGeom, Work<double>) pairs with
k_accum(PassGeom, Work).  Each pair prints its VGPR / SGPR / spill / scratch / LDS figures and code size, and whether the
symbol's bytes are equal; otherwise how many bytes differ and where.  With --objdump, a kernel whose bytes differ is
disassembled from both builds and the instruction diff printed.  Exit status 1 when a kernel is unpaired or a figure
or a size differs (differing bytes at equal size are reported, not judged: a pc-relative call to an out-of-line helper
that moved changes its literal).  Reads ELF bytes only (tools/kernel_resources.py): no GPU."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402

FIGURES = ((".vgpr_count", "vgpr"), (".agpr_count", "agpr"), (".sgpr_count", "sgpr"), (".vgpr_spill_count", "spill"),
           (".private_segment_fixed_size", "scratch"), (".group_segment_fixed_size", "lds"), (".code_size", "code"))


def pair_key(mangled):
    """The pairing key of a kernel symbol: its (nested) name and template arguments, without a leading scalar type
    argument and without the parameter list.  Template arguments are literals (L<type><value>E) or builtin types."""
    m = re.match(r"_ZL?(N?)", mangled)
    if not m:
        return mangled
    at, nested, names = m.end(), bool(m.group(1)), []
    while True:
        n = re.compile(r"\d+").match(mangled, at)
        if not n:
            break
        at = n.end() + int(n.group())
        names.append(mangled[n.end():at])
        if not nested:
            break
    args = []
    if mangled[at:at + 1] == "I":
        at += 1
        while mangled[at] != "E":
            a = re.compile(r"L[a-z]n?\d+E|[a-z]").match(mangled, at)
            if not a:
                raise ValueError(f"template argument not understood at {at} in {mangled}")
            args.append(a.group())
            at = a.end()
    if args and args[0] in ("d", "f"):
        del args[0]
    return "::".join(names) + ("<" + ",".join(args) + ">" if args else "")


def code_by_kernel(path):
    """{kernel symbol: (metadata with .code_size, code bytes, code object bytes)} of a library."""
    out = {}
    for co in kr.code_objects(kr.fatbin(path)):
        code = kr.function_code(co)
        for k in kr.kernel_metadata(co):
            k[".code_size"] = len(code[k[".name"]])
            out[k[".name"]] = (k, code[k[".name"]], co)
    return out


def disassembly(objdump, co, symbol):
    """The instructions of one symbol, addresses and encodings stripped from the text but the literal words kept."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        text = subprocess.run([objdump, "-d", "--disassemble-symbols=" + symbol, f.name], check=True, capture_output=True, text=True).stdout
    lines = []
    for ln in text.splitlines():
        m = re.match(r"\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:\s*(.*)$", ln)
        if m:
            lines.append(f"{m.group(1):<60} // " + re.sub(r"\s*<\S*>$", "", m.group(2)))  # less the branch target's symbol
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--objdump", help="llvm-objdump: print the instruction diff of every kernel whose bytes differ")
    a = ap.parse_args()
    old, new = code_by_kernel(a.old), code_by_kernel(a.new)
    by_key = {}
    for side, ks in enumerate((old, new)):
        for name in ks:
            by_key.setdefault(pair_key(name), [[], []])[side].append(name)
    bad = same = differ = 0
    for key, (o, n) in sorted(by_key.items()):
        if len(o) != 1 or len(n) != 1:
            print(f"{key}: UNPAIRED old {o or '-'} new {n or '-'}")
            bad += 1
            continue
        (ko, co, oo), (kn, cn, on) = old[o[0]], new[n[0]]
        fo = [ko.get(f, 0) for f, _ in FIGURES]
        fn = [kn.get(f, 0) for f, _ in FIGURES]
        figs = " ".join(f"{label} {x}" if x == y else f"{label} {x} -> {y} DIFFERS" for (_, label), x, y in zip(FIGURES, fo, fn))
        if fo != fn:
            bad += 1
            print(f"{key}: {figs}")
            continue
        if co == cn:
            same += 1
            print(f"{key}: {figs} bytes identical")
            continue
        differ += 1
        offs = [i for i, (x, y) in enumerate(zip(co, cn)) if x != y]
        print(f"{key}: {figs} {len(offs)} bytes differ at " + " ".join(hex(i) for i in offs[:16]) + (" ..." if len(offs) > 16 else ""))
        if a.objdump:
            do, dn = disassembly(a.objdump, oo, o[0]), disassembly(a.objdump, on, n[0])
            for ln in difflib.unified_diff(do, dn, "old", "new", n=2, lineterm=""):
                print("    " + ln)
    print(f"{len(old)} kernels in {a.old}, {len(new)} in {a.new}: {same} pairs byte-identical, {differ} with equal figures and size but "
          f"differing bytes, {bad} unpaired or with differing figures")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
