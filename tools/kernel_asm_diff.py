#!/usr/bin/env python3
"""Do two trees compile to the same kernels?  A per-kernel diff of gfx950 assembly.

  tools/kernel_asm_diff.py OLD_TREE NEW_TREE volume.hip [more.hip ...]   compile gravit_amd/csrc/<file> of both trees, compare
  tools/kernel_asm_diff.py --asm OLD.s NEW.s                             compare two ready assembly files

Each .hip is compiled with gravit_amd._build.FLAGS (of THIS tree) plus --offload-device-only -S, the two trees side by side.  Per kernel
(every name that has a kernel descriptor) the lines between its label and its descriptor are compared, comments dropped and the
local labels (.LBB*, .Ltmp*, .Lfunc_end*) replaced by one token, since a kernel added in front renumbers them.  Printed: the counts
of identical, differing, new and vanished kernels, for each differing kernel both instruction counts and the kernel info side by
side, and for each new kernel its own.  Exit status 1 when a kernel differs or has vanished, else 0.  It is a diff: it knows no instruction.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LOCAL = re.compile(r"\.L(?:BB|tmp|func_end|func_begin)[0-9_]+")
_DESC = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
# the kernel info's rows (the comment block behind a descriptor), then the metadata's
INFO = [("VGPRs", "NumVgprs"), ("AGPRs", "NumAgprs"), ("SGPRs", "TotalNumSgprs"), ("SGPR spills", ".sgpr_spill_count"),
        ("VGPR spills", ".vgpr_spill_count"), ("scratch", "ScratchSize"), ("LDS", "LDSByteSize"), ("occupancy", "Occupancy")]


def _code(line):
    """A line without its comment and outer blanks, local labels as one token."""
    return _LOCAL.sub(".L", line.split(";", 1)[0].strip())


def parse(text):
    """{kernel: {"body": [lines], "insts": n, "info": {key: value}}} of one assembly file."""
    lines = text.splitlines()
    label_at = {}
    for i, l in enumerate(lines):
        if l[:1] not in ("", "\t", " ", ";", ".") and ":" in l:
            label_at.setdefault(l.split(":", 1)[0], i)
    out = {}
    for i, l in enumerate(lines):
        m = _DESC.match(l)
        if not m or m.group(1) not in label_at:
            continue
        name = m.group(1)
        body = [c for c in (_code(x) for x in lines[label_at[name] + 1:i]) if c]
        info = {}
        j = i
        while j < len(lines) and not lines[j].startswith("; Kernel info:"):
            j += 1
        for x in lines[j + 1:]:
            if not x.startswith(";"):
                break
            k, _, v = x[1:].partition(":")
            info[k.strip()] = v.split()[0] if v.split() else ""
        out[name] = {"body": body, "insts": sum(1 for c in body if not c.startswith(".") and not c.endswith(":")), "info": info}
    # the metadata's spill counts: a list of maps, each with its .name
    entry = {}
    for l in lines[label_at.get("amdhsa.kernels", len(lines)):]:
        s = l.strip()
        if l.startswith("  - ."):  # (a kernel's map; the arguments' maps lie deeper)
            if entry.get(".name") in out:
                out[entry[".name"]]["info"].update(entry)
            entry = {}
            s = s[2:]
        if s.startswith(".") and ":" in s:
            k, _, v = s.partition(":")
            if k in (".name", ".sgpr_spill_count", ".vgpr_spill_count"):
                entry[k] = v.strip()
    if entry.get(".name") in out:
        out[entry[".name"]]["info"].update(entry)
    return out


def compare(old, new):
    """(identical, differing, new, vanished): lists of kernel names."""
    same = [k for k in old if k in new and old[k]["body"] == new[k]["body"] and _row(old[k]) == _row(new[k])]
    differ = [k for k in old if k in new and k not in set(same)]
    return same, differ, [k for k in new if k not in old], [k for k in old if k not in new]


def _row(kern):
    return [kern["info"].get(key, "?") for _, key in INFO]


def report(old, new, out=sys.stdout):
    same, differ, fresh, gone = compare(old, new)
    print("kernels: %d identical, %d differing, %d new, %d vanished" % (len(same), len(differ), len(fresh), len(gone)), file=out)
    for k in differ:
        print("differs: %s" % k, file=out)
        print("  %-12s %10s %10s" % ("", "old", "new"), file=out)
        print("  %-12s %10d %10d" % ("instructions", old[k]["insts"], new[k]["insts"]), file=out)
        for (title, _), a, b in zip(INFO, _row(old[k]), _row(new[k])):
            print("  %-12s %10s %10s%s" % (title, a, b, "" if a == b else "   <--"), file=out)
    for k in fresh:
        print("new: %s" % k, file=out)
        print("  %-12s %10d" % ("instructions", new[k]["insts"]), file=out)
        for (title, _), b in zip(INFO, _row(new[k])):
            print("  %-12s %10s" % (title, b), file=out)
    for k in gone:
        print("vanished: %s" % k, file=out)
    return 1 if differ or gone else 0


def assemble(tree, hip, out_path):
    sys.path.insert(0, ROOT)
    from gravit_amd._build import FLAGS, hipcc
    src = os.path.join(tree, "gravit_amd", "csrc", hip)
    return subprocess.Popen([hipcc()] + FLAGS + ["--offload-device-only", "-S", src, "-o", out_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", action="store_true", help="OLD and NEW are ready .s files")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files here")
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("hip", nargs="*", help=".hip files under gravit_amd/csrc")
    a = ap.parse_args(argv)
    if a.asm:
        return report(parse(open(a.old).read()), parse(open(a.new).read()))
    if not a.hip:
        ap.error("name at least one .hip file, or give two .s files with --asm")
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        for hip in a.hip:
            paths = [os.path.join(d, "%s.%s.s" % (os.path.splitext(hip)[0], side)) for side in ("old", "new")]
            procs = [assemble(t, hip, p) for t, p in zip((a.old, a.new), paths)]
            for p in procs:
                log, _ = p.communicate()
                if p.returncode:
                    sys.exit("hipcc failed on %s:\n%s" % (hip, log.decode(errors="replace")))
            print("== %s" % hip)
            rc |= report(parse(open(paths[0]).read()), parse(open(paths[1]).read()))
    return rc


if __name__ == "__main__":
    sys.exit(main())
