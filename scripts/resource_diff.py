#!/usr/bin/env python3
"""Compare two compiler resource reports of one source file, kernel by kernel.

  hipcc <the product flags> --offload-device-only -Rpass-analysis=kernel-resource-usage -c csrc/pt_wave.hip \
        -o /dev/null 2> report.txt            (once per commit)
  scripts/resource_diff.py parent.txt change.txt

Prints, per kernel (demangled with c++filt when it is there), VGPRs, SGPRs, SGPR and VGPR spills, scratch bytes per
lane and occupancy of both reports, and marks the kernels that differ.  Exit status 1 when a kernel gained scratch or
a kernel of one report is missing from the other."""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("SGPRs", "TotalSGPRs"), ("sspill", "SGPRs Spill"), ("vspill", "VGPRs Spill"),
          ("scratch", "ScratchSize [bytes/lane]"), ("occ", "Occupancy [waves/SIMD]"))


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name is not None:
            out[name][key] = val
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(s):
    s = re.sub(r"\(pt::WfArgs const\*.*$", "", s)
    return s.replace("pt::", "").replace("void ", "")


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    bad = 0
    print("%-60s %s" % ("kernel (parent -> change)", "  ".join("%-9s" % f for f, _ in FIELDS)))
    for n in names:
        if n not in a or n not in b:
            print("%-60s only in %s" % (short(pretty[n]), "parent" if n in a else "change"))
            bad = 1
            continue
        cells, diff = [], False
        for _, key in FIELDS:
            x, y = a[n].get(key, "?"), b[n].get(key, "?")
            diff |= x != y
            cells.append("%-9s" % (x if x == y else "%s->%s" % (x, y)))
        if int(b[n].get("ScratchSize [bytes/lane]", 0)) > int(a[n].get("ScratchSize [bytes/lane]", 0)):
            bad = 1
        print("%-60s %s%s" % (short(pretty[n])[:60], "  ".join(cells), "   *" if diff else ""))
    return bad


if __name__ == "__main__":
    sys.exit(main())
