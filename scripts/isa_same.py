"""Which kernels of two ISA listings (make isa) are the same instruction for instruction:
    python scripts/isa_same.py parent.s change.s [more pairs ...]

Kernel bodies are compared as text, comments dropped and the function number taken out of local labels
(.LBB<function>_<block>: a kernel added to the file renumbers the functions after it)."""
import re
import sys


def bodies(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end", s, re.S | re.M):
        lines = []
        for l in m.group(2).split("\n"):
            l = l.split(";")[0].rstrip()
            if not l or l.startswith("\t."):
                continue
            lines.append(re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", l))
        out[m.group(1)] = "\n".join(lines)
    return out


def main():
    print("Kernel bodies of the parent's and the change's ISA listings (make isa), compared as text:")
    for a, b in zip(sys.argv[1::2], sys.argv[2::2]):
        pa, pb = bodies(a), bodies(b)
        rows = []
        for name in sorted(set(pa) | set(pb)):
            what = "same" if pa.get(name) == pb.get(name) else ("changed" if name in pa and name in pb else
                                                                ("new" if name in pb else "gone"))
            rows.append((what, name))
        print("%s identical: %d changed: %d new: %d gone: %d" % (
            b.split("/")[-1], *(sum(1 for w, _ in rows if w == k) for k in ("same", "changed", "new", "gone"))))
        for k in ("same", "changed", "new", "gone"):
            for w, name in rows:
                if w == k:
                    print("  %-7s %s" % (w, name))


if __name__ == "__main__":
    main()
