"""Compare the gfx950 ISA of kernels between two `hipcc -S --cuda-device-only` outputs (a check that
a source refactoring left a tuned kernel's code untouched).  usage: isa_diff.py old.s new.s [filter]
A kernel of old.s is matched to the kernel of new.s whose mangled name is equal, or equal after
`--map OLD=NEW` substring substitutions.  A kernel's code runs from its label to the end of the
function and includes its `.amdhsa_*` descriptor (registers, LDS).  Basic-block labels are compared
without the function's number (`.LBB<fn>_<n>` -> `.LBB_<n>`), which moves with the order in which
the instantiations are emitted.  Exit status 0 only when every kernel is IDENTICAL and both files
hold the same kernels."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = []
        for ln in m.group(2).split("\n"):
            ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln.split(";")[0].strip())
            if ln and (not ln.startswith(".") or ln.startswith((".LBB_", ".amdhsa_"))):
                body.append(ln)
        out[m.group(1)] = body
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--map")]
    maps = [a.split("=", 1) for a in sys.argv[1:] if a.startswith("--map") for a in [a[6:]]]
    old, new = kernels(args[0]), kernels(args[1])
    flt = args[2] if len(args) > 2 else ""
    ok, matched = True, set()
    for name, body in old.items():
        if flt not in name:
            continue
        other = name
        for a, b in maps:
            other = other.replace(a, b)
        if other not in new:
            print(f"{name[:90]}: no counterpart")
            ok = False
            continue
        matched.add(other)
        nb = new[other]
        diff = sum(1 for x, y in zip(body, nb) if x != y) + abs(len(body) - len(nb))
        print(f"{name[:90]}: {len(body)} / {len(nb)} lines, "
              + ("IDENTICAL" if body == nb else f"{diff} lines differ"))
        ok = ok and body == nb
    for name in new:
        if flt in name and name not in matched:
            print(f"{name[:90]}: only in {args[1]}")
            ok = False
    print(f"{len(matched)} kernels compared: " + ("all IDENTICAL, same kernel sets" if ok else "DIFFERENT"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
