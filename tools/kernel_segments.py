"""Static figures of one kernel's text, cut at its workgroup barriers: python tools/kernel_segments.py <file.s> [kernel name part]

<file.s> is a device-only -S compile with the flags of tools/kernel_regs.sh (same hipcc line, `-S -o file.s` in place of `-c -o`).
The kernel is the one whose mangled name contains every '+'-separated piece of the name part (default: the narrow lean step
kernel).  Per segment (entry -> first s_barrier, ..., last s_barrier -> end) and for the whole kernel: instructions, v_writelane,
v_readlane, s_load (the kernel-argument loads are the ones on s[0:1] at entry; all scalar loads are counted), s_nop, s_waitcnt,
global loads and global stores.  Also the 1-based position, among the kernel's instructions, of the first and last global load
and the first LDS store of the first segment, and what scalar loads and v_writelanes stand before the first global load.
It reads text only; no GPU."""
import re
import sys

NARROW = "env_kernelILi511ELb0ELb0ELb0ELi256ELb1EE"
COLS = ("v_writelane", "v_readlane", "s_load", "s_nop", "s_waitcnt", "global_load", "global_store")


def kernel_text(path, parts):
    """The instruction lines of the kernel whose label contains all of `parts`."""
    lines, inside = [], False
    for line in open(path):
        s = line.split(";")[0].strip()
        if not inside:
            if s.endswith(":") and not s.startswith(".") and all(p in s for p in parts):
                inside = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        lines.append(s)
    return lines


def main():
    path = sys.argv[1]
    parts = (sys.argv[2] if len(sys.argv) > 2 else NARROW).split("+")
    ins = kernel_text(path, parts)
    if not ins:
        sys.exit("no kernel matches %s" % parts)
    cuts = [i for i, s in enumerate(ins) if s.startswith("s_barrier")]
    bounds = [0] + [c + 1 for c in cuts] + [len(ins)]
    print("%-22s %6s " % ("segment", "instr") + " ".join("%11s" % c for c in COLS))

    def row(name, seg):
        print("%-22s %6d " % (name, len(seg)) + " ".join("%11d" % sum(1 for s in seg if s.startswith(c)) for c in COLS))

    for k in range(len(bounds) - 1):
        name = "entry -> barrier 1" if k == 0 else ("barrier %d -> end" % k if k == len(bounds) - 2 else "barrier %d -> %d" % (k, k + 1))
        row(name, ins[bounds[k]:bounds[k + 1]])
    row("whole kernel", ins)
    first = ins[:bounds[1]]
    gl = [i + 1 for i, s in enumerate(first) if s.startswith("global_load")]
    ds = [i + 1 for i, s in enumerate(first) if s.startswith("ds_write")]
    print("first segment: global loads at instructions %s; first LDS store at %s" % (gl, ds[0] if ds else None))
    if gl:
        head = first[:gl[0] - 1]
        print("before the first global load: %d v_writelane, scalar loads:" % sum(1 for s in head if s.startswith("v_writelane")))
        for s in head:
            if s.startswith("s_load"):
                print("   ", s)


if __name__ == "__main__":
    main()
