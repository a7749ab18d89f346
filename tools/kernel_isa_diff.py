#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library, instruction by instruction:

    python tools/kernel_isa_diff.py graph-neural-mapping_amd/lib/variants/parent.so graph-neural-mapping_amd/lib/libgnm_hip.so

Each build (.so or .o) is unbundled with `llvm-objdump --offloading` and its code objects are disassembled; the
instruction lines are grouped by kernel symbol, without addresses, encodings or the padding between kernels.  Prints one
line per kernel -- same / differs / only in A / only in B -- and the totals; the exit status is 0 only when every kernel
of A is in B with the same instruction stream.  The check of a refactor that must leave the device code as it was."""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"        # as tests/test_isa_hazards.py


def kernels(path):
    """{symbol: [instruction lines]} of every gfx950 code object bundled in `path`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = shutil.copy(path, tmp)            # --offloading extracts the bundles NEXT to the file it is given
        subprocess.run([OBJDUMP, "--offloading", copy], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
        objs = sorted(glob.glob(copy + ".*gfx950"))
        if not objs:
            raise SystemExit("no gfx950 code object inside %s" % path)
        for o in objs:
            asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", o], check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            cur = None
            for line in asm.splitlines():
                if line.startswith("<") and line.endswith(">:"):
                    cur = out.setdefault(line[1:-2], [])
                    continue
                ins = line.split("//")[0].strip()
                if cur is not None and ins and ins != "...":
                    cur.append(ins)
    for ins in out.values():                     # the alignment fill behind a kernel's last s_endpgm is padding too
        while ins and ins[-1] == "s_nop 0":
            ins.pop()
    return out


def compare(a, b):
    """(report lines, all of A the same in B)"""
    lines, counts = [], {"same": 0, "differs": 0, "only in A": 0, "only in B": 0}
    for name in sorted(set(a) | set(b)):
        if name not in b or name not in a:
            verdict = "only in A" if name in a else "only in B"
            lines.append("%-10s %s" % (verdict, name))
        elif a[name] == b[name]:
            verdict = "same"
            lines.append("%-10s %s (%d instructions)" % (verdict, name, len(a[name])))
        else:
            verdict = "differs"
            n = min(len(a[name]), len(b[name]))
            first = next((i for i in range(n) if a[name][i] != b[name][i]), n)
            at = lambda k: k[name][first] if first < len(k[name]) else "<end>"
            lines.append("%-10s %s (instruction %d: `%s` | `%s`; %d | %d instructions)"
                         % (verdict, name, first, at(a), at(b), len(a[name]), len(b[name])))
        counts[verdict] += 1
    lines.append("kernels: %d in A, %d in B; " % (len(a), len(b)) + ", ".join("%d %s" % (counts[k], k) for k in counts))
    return lines, counts["differs"] == 0 and counts["only in A"] == 0


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    lines, ok = compare(kernels(sys.argv[1]), kernels(sys.argv[2]))
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
