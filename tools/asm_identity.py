#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 device assembly files (DESIGN.md §13,
§15: "existing kernels must not change").

    hipcc $(HIPFLAGS) --offload-device-only -S file.hip -o before.s   # parent
    hipcc $(HIPFLAGS) --offload-device-only -S file.hip -o after.s    # this tree
    python tools/asm_identity.py before.s after.s

Where a file only GAINS kernels a whole-file diff cannot be empty, so the files
are cut into one piece per kernel: its code section with the kernel descriptor
and the resource symbols, and its entry in the code-object metadata.  What
is normalised is not code: the lines with the compilation unit id
(`__hip_cuid_`) are dropped; the function number in local labels (`.LBB12_3`,
`.Lfunc_end12`, `BB12_3` in loop comments), which counts the kernels emitted
before this one, is blanked; and the padding between a label and its comment,
which depends on how many digits that number has, is one space.  Exit status 0: every kernel of `before` is in `after` with
the same bytes (kernels only in `after` are listed); 1 otherwise.
"""
import re
import sys

_SEC = re.compile(r"^\t\.section\t\.text\.([^,]+),")
_LBL = re.compile(r"(\.LBB|\bBB|Lfunc_end|Lfunc_begin)\d+")
_PAD = re.compile(r" +;")
_NAME = re.compile(r"^\s+\.name:\s+(\S+)")


def pieces(path):
    """{kernel: (code lines, metadata lines)} of one assembly file"""
    code, meta, cur, entry = {}, {}, None, None
    in_meta = False
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            if line.startswith("\t.amdgpu_metadata"):
                in_meta, cur = True, None
                continue
            if in_meta:
                if line.startswith("  - ."):  # next kernel's entry
                    entry = []
                elif not line.startswith(" "):  # past the kernel list
                    entry = None
                if entry is not None:
                    entry.append(line)
                    m = _NAME.match(line)
                    if m:
                        meta[m.group(1)] = entry
                continue
            m = _SEC.match(line)
            if m:
                cur = m.group(1)
            elif line.startswith("\t.section\t.AMDGPU") or \
                    line.startswith("\t.text"):
                cur = None
            if cur is not None:
                code.setdefault(cur, []).append(
                    _PAD.sub(" ;", _LBL.sub(r"\1#", line)))
    return {k: (code[k], meta.get(k)) for k in code if k in meta}


def main(a, b):
    A, B = pieces(a), pieces(b)
    changed = [k for k in A if k in B and A[k] != B[k]]
    missing = [k for k in A if k not in B]
    added = [k for k in B if k not in A]
    print("%s: %d kernels, %s: %d kernels; identical %d, changed %d, "
          "missing %d, new %d" % (a, len(A), b, len(B),
                                  len(A) - len(changed) - len(missing),
                                  len(changed), len(missing), len(added)))
    for what, names in (("changed", changed), ("missing", missing)):
        for k in names[:16]:
            print(" ", what, k)
        if len(names) > 16:
            print("  ... and %d more" % (len(names) - 16))
    return 1 if changed or missing or not A else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
