#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libcocytus_ec.so, instruction for instruction.

    python tools/kernel_isa_diff.py OLD.so [NEW.so]      (NEW defaults to the in-tree library)

Disassembles both code objects (ec.kernel_disassembly: llvm-objdump, addresses and encodings
dropped) and prints, as one JSON line, which kernels are identical, which changed, and which
exist in one build only.  Exit status 1 if a kernel of OLD changed or is gone: a pull request
that adds a kernel shows with it that every existing kernel is the parent's.  Loads nothing
and needs no GPU.
"""
from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    from cocytus_amd import ec

    if len(sys.argv) not in (2, 3):
        print(__doc__, file=sys.stderr)
        return 2
    old, new = ec.kernel_disassembly(sys.argv[1]), ec.kernel_disassembly(sys.argv[2] if len(sys.argv) > 2 else None)
    if old is None or new is None:
        print("cannot disassemble (missing file or llvm-objdump)", file=sys.stderr)
        return 2
    changed = sorted(n for n in old if n in new and old[n] != new[n])
    removed = sorted(set(old) - set(new))
    print(json.dumps({"tool": "kernel_isa_diff", "kernels_old": len(old), "kernels_new": len(new),
                      "identical": len(old) - len(changed) - len(removed), "changed": changed,
                      "removed": removed, "added": sorted(set(new) - set(old)),
                      "kernel_code_id_old": ec.kernel_code_id(sys.argv[1]),
                      "kernel_code_id_new": ec.kernel_code_id(sys.argv[2] if len(sys.argv) > 2 else None)}))
    return 1 if changed or removed else 0


if __name__ == "__main__":
    sys.exit(main())
