#!/usr/bin/env python3
"""Regenerate tests/golden/sphere_eta_record.txt: the first 8001 lines (t = 0 .. 120 s at 0.015 s) of the free-surface elevation
record that the reference's eta-import demo reads (demos/sphere/eta/eta.txt of a HydroChrono checkout), copied byte for byte.
The file is data ("time : eta" lines, IrregularWaves::ReadEtaFromFile's format); the tests read only the copy.

  python tests/golden/make_eta_fixture.py <HydroChrono checkout>
"""
import os
import sys

LINES = 8001
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sphere_eta_record.txt")


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(argv[1], "demos", "sphere", "eta", "eta.txt")
    with open(src, "rb") as f:
        lines = [f.readline() for _ in range(LINES)]
    if not lines[-1]:
        sys.exit(f"{src} has fewer than {LINES} lines")
    with open(OUT, "wb") as f:
        f.writelines(lines)
    print(f"wrote {OUT}: {LINES} lines, {sum(map(len, lines))} bytes")


if __name__ == "__main__":
    main(sys.argv)
