"""The reference's own hydro.yaml parser, answered once and stored: tests/golden/hydro_yaml_reference.json.

For every hand-written case of tests/test_hydro_yaml.py (CASES) and every *.hydro.yaml the reference tree ships (stored with its text,
at its path relative to the tree), the flat key=value dump of oracle/_ref/libref_yaml.so (oracle/Makefile `ref`: the reference's
src/hydro_yaml_parser.cpp plus oracle/ref_yaml_shim.cpp) or its error message.  The parser resolves h5_file against the directory of
the file it reads, so every document is parsed below a scratch directory whose real path is stored as "{base}"; the tests put their
own directory back in.  tests/test_hydro_yaml.py and tests/test_host_sanitizers.py read this file, so neither needs the reference.

Run where the reference tree and oracle/_ref are present:  python tests/golden/make_yaml_goldens.py REFERENCE_ROOT
"""
import ctypes as C
import glob
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_yaml.so")
DST = os.path.join(HERE, "hydro_yaml_reference.json")


def dump(lib, path, base):
    st = C.c_int()
    text = lib.ref_yaml_dump(path.encode(), C.byref(st)).decode()
    return {"ok": st.value == 0, "dump": text.replace(os.path.realpath(base), "{base}")}


def parse_below(lib, rel, text):
    """Writes `text` to <scratch>/<rel> (bytes as given: CRLF stays CRLF) and parses it there."""
    with tempfile.TemporaryDirectory() as base:
        path = os.path.join(base, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as fh:
            fh.write(text.encode())
        return dump(lib, path, base)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = os.path.abspath(sys.argv[1])
    lib = C.CDLL(REF_LIB)
    lib.ref_yaml_dump.restype = C.c_char_p
    sys.path.insert(0, os.path.dirname(HERE))
    from test_hydro_yaml import CASES, case_path
    out = {"generated_by": "tests/golden/make_yaml_goldens.py", "hand_written": {}, "reference_files": {}}
    for name, text in sorted(CASES.items()):
        out["hand_written"][name] = dict(text=text, **parse_below(lib, case_path(name), text))
    for f in sorted(glob.glob(os.path.join(ref_root, "**", "*.hydro.yaml"), recursive=True)):
        rel = os.path.relpath(f, ref_root)
        text = open(f, newline="").read()
        out["reference_files"][rel] = dict(text=text, **parse_below(lib, rel, text))
    with open(DST, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{DST}: {len(out['hand_written'])} hand-written cases, {len(out['reference_files'])} reference files")


if __name__ == "__main__":
    main()
