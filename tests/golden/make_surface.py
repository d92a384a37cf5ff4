"""Regenerate tests/golden/reference_surface.json: the names of the public
methods the reference's ORBextractor and ORBmatcher classes declare
(include/ORBextractor.h, include/ORBmatcher.h), the list that
tests/test_shim.py::test_shim_declares_reference_surface holds the drop-in
shim's headers to. Names only; no text of the headers is stored.

    python tests/golden/make_surface.py <reference checkout>/include
"""
import json
import os
import re
import sys

HEADERS = {"ORBextractor.h": "ORBextractor", "ORBmatcher.h": "ORBmatcher"}
NAMES = r"\b(ORBextractor|ORBmatcher|operator\(\)|Get\w+|Search\w+|Fuse|DescriptorDistance)\s*\("


def methods(text, cls):
    """Method names declared from `class cls {` on (the same expression the test applies to the shim)."""
    body = text[re.search(rf"class\s+{cls}\s*\{{", text).start():]
    return set(re.findall(NAMES, body))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    out = {}
    for name, cls in HEADERS.items():
        with open(os.path.join(sys.argv[1], name), encoding="utf-8", errors="replace") as f:
            out[name] = {"class": cls, "methods": sorted(methods(f.read(), cls))}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_surface.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")


if __name__ == "__main__":
    main()
