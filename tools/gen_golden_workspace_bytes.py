"""Writes tests/golden/workspace_bytes.json: what the *_workspace_bytes queries of the graph-build, clustering and
shortest-path sources answer on the grid of tests/workspace_bytes_cases.py, once per setting of the knn_filter option for the
queries that read it.  Host arithmetic only: no GPU is touched.  The file pins the answers of the library it is given: build
the commit whose answers are the reference (the last one before a change that must keep them) in a separate worktree and pass
its library, then test_workspace_bytes_host.py holds every later build to it.

    python tools/gen_golden_workspace_bytes.py /path/to/reference/vqvae_amd/libgeo_hip.so
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import workspace_bytes_cases as W  # noqa: E402
from vqvae_amd import _lib  # noqa: E402  (the signatures only: the library loaded is the one named on the command line)

OUT = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    L = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    for name in {n for n, _ in W.common_cases() + W.knn_cases()} | {"geo_set_option", "geo_version"}:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    doc = {"geo_version": int(L.geo_version())}
    doc.update(W.sizes(L))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in doc["common"].values()) + sum(len(v) for s in doc["knn_filter"].values() for v in s.values())
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", n, "answers")


if __name__ == "__main__":
    main()
