"""Writes tests/golden/workspace_bytes.json: what the *_workspace_bytes queries of the graph-build, clustering,
shortest-path and model-side sources answer on the grid of tests/workspace_bytes_cases.py, once per setting of the knn_filter
option for the queries that read it and once per setting of the decoder JVP's route options for its queries and for the route
codes of geo_jvp_plan_part (those settings are kept as what they change against the defaults: pack_model).  Host arithmetic
only: no GPU is touched.  The file pins the answers of the library it is given: build the commit whose answers are the
reference (the last one before a change that must keep them) in a separate worktree and pass its library, then
test_workspace_bytes_host.py holds every later build to it.

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


def dump(doc):
    """One key or answer per line; the model side's lists of answers one list per line."""
    model = doc.pop("model")
    text = json.dumps(doc, indent=0, sort_keys=True)[:-2] + ',\n"model": {\n'
    settings = []
    for setting in sorted(model):
        queries = []
        for q in sorted(model[setting]):
            lists = ",\n".join(f"{json.dumps(d)}: {json.dumps(v, separators=(',', ':'))}" for d, v in sorted(model[setting][q].items()))
            queries.append(f"{json.dumps(q)}: {{\n{lists}\n}}")
        settings.append(f"{json.dumps(setting)}: {{\n" + ",\n".join(queries) + "\n}")
    doc["model"] = model
    return text + ",\n".join(settings) + "\n}\n}\n"


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    L = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    for name in {n for n, _ in W.common_cases() + W.knn_cases()} | W.model_queries() | {"geo_set_option", "geo_version"}:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    doc = {"geo_version": int(L.geo_version())}
    doc.update(W.sizes(L))
    doc["model"] = W.pack_model(doc["model"])
    with open(OUT, "w") as f:
        f.write(dump(doc))
    n = sum(len(v) for v in doc["common"].values()) + sum(len(v) for s in doc["knn_filter"].values() for v in s.values())
    n += sum(len(a) for setting in W.unpack_model(doc["model"]).values() for by_desc in setting.values() for a in by_desc.values())
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", n, "answers")


if __name__ == "__main__":
    main()
