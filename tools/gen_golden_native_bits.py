"""Writes tests/golden/native_bits.json on the MI355X: SHA-256 hashes of the inputs and of every output array of the native
encode, decode, vanilla pull-back and LPIPS for the cases of tests/native_bits_cases.py, and the *_workspace_bytes answers for
its WORKSPACE_N.  The file pins the bits of the build it was written with: run it at the commit whose outputs are the
reference (the last one before a change that must keep them), then test_gpu_native_bits.py and test_native_bits_host.py hold
every later build to it.

    python tools/gen_golden_native_bits.py        (needs the GPU and the built library)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import native_bits_cases as NB  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "native_bits.json")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("gen_golden_native_bits.py records device outputs; no GPU here")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0), "workspace_n": list(NB.WORKSPACE_N), "cases": {}, "workspace_bytes": {}}
    for area, name in NB.ALL:
        doc["cases"].update(NB.run(area, name, dev))
        doc["workspace_bytes"][f"{area}/{name}"] = NB.workspace_answers(area, name)
        print(area, name, "ok", flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
