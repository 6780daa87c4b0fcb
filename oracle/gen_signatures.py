#!/usr/bin/env python3
"""Record the parameter names and defaults of the reference's public entry points as a data fixture.

Usage (where a checkout of the reference exists; the suite itself only reads the fixture):

    python oracle/gen_signatures.py <reference checkout>/sageattention/core.py

Parses (never executes: the reference package cannot be imported without its compiled extension) every top-level
``sageattn*`` function of core.py and writes ``tests/golden/reference_signatures.json``:
``{name: {"params": [...], "defaults": [...], "kwarg": name or null}}``, with ``defaults`` aligned to ``params``
(null where a parameter has no default, as tests/test_import_dropin.py compares them).
"""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reference_signatures.json")


def signatures(core_py: str) -> dict:
    tree = ast.parse(open(core_py).read())
    want = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name.startswith("sageattn"):
            args = node.args
            names = [a.arg for a in args.args]
            defaults = [None] * (len(names) - len(args.defaults)) + [ast.literal_eval(d) for d in args.defaults]
            want[node.name] = {"params": names, "defaults": defaults, "kwarg": args.kwarg.arg if args.kwarg else None}
    return want


if __name__ == "__main__":
    sigs = signatures(sys.argv[1])
    with open(OUT, "w") as f:
        json.dump(sigs, f, indent=1)
        f.write("\n")
    print(f"wrote {len(sigs)} signatures to {os.path.normpath(OUT)}")
