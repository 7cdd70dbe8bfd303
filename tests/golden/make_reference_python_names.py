#!/usr/bin/env python3
"""Generates tests/golden/reference_python_names.json: for each of the reference's own Python examples, the dotted
names it reads from `teaserpp_python`, from the solver object (`solver.X`, `teaser_solver.X`) and from the solver
parameters (`solver_params.X`).  Only the names are stored, no program text, so tests/test_python_shim.py checks
them without the reference tree.

Run from the repo root:  python tests/golden/make_reference_python_names.py <reference checkout>
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EXAMPLES = ["python/teaserpp_python/teaserpp_example.py",
            "examples/teaser_python_ply/teaser_python_ply.py",
            "examples/teaser_python_fpfh_icp/example.py",
            "examples/teaser_python_fpfh_icp/helpers.py",
            "examples/teaser_python_3dsmooth/teaser_python_3dsmooth.py"]
HEADS = ("teaserpp_python", "solver", "teaser_solver", "solver_params")


def attribute_chains(tree):
    """Dotted names read in the file: 'teaserpp_python.X.Y' and 'solver.attr' style chains."""
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            parts, cur = [], node
            while isinstance(cur, ast.Attribute):
                parts.append(cur.attr)
                cur = cur.value
            if isinstance(cur, ast.Name):
                out.add((cur.id,) + tuple(reversed(parts)))
    return out


def main(reference):
    doc = {}
    for rel in EXAMPLES:
        tree = ast.parse(open(os.path.join(reference, rel)).read())
        doc[rel] = sorted(list(c) for c in attribute_chains(tree) if c[0] in HEADS)
    with open(os.path.join(ROOT, "tests", "golden", "reference_python_names.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
