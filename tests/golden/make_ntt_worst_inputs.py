"""Writes tests/golden/ntt_worst_inputs.json: inputs that drive the lazy values of the Fr transforms towards their bound,
built by tests/ntt_lazy_model.py (build_all: about a hundred small model runs, a few seconds).  The tests read the file
and never search.  Run from the repository root:  python tests/golden/make_ntt_worst_inputs.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ntt_lazy_model as M  # noqa: E402

if __name__ == "__main__":
    vectors = M.build_all()
    with open(os.path.join(HERE, "ntt_worst_inputs.json"), "w") as f:
        json.dump({"r": "%x" % M.R, "vectors": vectors}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for v in vectors:
        print("%-28s %s" % (v["name"], " ".join("%.2fr" % (int(x, 16) / M.R) for x in v["reached"][:8])))
