"""Writes zero_poly_known.json: the known answer of the reference's zero_poly_known test
(kzg-bench/src/tests/zero_poly.rs:7-50) as data — the EXISTS mask and the 2 x 16 expected field elements (canonical
integers, as hex strings), nothing else.

    python tests/golden/make_zero_poly_known.py <path to kzg-bench/src/tests/zero_poly.rs>

The numbers are read out of the three constant tables of that file; the generator checks them before it writes:
with w the primitive 16th root of unity the product of (X - w^i) over the missing indices is the polynomial, its
transform is the evaluation, and the evaluation is zero exactly on the missing indices."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def table(src, name):
    body = re.search(r"const %s\b[^=]*=\s*\[(.*?)\];" % name, src, flags=re.S).group(1)
    return body


def main(path):
    import fk20_model as FM

    src = open(path).read()
    exists = [w == "true" for w in re.findall(r"\b(true|false)\b", table(src, "EXISTS"))]
    rows = {}
    for name in ("EXPECTED_EVAL_U64", "EXPECTED_POLY_U64"):
        limbs = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})", table(src, name))]
        assert len(limbs) == 64, name
        rows[name] = [sum(limbs[4 * i + k] << (64 * k) for k in range(4)) for i in range(16)]
    assert len(exists) == 16
    R, w = FM.R, FM.root_of_order(16)
    poly = [1]
    for i, e in enumerate(exists):
        if not e:
            r = pow(w, i, R)
            poly = [((poly[j - 1] if j else 0) - r * (poly[j] if j < len(poly) else 0)) % R for j in range(len(poly) + 1)]
    poly += [0] * (16 - len(poly))
    assert poly == rows["EXPECTED_POLY_U64"]
    assert FM.fft(poly, w) == rows["EXPECTED_EVAL_U64"]
    assert [v == 0 for v in rows["EXPECTED_EVAL_U64"]] == [not e for e in exists]
    out = {"source": "kzg-bench/src/tests/zero_poly.rs:7-50", "exists": exists,
           "expected_eval": ["%064x" % v for v in rows["EXPECTED_EVAL_U64"]],
           "expected_poly": ["%064x" % v for v in rows["EXPECTED_POLY_U64"]]}
    with open(os.path.join(HERE, "zero_poly_known.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
