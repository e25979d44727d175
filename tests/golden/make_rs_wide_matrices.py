"""Generate tests/golden/rs_wide_matrices.json: the coding matrices of the large geometries of the
wide Reed-Solomon coder (dm_rs_create_wide), as digests.

``oracle.py_rs_matrix`` (pure-Python GF(2^8) arithmetic, no log tables) takes 12 s at 128 + 128
and over a minute at 255 + 1, too slow inside a test, so its results are pinned here once: for
each geometry the SHA-256 of the (data + parity) x data matrix, row-major, and its first parity
row in hex.  Restatement-pinned like rs_golden.json: klauspost/reedsolomon is not vendored.

Run: python tests/golden/make_rs_wide_matrices.py   (a few minutes)
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from oracle import py_rs_matrix  # noqa: E402

OUT = os.path.join(HERE, "rs_wide_matrices.json")
GEOMETRIES = [(128, 128), (200, 56), (255, 1), (1, 255)]


def main() -> None:
    matrices = []
    for k, m in GEOMETRIES:
        rows = py_rs_matrix(k, k + m)
        assert len(rows) == k + m and all(len(r) == k for r in rows)
        raw = b"".join(bytes(r) for r in rows)
        matrices.append({"data": k, "parity": m, "sha256": hashlib.sha256(raw).hexdigest(),
                         "first_parity_row": bytes(rows[k]).hex()})
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_rs_wide_matrices.py", "matrices": matrices}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
