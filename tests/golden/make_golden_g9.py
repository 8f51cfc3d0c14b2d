"""Generates tests/golden/g9_softssv_reference.npz: the REFERENCE's softSsv on random int8 models and symbol strings.

Run in the build container only (needs /root/reference):

    make -C oracle _ref && python tests/golden/make_golden_g9.py

The answers come from oracle/_ref/libsoftssv_ref.so, the reference's test/softSsv/SoftSsv.cpp compiled from where it
lies (oracle/Makefile).  tests/test_oracle.py checks the restatement against them on every box; where oracle/_ref
exists it also checks the live reference against them.

Case k: model_k [rows,4] int8, symbols_k uint8 (0..3), hits_k the packed records in device order; and raw_rows /
raw_cols, the reference's own emission order for one small case (rows ascending, columns descending).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

NCASES = 12


def main():
    from oracle import pyoracle as O
    O.build()
    if not O.ref_available():
        sys.exit("oracle/_ref/libsoftssv_ref.so is not built (make -C oracle _ref needs the reference tree)")
    rng = np.random.default_rng(11)
    arrays = {"ncases": np.array(NCASES)}
    for k in range(NCASES):
        nrows, n = int(rng.integers(1, 300)), int(rng.integers(1, 4000))
        model = rng.integers(-128, 128, size=(nrows, 4)).astype(np.int8)
        sym = rng.integers(0, 4, size=n, dtype=np.uint8)
        hits = O.ssv_reference(sym, model)
        assert np.array_equal(hits, O.ssv(sym, model))
        arrays[f"model_{k}"], arrays[f"symbols_{k}"], arrays[f"hits_{k}"] = model, sym, hits
    rows, cols = O.ssv_reference_raw(np.zeros(5, np.uint8), np.full((3, 4), 127, np.int8))
    arrays["raw_rows"], arrays["raw_cols"] = np.asarray(rows, np.uint64), np.asarray(cols, np.uint64)
    path = os.path.join(OUT, "g9_softssv_reference.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", sum(arrays[f"hits_{k}"].size for k in range(NCASES)), "hits")


if __name__ == "__main__":
    main()
