#!/usr/bin/env python3
"""Generates tests/golden/pq_exponent_fields_codes.npz ON A GPU, from the library the package loads (AVIFGPU_LIB or the tree's): the
codes every close-form PQ kernel gives the exponent-field sweep of tests/pq_exponent_fields.py, one (7 680, channels) uint16 array
per form and depth ("hot_pxl8_b10", ...).

The committed fixture was recorded from the build BEFORE the exponent tables lost their sign half (512 entries, the sign bit part of
the index): tests/test_zzzzzz_gpu_pq_half_table.py holds the 256-entry tables to those codes.  Run it again only from a build whose codes
are meant to become the new record."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import pq_exponent_fields as pf
    gpu = pf.pkg.AvifGpu(0)
    out = {}
    for bits in pf.DEPTHS:
        for form in pf.FORMS:
            codes = pf.run(gpu, form, bits)
            assert codes.min() >= 0 and codes.max() < (1 << bits), (form[0], bits, "a sample nothing wrote, or out of range")
            out[f"{form[0]}_b{bits}"] = codes.astype(np.uint16)
    np.savez_compressed(os.path.join(HERE, "pq_exponent_fields_codes.npz"), **out)
    print("written", len(out), "arrays from", pf.pkg.LIB_PATH)


if __name__ == "__main__":
    main()
