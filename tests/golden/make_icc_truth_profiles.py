#!/usr/bin/env python3
"""Generates tests/golden/icc_truth_profiles.npz with the REAL Little CMS 2 (oracle/liboracle_icc.so, oracle_icc_make_profile): the
bytes of the document profiles of tests/test_gpu_icc.py -- the six PROFILES, the three SAMPLED and the three MIXED -- and nothing
else.  The fixture lets tests/test_truth64_icc.py and tests/test_gpu_icc_determined.py run where lcms2 is absent: the float64 truth
(tests/truth64.py) needs the prepared transform only, and the library prepares that from the profile bytes."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import icc_profiles
    L = icc_profiles.lcms()
    assert L is not None, "oracle/liboracle_icc.so is not built"
    out = {name: np.frombuffer(icc_profiles.make_profile(L, name), dtype=np.uint8) for name in icc_profiles.SPECS}
    np.savez_compressed(os.path.join(HERE, "icc_truth_profiles.npz"), **out)
    print("written", len(out), "profiles,", sum(v.nbytes for v in out.values()), "bytes")


if __name__ == "__main__":
    main()
