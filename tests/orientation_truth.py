"""The definition of the oriented open (the table of include/avifgpu.h), as numpy on an (H, W, C) array: shared by the CPU and the GPU tests."""
import numpy as np


def orient(code, a):
    return {1: lambda: a, 2: lambda: a[:, ::-1], 3: lambda: a[::-1, ::-1], 4: lambda: a[::-1, :],
            5: lambda: a.transpose(1, 0, 2), 6: lambda: np.rot90(a, -1), 7: lambda: a[::-1, ::-1].transpose(1, 0, 2),
            8: lambda: np.rot90(a, 1)}[code]()
