"""Source channels for the multi-channel tests (tests/test_gpu_channels.py,
tests/test_channels_cpu.py), built from a case's own source f:

    ch0 = f, ch1 = f reversed along every axis (a different field on the same grid),
    ch2 = all zeros, ch3 = -f.
"""
import numpy as np

DIRICHLET_VALUES = (1.0, 0.0, -2.0, 0.5)


def channels(f, c):
    f = np.ascontiguousarray(f, np.float32)
    rev = np.ascontiguousarray(f[tuple(slice(None, None, -1) for _ in f.shape)])
    return np.ascontiguousarray(np.stack([f, rev, np.zeros_like(f), -f])[:c])


def eq_bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)
