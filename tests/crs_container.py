"""The ZKCRSv2 container (zk_crs_save of an integer-roots CRS) read on the host: shared by the device tests that compare the three
Lagrange-basis arrays a CRS carries with a model's."""
import numpy as np


def read_v2(path, n):
    """(header fields, v1 payload bytes, dict of the three Lagrange-basis arrays) of a ZKCRSv2 file"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"ZKCRSv2\0"
    tail = 8 * (8 * n + 8 * (n - 1) + 16 * n)
    body = np.frombuffer(raw[len(raw) - tail:], dtype=np.uint64)
    lag = dict(lag1=body[:8 * n].reshape(n, 8).copy(), lagS_t1=body[8 * n:8 * n + 8 * (n - 1)].reshape(n - 1, 8).copy(),
               lag2=body[8 * n + 8 * (n - 1):].reshape(n, 16).copy())
    return raw[8:32], raw[40:len(raw) - tail], lag
