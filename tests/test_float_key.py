"""CPU check of the ordered float keys (envgs_amd/csrc/float_key.h): the header is host + device code shared by the radix selects, the
densification plan and this test, which compiles it into a tiny host library with g++ and runs the three functions over a fixed list of
edge values and 10^5 seeded random bit patterns (no NaNs): both encoders are strictly monotone in the float order -- except that the
canonicalising one gives -0 and +0 the same key --, the decoder inverts the raw encoder bit for bit, and the canonical key of -0 decodes to +0."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "envgs_amd", "csrc", "float_key.h")

SRC = """
#include "%s"
extern "C" void fk_apply(const float *f, int n, uint32_t *raw, uint32_t *canon, float *back, float *back_canon)
{
    for (int i = 0; i < n; i++) {
        raw[i] = envgs::float_key(f[i]);
        canon[i] = envgs::float_key_canon(f[i]);
        back[i] = envgs::float_of_key(raw[i]);
        back_canon[i] = envgs::float_of_key(canon[i]);
    }
}
"""


@pytest.fixture(scope="module")
def fk():
    d = tempfile.mkdtemp(prefix="float_key_")
    src = os.path.join(d, "fk.cpp")
    with open(src, "w") as f:
        f.write(SRC % HDR)
    so = os.path.join(d, "libfk.so")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    pf, pu = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    lib.fk_apply.argtypes = [pf, ctypes.c_int, pu, pu, pf, pf]

    def apply(bits):
        f = np.ascontiguousarray(bits, np.uint32).view(np.float32)
        raw, canon = np.empty(f.size, np.uint32), np.empty(f.size, np.uint32)
        back, back_canon = np.empty(f.size, np.float32), np.empty(f.size, np.float32)
        lib.fk_apply(f.ctypes.data_as(pf), f.size, raw.ctypes.data_as(pu), canon.ctypes.data_as(pu), back.ctypes.data_as(pf),
                     back_canon.ctypes.data_as(pf))
        return raw, canon, back.view(np.uint32), back_canon.view(np.uint32)
    return apply


def _inputs():
    """Distinct non-NaN bit patterns in the float order, -0 directly before +0."""
    one = np.float32(1.0).view(np.uint32)
    mags = np.array([0x00000000, 0x00000001, 0x00800000, one - 1, one, one + 1, 0x7f7fffff, 0x7f800000], np.uint32)   # 0, denormal min, FLT_MIN,
    fixed = np.concatenate([mags, mags | np.uint32(0x80000000)])                                                        # 1 -+ 1 ulp, FLT_MAX, inf
    rnd = np.random.default_rng(20).integers(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32)
    bits = np.unique(np.concatenate([fixed, rnd]))
    bits = bits[(bits & np.uint32(0x7fffffff)) <= np.uint32(0x7f800000)]                                                # no NaNs
    neg = bits[bits >= np.uint32(0x80000000)]
    return np.concatenate([neg[::-1], bits[bits < np.uint32(0x80000000)]])           # negatives: larger magnitude first; then +0 upwards


def test_keys_follow_the_float_order_and_decode_back(fk):
    bits = _inputs()
    f = bits.view(np.float32)
    assert bits.size > 99000 and np.all(np.diff(f.astype(np.float64)) >= 0)          # the list is in float order ...
    zero = int(np.flatnonzero(bits == np.uint32(0x80000000))[0])
    assert bits[zero + 1] == 0                                                       # ... with -0 directly before +0
    raw, canon, back, back_canon = fk(bits)
    assert np.all(raw[1:] > raw[:-1])                                                # raw: strictly monotone, -0 < +0 included
    step = canon[1:].astype(np.int64) - canon[:-1].astype(np.int64)
    assert step[zero] == 0 and np.all(np.delete(step, zero) > 0)                     # canonical: strictly monotone but for -0 == +0
    assert np.array_equal(canon[bits != np.uint32(0x80000000)], raw[bits != np.uint32(0x80000000)])
    assert np.array_equal(back, bits)                                                # the decoder inverts the raw encoder exactly
    assert back_canon[zero] == 0 and np.array_equal(np.delete(back_canon, zero), np.delete(bits, zero))    # canon(-0) decodes to +0
