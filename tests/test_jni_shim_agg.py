"""CPU: readGrouped of the JNI shim (jni/sgx_jni.c) with a reducing aggregation, through the fake
JNIEnv and a recording stand-in for the engine (tests/native/jni_fake_agg.c): the engine sees
the aggregation the JVM passed (AGG_MIN = 2, ...), and a reducing read may leave group_starts out
(Java null -> NULL; the capacity in groups then comes from the keys buffer alone)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(sgx_lib, tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    out = str(tmp_path_factory.mktemp("jni_agg") / "libjniagg.so")
    lib_dir = os.path.join(ROOT, "sparkucx_amd")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-Wl,-Bsymbolic",
                    "-I" + os.path.join(ROOT, "jni", "stub"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "sgx_jni.c"), os.path.join(ROOT, "tests", "native", "jni_fake_agg.c"),
                    "-L" + lib_dir, "-l:libsgx.so", "-Wl,-rpath," + lib_dir, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.fake_exception_class.restype = ctypes.c_char_p
    L.fake_read_grouped.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p, ctypes.c_int64] * 3 + [ctypes.c_void_p] * 2
    return L


def read_grouped(shim, agg, nmaps, keys, starts, vals):
    out3, seen = np.zeros(3, np.int64), np.zeros(8, np.int64)
    args = []
    for a in (keys, starts, vals):
        args += [a.ctypes.data if a is not None else None, a.nbytes if a is not None else 0]
    shim.fake_clear()
    n = shim.fake_read_grouped(agg, nmaps, *args, out3.ctypes.data, seen.ctypes.data)
    return n, out3.tolist(), dict(zip(("agg", "keys_null", "starts_null", "values_null", "cap_groups", "cap_values",
                                       "start", "end"), seen.tolist())), shim.fake_exception_class().decode()


@pytest.mark.parametrize("agg", [2, 3, 4, 1])  # AGG_MIN, AGG_MAX, AGG_COUNT; AGG_SUM as before
def test_read_grouped_reducing_aggregation(shim, sgx_lib, agg):
    assert (sgx_lib.AGG_SUM, sgx_lib.AGG_MIN, sgx_lib.AGG_MAX, sgx_lib.AGG_COUNT) == (1, 2, 3, 4)
    # size query: Java nulls, capacities 0
    n, out3, seen, exc = read_grouped(shim, agg, 3, None, None, None)
    assert (n, out3, exc) == (3, [6, 6, 42], "")
    assert seen == dict(agg=agg, keys_null=1, starts_null=1, values_null=1, cap_groups=0, cap_values=0, start=1, end=3)
    # the fill without a group_starts buffer: NULL reaches the engine, the keys buffer bounds the groups
    keys, vals = np.zeros(7, np.int64), np.zeros(6, np.int64)
    n, out3, seen, exc = read_grouped(shim, agg, 3, keys, None, vals)
    assert (n, out3, exc) == (3, [6, 6, 42], "")
    assert seen == dict(agg=agg, keys_null=0, starts_null=1, values_null=0, cap_groups=7, cap_values=6, start=1, end=3)
    assert keys[:6].tolist() == list(range(100, 106)) and vals.tolist() == [-7 - v for v in range(6)]
    # GpuShuffleReader passes a starts buffer for every aggregation: the smaller buffer bounds both
    starts = np.full(6, -1, np.int64)
    n, out3, seen, exc = read_grouped(shim, agg, 3, keys, starts, vals)
    assert (n, exc) == (3, "") and seen["starts_null"] == 0 and seen["cap_groups"] == 6
    # too small a values buffer: the engine's SGX_ERR_INVALID becomes IllegalArgumentException
    n, _, _, exc = read_grouped(shim, agg, 3, keys, None, vals[:5])
    assert (n, exc) == (-1, "java/lang/IllegalArgumentException")
