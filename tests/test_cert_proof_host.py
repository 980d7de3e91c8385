"""The C ABI of the certificate's proof (fast_verification STEP 1, dpgo_amd/csrc/cert.cpp: dpgo_group_cert_factor,
dpgo_group_verify, dpgo_group_cert_matrix): the symbols, their signatures, the constants and the argument checks that
return before any device call.  No GPU."""
import ctypes as C

import numpy as np

import dpgo_amd

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_symbols_signatures_and_constants():
    L = dpgo_amd.lib()
    want = {
        "dpgo_group_cert_factor": [C.c_void_p, DP, C.c_int, C.c_double, C.c_longlong, C.c_void_p],
        "dpgo_group_verify": [C.c_void_p, DP, C.c_int, C.c_void_p, C.c_longlong, DP, C.c_int, C.c_void_p, DP, C.c_int, C.c_void_p],
        "dpgo_group_cert_matrix": [C.c_void_p, DP, C.c_int, C.c_double, IP, IP, DP, C.c_longlong, C.POINTER(C.c_longlong)],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == args, name
    assert dpgo_amd.CERT_PROVEN == 3 and dpgo_amd.CERT_NAMES[dpgo_amd.CERT_PROVEN] == "PROVEN"
    assert (dpgo_amd.CERT_UNDECIDED, dpgo_amd.CERT_NONNEGATIVE, dpgo_amd.CERT_NEGATIVE) == (0, 1, 2)
    assert (dpgo_amd.CERT_FACTOR_NOT_PD, dpgo_amd.CERT_FACTOR_PD, dpgo_amd.CERT_FACTOR_SKIPPED) == (0, 1, 2)


def test_cert_factor_struct_layout():
    """dpgo_cert_factor_t: four ints, two long longs, six doubles -- 80 bytes, no padding."""
    f = dpgo_amd.CertFactor()
    names = [n for n, _ in dpgo_amd.CertFactor._fields_]
    assert names == ["outcome", "fronts", "levels", "max_front", "factor_entries", "factor_bytes", "eta", "pivot_min",
                     "pivot_max", "stationarity", "symbolic_s", "numeric_s"]
    assert C.sizeof(f) == 4 * 4 + 2 * 8 + 6 * 8
    assert dpgo_amd.CertFactor.factor_entries.offset == 16 and dpgo_amd.CertFactor.eta.offset == 32


def test_null_arguments_return_minus_one():
    L = dpgo_amd.lib()
    X = np.zeros((8, 3), order="F")
    dp = X.ctypes.data_as(DP)
    o, res, fac = dpgo_amd.CertOptions(), dpgo_amd.CertResult(), dpgo_amd.CertFactor()
    nnz = C.c_longlong(-7)
    fake = C.c_void_p(0)
    # no group
    assert L.dpgo_group_cert_factor(None, dp, 8, 1e-3, 0, C.byref(fac)) == -1
    assert L.dpgo_group_verify(None, dp, 8, C.byref(o), 0, None, 0, C.byref(res), None, 0, C.byref(fac)) == -1
    assert L.dpgo_group_cert_matrix(None, dp, 8, 1e-3, None, None, None, 0, C.byref(nnz)) == -1
    # no X, no options, no result, no factor record, no count
    assert L.dpgo_group_cert_factor(fake, None, 8, 1e-3, 0, C.byref(fac)) == -1
    assert L.dpgo_group_cert_factor(fake, dp, 8, 1e-3, 0, None) == -1
    assert L.dpgo_group_verify(fake, None, 8, C.byref(o), 0, None, 0, C.byref(res), None, 0, C.byref(fac)) == -1
    assert L.dpgo_group_verify(fake, dp, 8, None, 0, None, 0, C.byref(res), None, 0, C.byref(fac)) == -1
    assert L.dpgo_group_verify(fake, dp, 8, C.byref(o), 0, None, 0, None, None, 0, C.byref(fac)) == -1
    assert L.dpgo_group_verify(fake, dp, 8, C.byref(o), 0, None, 0, C.byref(res), None, 0, None) == -1
    assert L.dpgo_group_cert_matrix(fake, None, 8, 1e-3, None, None, None, 0, C.byref(nnz)) == -1
    assert L.dpgo_group_cert_matrix(fake, dp, 8, 1e-3, None, None, None, 0, None) == -1
    # nothing was written on the way out
    assert nnz.value == -7 and fac.outcome == 0 and fac.fronts == 0 and res.status == 0 and res.iterations == 0
