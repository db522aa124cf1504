"""CPU checks of the batched parameter-derivative interface: the C-ABI declares and exports it, and the Python layer binds it."""
import ctypes as ct
import os
import re
import pytest
import parity_util as P

SYMBOLS = ['upside_hip_get_param_deriv_all', 'upside_hip_param_deriv_accumulate', 'upside_hip_param_deriv_read']


def test_header_declares_the_batched_calls():
    txt = open(os.path.join(P.ROOT, 'include', 'upside_engine_c.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'int\s+upside_hip_get_param_deriv_all\s*\(\s*DerivEngine\s*\*\s*\w+\s*,\s*const char\s*\*\s*\w+\s*,\s*int\s+\w+\s*,'
                     r'\s*float\s*\*\s*\w+\s*\)\s*;', txt)
    assert re.search(r'int\s+upside_hip_param_deriv_accumulate\s*\(\s*DerivEngine\s*\*\s*\w+\s*,\s*const char\s*\*\s*\w+\s*,'
                     r'\s*const float\s*\*\s*\w+\s*\)\s*;', txt)
    assert re.search(r'int\s+upside_hip_param_deriv_read\s*\(\s*DerivEngine\s*\*\s*\w+\s*,\s*const char\s*\*\s*\w+\s*,\s*int\s+\w+\s*,'
                     r'\s*double\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;', txt)


def test_library_exports_the_batched_calls():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.skip('libupside_hip.so not built (run __graft_entry__.build())')
    lib = ct.CDLL(P.pkg.PRODUCT_LIB)
    missing = [n for n in SYMBOLS + ['upk_rotamer_param_deriv_all', 'upk_igraph_param_deriv_all', 'upk_param_deriv_reduce']
               if not hasattr(lib, n)]
    assert not missing, missing


def test_ensemble_binds_the_batched_calls():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.skip('libupside_hip.so not built (run __graft_entry__.build())')
    lib = P.pkg.UpsideLibrary(P.pkg.PRODUCT_LIB)
    P.pkg.engine.Ensemble._bind(lib.calc)
    for n in SYMBOLS:
        assert getattr(lib.calc, n).argtypes, n
    for m in ('param_deriv', 'param_deriv_accumulate', 'param_deriv_read'):
        assert callable(getattr(P.pkg.engine.Ensemble, m))
