"""CPU-side checks (-m "not gpu") of the one-launch sampling rollout's C ABI: the two entry points are exported by the built library,
declared in the public header and bound by stove_amd._lib with the header's argument counts, and the addition leaves the ABI
version where it was.  (Fails before the sampling rollout: the symbols do not exist.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('stove_rollout_sample_fwd', 'stove_rollout_sample_fwd_cl')


def _header_params(name):
    """the parameter list of `name` in include/stove_hip.h -> [parameter text, ...]"""
    header = open(os.path.join(ROOT, 'include', 'stove_hip.h')).read()
    m = re.search(r'^int\s+%s\s*\(([^;]*?)\)\s*;' % re.escape(name), header, flags=re.M | re.S)
    assert m, name + ' is not declared in include/stove_hip.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_sampling_rollout_symbols_are_exported_declared_and_bound():
    from stove_amd import _lib, build
    build.build_library()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
    lib = _lib.load()                                   # _declare() binds every entry of its table: a missing one raises here
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        params = _header_params(name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
        for ct, text in zip(fn.argtypes, params):        # pointers, ints and floats in the header's order
            want = ctypes.c_void_p if '*' in text else (ctypes.c_float if text.startswith('float') else ctypes.c_int)
            assert ct is want, (name, text, ct)
    assert lib.stove_abi_version() == _lib.ABI_VERSION == 7


def test_sampling_entry_points_extend_the_mean_rollout_signatures():
    """eps after params, log_q after z_pred; everything else is the mean rollout's list, in its order (`cl` included)."""
    for sfx in ('', '_cl'):
        mean = [p.split()[-1].lstrip('*') for p in _header_params('stove_rollout_fwd' + sfx)]
        smp = [p.split()[-1].lstrip('*') for p in _header_params('stove_rollout_sample_fwd' + sfx)]
        assert smp == mean[:3] + ['eps'] + mean[3:4] + ['log_q'] + mean[4:], (sfx, smp)
