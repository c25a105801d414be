"""CPU-side checks (-m "not gpu") of the rollout backward's C ABI: the four entry points (stove_rollout_bwd_ws_bytes, stove_rollout_bwd
and their _cl siblings) are exported by the built library, declared in the public header and bound by stove_amd._lib with the header's
argument counts and types, and the addition leaves the ABI version where it was.  (Fails before the rollout backward: the symbols do
not exist.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('stove_rollout_bwd_ws_bytes', 'stove_rollout_bwd', 'stove_rollout_bwd_ws_bytes_cl', 'stove_rollout_bwd_cl')


def _header_decl(name):
    """the declaration of `name` in include/stove_hip.h -> (return type, [parameter text, ...])"""
    header = open(os.path.join(ROOT, 'include', 'stove_hip.h')).read()
    m = re.search(r'^(int|size_t)\s+%s\s*\(([^;]*?)\)\s*;' % re.escape(name), header, flags=re.M | re.S)
    assert m, name + ' is not declared in include/stove_hip.h'
    return m.group(1), [a.strip() for a in m.group(2).split(',')]


def _names(name):
    return [p.split()[-1].lstrip('*') for p in _header_decl(name)[1]]


def test_rollout_backward_symbols_are_exported_declared_and_bound():
    from stove_amd import _lib, build
    build.build_library()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
    lib = _lib.load()                                   # _declare() binds every entry of its table: a missing one raises here
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        ret, params = _header_decl(name)
        assert fn.restype is (ctypes.c_int if ret == 'int' else ctypes.c_size_t), (name, fn.restype)
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
        for ct, text in zip(fn.argtypes, params):        # pointers, ints and floats in the header's order
            want = ctypes.c_void_p if '*' in text else (ctypes.c_float if text.startswith('float') else ctypes.c_int)
            assert ct is want, (name, text, ct)
    assert lib.stove_abi_version() == _lib.ABI_VERSION == 7


def test_backward_entry_points_follow_the_forward_signatures():
    """The backward takes the sampling forward's inputs (z_last, extra, params, eps), its output z_pred, the three upstream gradients,
    the three outputs and the workspace, then the forward's scalars in the forward's order; `cl` sits between the pointers and B."""
    fwd = _names('stove_rollout_sample_fwd')
    want = ['z_last', 'extra', 'params', 'eps', 'z_pred', 'd_z_pred', 'd_log_q', 'd_pred', 'd_z_last', 'd_extra', 'g_params', 'ws']
    assert _names('stove_rollout_bwd') == want + fwd[8:]
    assert _names('stove_rollout_bwd_cl') == want + ['cl'] + fwd[8:]
    assert _names('stove_rollout_bwd_ws_bytes') == ['B', 'N'] and _names('stove_rollout_bwd_ws_bytes_cl') == ['cl', 'B', 'N']


def test_workspace_query_rejects_what_the_call_rejects():
    """The queries run on the host alone: one partial gradient image per workgroup for shapes the entry points take, 0 otherwise."""
    from stove_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    grads = lib.stove_gnn_grad_floats()
    for B, N in ((1, 1), (11, 3), (11, 7), (256, 6), (600, 8)):
        assert lib.stove_rollout_bwd_ws_bytes(B, N) == lib.stove_gnn_blocks(B, N) * grads * 4, (B, N)
    for B, N in ((0, 3), (-1, 3), (4, 0), (4, 9)):
        assert lib.stove_rollout_bwd_ws_bytes(B, N) == 0, (B, N)
    for cl in (16, 64):
        assert lib.stove_rollout_bwd_ws_bytes_cl(cl, 11, 5) == lib.stove_gnn_bwd_ws_bytes_cl(cl, 11, 5) > 0
        assert lib.stove_rollout_bwd_ws_bytes_cl(cl, 11, 7) == 0
    assert lib.stove_rollout_bwd_ws_bytes_cl(32, 11, 3) == 0
