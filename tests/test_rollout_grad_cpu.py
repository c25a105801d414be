"""CPU-side checks (-m "not gpu") of the rollout backward's C ABI: the four entry points (stove_rollout_bwd_ws_bytes, stove_rollout_bwd
and their _cl siblings) take the forward's parameters in the forward's order, and their workspace queries reject what the calls reject.
(That they are exported, declared and bound with the header's types: tests/test_host_cpu.py, test_binding_table_follows_the_header.)"""
from control_harness import header_decl


def _names(name):
    return [p.split()[-1].lstrip('*') for p in header_decl(name)[1]]


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
