"""CPU-side check (-m "not gpu") of the one-launch sampling rollout's C ABI: the two entry points extend the mean rollout's parameter
lists.  (That they are exported, declared and bound with the header's types: tests/test_host_cpu.py,
test_binding_table_follows_the_header.)"""
from control_harness import header_decl


def test_sampling_entry_points_extend_the_mean_rollout_signatures():
    """eps after params, log_q after z_pred; everything else is the mean rollout's list, in its order (`cl` included)."""
    for sfx in ('', '_cl'):
        mean = [p.split()[-1].lstrip('*') for p in header_decl('stove_rollout_fwd' + sfx)[1]]
        smp = [p.split()[-1].lstrip('*') for p in header_decl('stove_rollout_sample_fwd' + sfx)[1]]
        assert smp == mean[:3] + ['eps'] + mean[3:4] + ['log_q'] + mean[4:], (sfx, smp)
