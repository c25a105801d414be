"""Same-process A/B of the replayed training step on colour billiards (config.channels = 3, debug_bw = False): the fused colour scene
likelihood (stove_scene_fwd_ch / _bwd_ch) against the reference's composed op sequence (config.scene_composed = True), alternating.
The model is built as bench.Job builds it, with the config overridden here.
Usage: python tools/colour_ab.py [T ...]      (default: 8 100; 256 clips each)     env COLOUR_REPS (3), COLOUR_STEPS (30),
COLOUR_MODES (fused,composed)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
frames, sys.argv = [int(a) for a in sys.argv[1:]] or [8, 100], sys.argv[:1]
import torch  # noqa: E402

import bench  # noqa: E402

dev = torch.device('cuda:0')
REPS = int(os.environ.get('COLOUR_REPS', '3'))
STEPS = int(os.environ.get('COLOUR_STEPS', '30'))
MODES = os.environ.get('COLOUR_MODES', 'fused,composed').split(',')
_build_config = bench.build_config


def colour_config(composed):
    def build(*a, **kw):
        cfg = _build_config(*a, **kw)
        cfg.channels, cfg.debug_bw, cfg.scene_composed = 3, False, composed
        return cfg
    return build


for T in frames:
    data = bench.make_batch('billiards', 256, T, 0)
    for rep in range(REPS):
        for mode in MODES:
            bench.build_config = colour_config(mode == 'composed')
            job = bench.Job('billiards', dev, data, 'bf16x3', 'f32', 1)
            assert job.cfg.channels == 3 and not job.cfg.debug_bw and job.model.sup.bg_spn.num_dims == 3 * 32 * 32
            job.step(0)
            ms, ms_max, _ = job.median_ms(STEPS)
            print('T=%d %-8s ms/step %.3f (max %.3f)' % (T, mode, ms, ms_max), flush=True)
            del job
            torch.cuda.empty_cache()
    bench.build_config = _build_config
