"""Train a PPO arm (stove_amd/rl/main_rl.py), the model-free one on states or the model-based one on the learned dynamics:

    python tools/run_ppo.py --use-states --experiment_id run0 [--device-envs] [--fused-update] [--num-env-steps 409600]
    python tools/run_ppo.py --use-pretrained-model --checkpoint RUN_DIR --data SEQUENCES.pkl --experiment_id run1 [--fused-update]
                            [--fused-widths 16,32,64]
    python tools/run_ppo.py --use-images --experiment_id run2 [--device-envs] [--fused-update] [--hidden-size 512] [--num-stacked-frames 4]

The reference's `python -m model.rl.main_rl --use-states` with the same flags; `--device-envs` keeps the environments on the GPU, where a
batch of trajectories is collected in one launch; `--fused-update` runs the PPO update there in one launch too (off by default).
`--use-pretrained-model` imagines the trajectories on the trained action-conditioned model of RUN_DIR, one launch per batch on a GPU
(a model of state-code length 16 or 64: with `--fused-widths 16,32,64`, else the composed loop).
`--use-images` is the reference's default arm, PPO on rendered frames (there: no flag); with `--device-envs` a batch is one launch, and with `--fused-update` its update runs on the device on the frames the
collection wrote (stove_ppo_update_images)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stove_amd import build  # noqa: E402


def main(argv=None):
    build.build_library()          # (hipcc is spawned before the process touches the GPU)
    from stove_amd.rl.main_rl import main as main_rl
    return main_rl(sys.argv[1:] if argv is None else argv)


if __name__ == '__main__':
    main()
