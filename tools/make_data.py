"""Write the reference's data files (its `python -m model.envs.envs`): <name>_train.pkl and <name>_test.pkl for billiards, gravity,
multibilliards or avoidance, every chunk of candidate sequences simulated together -- with --device in one launch of
stove_env_sequences, without it by the numpy specification (stove_amd/envs/synth.py: generate_data).

  python tools/make_data.py gravity --device cuda:0 --res 50 --out data
  python tools/make_data.py avoidance --runs 1000 300 --seed0 0
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stove_amd.envs.synth import main  # noqa: E402

if __name__ == '__main__':
    main()
