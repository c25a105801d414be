"""Write the reference's data files (its `python -m model.envs.envs`): <name>_train.pkl and <name>_test.pkl for billiards, gravity,
multibilliards or avoidance, every chunk of candidate sequences simulated together -- with --device in one launch of
stove_env_sequences, without it by the numpy specification (stove_amd/envs/synth.py: generate_data).  --starts counter draws the starts
and action rows from the counter-based stream -- with --device in one launch of stove_env_draw_starts, nothing of a sequence computed
on the host.  It is another random stream than the default --starts host: the same distributions, other files.

  python tools/make_data.py gravity --device cuda:0 --res 50 --out data
  python tools/make_data.py multibilliards --device cuda:0 --starts counter --out data
  python tools/make_data.py avoidance --runs 1000 300 --seed0 0
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stove_amd.envs.synth import main  # noqa: E402

if __name__ == '__main__':
    main()
