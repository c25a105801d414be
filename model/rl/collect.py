from stove_amd.rl.collect import *  # noqa: F401,F403
