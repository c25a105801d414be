from stove_amd.rl.pretrained import *  # noqa: F401,F403
