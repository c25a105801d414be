from stove_amd.rl.runners import *  # noqa: F401,F403
