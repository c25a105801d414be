from stove_amd.rl.rl_model import *  # noqa: F401,F403
