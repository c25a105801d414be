from stove_amd.rl.agents import *  # noqa: F401,F403
