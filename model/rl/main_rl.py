from stove_amd.rl.main_rl import *  # noqa: F401,F403
