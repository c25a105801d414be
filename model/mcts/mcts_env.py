from stove_amd.mcts.mcts_env import *  # noqa: F401,F403
from stove_amd.mcts.mcts_env import MCTS, EnvForest, plan_on_envs  # noqa: F401
