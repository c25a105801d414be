from stove_amd.mcts.mcts_stove import *  # noqa: F401,F403
from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler, run_mcts_model  # noqa: F401
from stove_amd.mcts.play import play  # noqa: F401
