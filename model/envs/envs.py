from stove_amd.envs.envs import *  # noqa: F401,F403
from stove_amd.envs.batched import BatchedAvoidance  # noqa: F401
