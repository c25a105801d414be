from stove_amd.envs.envs import *  # noqa: F401,F403
from stove_amd.envs.batched import BatchedAvoidance  # noqa: F401
from stove_amd.envs.synth import (BatchedSequences, accepted, draw_starts, generate_data, generate_runs,  # noqa: F401
                                  synth_sequences_batched)
