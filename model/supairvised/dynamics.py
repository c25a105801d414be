from stove_amd.supairvised.dynamics import *  # noqa: F401,F403
from stove_amd.supairvised.dynamics import SupervisedDynamics  # noqa: F401
