from stove_amd.supairvised.train import *  # noqa: F401,F403
from stove_amd.supairvised.train import SupTrainer  # noqa: F401
