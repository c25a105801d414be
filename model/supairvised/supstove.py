from stove_amd.supairvised.supstove import *  # noqa: F401,F403
from stove_amd.supairvised.supstove import SupStove  # noqa: F401
