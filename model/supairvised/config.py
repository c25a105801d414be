from stove_amd.supairvised.config import *  # noqa: F401,F403
from stove_amd.supairvised.config import SupStoveConfig  # noqa: F401
