"""The supervised model (reference model/supairvised/supstove.py): the dynamics core on given states.  The reference's `.sup`
(Supervisor: SuPAIR states in place of the environment's, chosen by load_encoder) is not built."""
import torch.nn as nn

from .dynamics import SupervisedDynamics

NO_SUPERVISOR = 'SuPAIR-state supervision (reference supairvised/supervisor.py, selected by load_encoder) is out of scope: ' \
                'the supervised baseline trains on ground-truth states only'


class SupStove(nn.Module):
    def __init__(self, config):
        super().__init__()
        if config.load_encoder is not None:
            raise NotImplementedError(NO_SUPERVISOR)
        self.dyn = SupervisedDynamics(config)
        self.c = config
