"""Configuration of the state-supervised baseline (reference model/supairvised/config.py:4-37): StoveConfig with the
reference's values for the supervised scenario, where the object states come from the environment."""
from ..video_prediction.config import StoveConfig


class SupStoveConfig(StoveConfig):
    supairvised = True               # for easy identification in logs

    num_epochs = 400
    num_visible = 6                  # two less than the full model: skip = 0
    num_rollout = 8
    frame_step = 1
    batch_size = 256
    cl = 16
    discount_factor = 0.98           # discount of the loss along the rollout
    learning_rate = 0.002
    min_learning_rate = 0.0002
    debug_anneal_lr = 20000

    num_obj = 3

    load_encoder = None
    debug_disable_v_error = False
    debug_disable_v_diff_error = False

    debug_rollout = True             # run the core over the observed states to initialise the latent
    debug_rollout_training = True    # ... during training too
    debug_add_noise = False
