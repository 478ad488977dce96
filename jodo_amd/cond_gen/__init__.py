"""The property classifier of the conditional evaluation (the reference's cond_gen package): EGNN on the HIP kernels, and its fitting."""
from .model import EGNN, get_classifier, get_model  # noqa: F401
from .train import classifier_loss, get_classifier_step_fn, save_classifier  # noqa: F401
