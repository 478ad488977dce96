"""The property classifier of the conditional evaluation (the reference's cond_gen package): EGNN on the HIP kernels."""
from .model import EGNN, get_classifier, get_model  # noqa: F401
