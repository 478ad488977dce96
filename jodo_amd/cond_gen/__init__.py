"""The reference's cond_gen package: the property classifier of the conditional evaluation (EGNN on the HIP kernels, and its fitting)
and the property prior that conditional sampling draws its targets from (DistributionProperty)."""
from .model import EGNN, get_classifier, get_model  # noqa: F401
from .property_distribution import DistributionProperty, compute_mean_mad  # noqa: F401
from .train import classifier_loss, get_classifier_step_fn, save_classifier  # noqa: F401
