"""Evaluation on the device: atom / molecule stability of sampled molecules.  The RDKit-dependent metrics of the
reference's evaluation package (validity, uniqueness, novelty, Complete, FCD, geometry MMD) are out of scope."""
from .rules import (MissingSectionError, RulesError, StabilityRules, UnknownDatasetError, UnknownElementError,  # noqa: F401
                    ValenceRangeError)
from .stability import COUNT_KEYS, get_2D_edm_metric, get_edm_metric, get_stability_fn  # noqa: F401
