"""Evaluation on the device: atom / molecule stability of sampled molecules and the sub-structure geometry MMD of bond
lengths, bond angles and dihedral angles.  The RDKit-dependent metrics of the reference's evaluation package (validity,
uniqueness, novelty, Complete, FCD) are out of scope."""
from .geometry import (GeometrySymbols, connected_mask, geometry_stat, get_geometry_fn, get_sub_geometry_metric,  # noqa: F401
                       merge_results)
from .mmd import compute_mmd, compute_mmd_many  # noqa: F401
from .rules import (MissingSectionError, RulesError, StabilityRules, UnknownDatasetError, UnknownElementError,  # noqa: F401
                    ValenceRangeError)
from .stability import COUNT_KEYS, get_2D_edm_metric, get_edm_metric, get_stability_fn  # noqa: F401
