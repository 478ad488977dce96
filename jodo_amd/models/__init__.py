"""Model registry of the hot path.  Importing this package registers the HIP-backed
'DGT_concat', 'cond_DGT_concat', 'DGT_concat_sim', 'DGT_concat_2D' and 'CDGS' (reference: models/__init__.py:1-4)."""
from .utils import create_model, register_model, get_model_class  # noqa: F401
from .node_distribution import get_node_dist, DistributionNodes, load_dataset_info  # noqa: F401
from .dgt import DGT_concat, Cond_DGT_concat, DGT_concat_sim  # noqa: F401
from .dgt2d import DGT_concat_2D  # noqa: F401
from .cdgs import CDGS  # noqa: F401
from .init_utils import deterministic_init_  # noqa: F401
