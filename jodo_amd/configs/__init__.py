"""Config surface of the JODO experiments on the hot path (same keys and defaults as the reference's
configs/vpsde_qm9_uncond_jodo.py, vpsde_geom_uncond_jodo.py, vpsde_qm9_cond_jodo.py, vpsde_qm9_cond_multi_jodo.py and the two 2-D
experiments vpsde_zinc_2d_jodo.py, vpsde_moses_2d_jodo.py, and the two CDGS
experiments vpsde_qm9_2d_cdgs.py, vpsde_geom_2d_cdgs.py)."""
from . import vpsde_qm9_uncond_jodo, vpsde_geom_uncond_jodo, vpsde_qm9_cond_jodo, vpsde_qm9_cond_multi_jodo  # noqa: F401
from . import vpsde_zinc_2d_jodo, vpsde_moses_2d_jodo  # noqa: F401
from . import vpsde_qm9_2d_cdgs, vpsde_geom_2d_cdgs  # noqa: F401


def get(name):
    import importlib
    return importlib.import_module(__name__ + '.' + name).get_config()
