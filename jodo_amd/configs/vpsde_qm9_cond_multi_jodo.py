"""Conditional JODO on QM9, two properties (the reference's configs/vpsde_qm9_cond_multi_jodo.py): context column 0 is
`cond_property1`, column 1 `cond_property2`.

Like the single-property file it has no `sampling.dpm_solver_*` keys.
"""
from ._common import build


def get_config():
    cfg = build(dict(
        exp_type='vpsde_edge_cond_multi', cond_property1='alpha', cond_property2='mu',
        data=dict(transform='EdgeComCondMulti', collate='collate_cond', info_name='qm9_second_half'),
        model=dict(name='cond_DGT_concat', cond_ch=2),
        training=dict(n_iters=2500000),
        eval=dict(begin_ckpt=50, end_ckpt=50, sub_geometry=False),
    ), drop=(('sampling', 'dpm_solver_method'), ('sampling', 'dpm_solver_order')))
    return cfg
