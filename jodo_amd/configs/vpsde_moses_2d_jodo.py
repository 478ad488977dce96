"""JODO on MOSES, 2-D graphs only (model DGT_concat_2D, AncestralSampler_2D): aromatic bond channel, no formal charges."""
from ._common import build
from .vpsde_zinc_2d_jodo import _DROP_2D


def get_config():
    return build(dict(
        exp_type='vpsde', only_2D=True,
        data=dict(root='data/MOSES', name='MOSES', collate='collate_edge_2D', info_name='moses', include_aromatic=True,
                  atom_types=7, bond_types=5, max_node=27),
        model=dict(name='DGT_concat_2D', include_fc_charge=False, normalize_factors='1, 2, 2, 1', edge_ch=3, time_dim=1024,
                   n_extra_heads=1, rw_depth=8, loss_weights='1., 1., 0.5'),
        training=dict(n_iters=1200000),
        optim=dict(grad_clip=20.),
        eval=dict(batch_size=2000, begin_ckpt=10, end_ckpt=10, sub_geometry=False),
    ), drop=_DROP_2D + (('data', 'fc_scale'),))
