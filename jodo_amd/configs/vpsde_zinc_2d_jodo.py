"""JODO on ZINC250k, 2-D graphs only (model DGT_concat_2D, AncestralSampler_2D)."""
from ._common import build

# keys of the 3-D experiments that the 2-D configs do not have
_DROP_2D = (('model', 'dist_gbf'), ('model', 'gbf_name'), ('model', 'CoM'), ('model', 'spatial_cut_off'),
            ('sampling', 'dpm_solver_method'), ('sampling', 'dpm_solver_order'))


def get_config():
    return build(dict(
        exp_type='vpsde', only_2D=True,
        data=dict(root='data/zinc250k', name='Zinc250k', collate='collate_edge_2D', info_name='zinc250k',
                  atom_types=9, bond_types=4, fc_scale=[-1., 1.], max_node=38),
        model=dict(name='DGT_concat_2D', normalize_factors='1, 2, 2, 1', time_dim=1024, n_extra_heads=1,
                   loss_weights='1., 1., 0.5'),
        optim=dict(grad_clip=20.),
        eval=dict(batch_size=2000, begin_ckpt=10, end_ckpt=10, sub_geometry=False),
    ), drop=_DROP_2D)
