"""CDGS on QM9, 2-D graphs only (model CDGS: noise prediction, no self-conditioning, AncestralSampler_2D)."""
from ._common import build

# keys of the JODO experiments that the CDGS configs do not have
_DROP_CDGS = (('model', 'dist_gbf'), ('model', 'gbf_name'), ('model', 'CoM'), ('model', 'spatial_cut_off'), ('model', 'edge_quan_th'),
              ('model', 'n_extra_heads'), ('sampling', 'dpm_solver_method'), ('sampling', 'dpm_solver_order'))


def get_config():
    return build(dict(
        exp_type='vpsde', only_2D=True,
        data=dict(collate='collate_edge_2D'),
        sde=dict(schedule='linear'),
        model=dict(name='CDGS', pred_data=False, include_fc_charge=False, normalize_factors='1, 2, 2, 1', self_cond=False,
                   rw_depth=8, softmax_inf=False, loss_weights='1., 1., 0.5'),
        eval=dict(batch_size=10000, begin_ckpt=90, end_ckpt=100, sub_geometry=False),
    ), drop=_DROP_CDGS)
