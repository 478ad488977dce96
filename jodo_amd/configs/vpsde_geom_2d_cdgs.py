"""CDGS on GEOM-Drugs, 2-D graphs only (model CDGS: 6 blocks, 16 random-walk steps, aromatic edge channel)."""
from ._common import build
from .vpsde_qm9_2d_cdgs import _DROP_CDGS


def get_config():
    return build(dict(
        exp_type='vpsde', only_2D=True,
        data=dict(root='data/geom', name='GeomDrug', processed_file='data_geom_drug_1.pt', collate='collate_edge_2D',
                  info_name='geom_with_h_1', include_aromatic=True, atom_types=16, bond_types=5, fc_scale=[-2., 3.], max_node=181),
        sde=dict(schedule='linear'),
        model=dict(name='CDGS', pred_data=False, include_fc_charge=False, normalize_factors='1, 2, 2, 1', edge_ch=3, n_layers=6,
                   self_cond=False, self_cond_type='clamp', rw_depth=16, softmax_inf=False, loss_weights='1., 1., 0.5'),
        training=dict(batch_size=16, eval_batch_size=16, eval_samples=96),
        optim=dict(grad_clip=20.),
        eval=dict(batch_size=200, begin_ckpt=20, end_ckpt=20, sub_geometry=False),
    ), drop=_DROP_CDGS)
