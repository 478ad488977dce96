"""Fitting and saving the property classifier (the EGNN of jodo_amd.cond_gen.model) on the GPU.

The conditional evaluation loops de-normalise a classifier's output as `pred * mad + mean` before taking the L1 distance to the target
property; a classifier is therefore fitted to `(label - mean) / mad` under an L1 loss (the published EDM classifiers are).  The step runs
the HIP training path (csrc/egnn_train.hip) through `EGNN.hip_training`; there is no CPU fallback.  Data loading and the property labels
are the caller's."""
import argparse
import pickle

import torch


def classifier_loss(pred, label, mean, mad):
    """L1 of pred [B] against the normalised label (label - mean) / mad: the inverse of `pred * mad + mean` in the evaluation loops."""
    return torch.nn.functional.l1_loss(pred, (label.to(pred.dtype) - mean) / mad)


def get_classifier_step_fn(optimizer, mean, mad, grad_clip=None):
    """step_fn(classifier, one_hot [B, N, in_node_nf], pos [B, N, 3], n_nodes, label [B]) -> loss (a detached 0-d tensor): one optimiser
    step on one batch.  Masks and edges are built as the evaluation loops build them, `hip_training` is switched on, gradients are
    clipped to the norm `grad_clip` when given.  `optimizer`: torch.optim.Adam / AdamW or jodo_amd.optim.FlatAdam over
    classifier.parameters()."""
    from ..sampling import build_masks, full_edge_index

    def step_fn(classifier, one_hot, pos, n_nodes, label):
        B, N = one_hot.shape[0], one_hot.shape[1]
        device = one_hot.device
        n_list = [int(v) for v in n_nodes]
        node_mask, edge_mask = build_masks(n_list, N, device)
        classifier.hip_training = True
        classifier.train()
        optimizer.zero_grad(set_to_none=True)
        pred = classifier(h0=one_hot.detach().reshape(B * N, -1), x=pos.detach().reshape(B * N, -1), edges=full_edge_index(N, B, device),
                          edge_attr=None, node_mask=node_mask.reshape(B * N, -1), edge_mask=edge_mask, n_nodes=N)
        loss = classifier_loss(pred, label.to(device), mean, mad)
        loss.backward()
        if grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(classifier.parameters(), grad_clip)
        optimizer.step()
        return loss.detach()

    return step_fn


def save_classifier(classifier, classifier_path, args_path):
    """Write the published layout that get_classifier reads: a pickled args object with nf, n_layers, attention, node_attr (plus
    model_name and device, which get_classifier overwrites) and the state_dict on the CPU."""
    args = argparse.Namespace(nf=int(classifier.hidden_nf), n_layers=int(classifier.n_layers), attention=bool(classifier.attention),
                              node_attr=int(classifier.node_attr), model_name='egnn', device='cpu')
    with open(args_path, 'wb') as f:
        pickle.dump(args, f)
    torch.save({k: v.detach().cpu() for k, v in classifier.state_dict().items()}, classifier_path)
