"""Plain torch restatements of the fused training kernels (jodo_amd/csrc/train_fused.h), one function per public host function, written
from the formulas of train_fused.h / train_ops.h and the reference lines they cite (mol_gnn.py:71-94, 270-322; layers.py:165-184,
291-295, 328-334).  Each takes `dtype` (float64: the yardstick, float32: what fp32 arithmetic in torch's own order reaches) and returns
EVERY array the kernel stores, as a dict keyed like the kernel's arguments.

tests/test_fused_kernels_host.py anchors them to the models (a block composed from them against oracle.forward_dense and its sim / 2-D
twins; every backward against autograd through its forward).  tests/test_fused_kernels_gpu.py compares the kernels with them.

Conventions: edge rows [R, .] with edge_a / edge_c (global node rows) and edge_mol per row; modulation rows per molecule; weights in
PyTorch layouts ([out, in]).  Dropout multipliers are oracle.philox_ref.drop_mul at element row * width + column."""
import math

import numpy as np
import torch
from torch.nn import functional as F

from oracle import philox_ref as PR

A_GAUSS = (2 * 3.14159) ** 0.5            # layers.py:291-295 writes pi as 3.14159


def c_(t, dtype):
    return None if t is None else t.to(dtype)          # (not detached: the host test differentiates through the forward restatements)


def ln_rs(x):
    """LayerNorm without affine, eps 1e-6, biased variance -> (xhat, rstd [rows])."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    return (x - mean) * rstd, rstd[..., 0]


def ln_mod_bwd(dy, xhat, rstd, scale):
    """dx of y = xhat (1 + scale) + shift, xhat = LayerNorm(x):  g = dy (1 + scale);  dx = rstd (g - mean(g) - xhat mean(g xhat))."""
    g = dy * (1 + scale)
    return rstd[..., None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def gauss(x, means, stds):
    """CondGaussianLayer's features of the modulated distance x [rows]: [x, gaussians] [rows, De]."""
    sd = stds.abs() + 1e-5
    g = torch.exp(-0.5 * ((x[:, None] - means) / sd) ** 2) / (A_GAUSS * sd)
    return torch.cat([x[:, None], g], dim=-1)


def drop_masks(seed, site, p, rows, width, dtype):
    return torch.from_numpy(PR.drop_mul(seed, site, p, rows * width).reshape(rows, width)).to(dtype)


# ---- the three forward chains ---------------------------------------------------------------------------------------------------
def chain_a(P, tp, pos, gm, e_in, emod, dtype=torch.float64):
    """d2 -> Gaussian basis -> edge_emb([G ; e]) -> LayerNorm1 -> modulate -> tanh(lin_edge0), tanh(lin_edge1)   (mol_gnn.py:279-296)"""
    P = {k: c_(v, dtype) for k, v in P.items()}
    pos, gm, e_in, emod = (c_(t, dtype) for t in (pos, gm, e_in, emod))
    De = e_in.shape[1]
    diff = pos[tp['edge_a']] - pos[tp['edge_c']]
    d2 = (diff ** 2).sum(-1)
    m = tp['edge_mol']
    x = d2 * (gm[m, 0] + 1) + gm[m, 1]
    G = gauss(x, P['gbf_means'], P['gbf_stds'])
    e1 = F.linear(torch.cat([G, e_in], dim=-1), P['edge_emb_w'], P['edge_emb_b'])
    xh, rs = ln_rs(e1)
    et = xh * (1 + emod[m, De:2 * De]) + emod[m, :De]
    return dict(d2=d2, G=G, xh=xh, rs=rs, et=et, t0=torch.tanh(F.linear(et, P['le0'])), t1=torch.tanh(F.linear(et, P['le1'])))


def chain_a_2d(P, tp, e_in, emod, dtype=torch.float64):
    """The 2-D model's chain A: LayerNorm1 acts on e itself."""
    P = {k: c_(v, dtype) for k, v in P.items()}
    e_in, emod = c_(e_in, dtype), c_(emod, dtype)
    De, m = e_in.shape[1], tp['edge_mol']
    xh, rs = ln_rs(e_in)
    et = xh * (1 + emod[m, De:2 * De]) + emod[m, :De]
    return dict(xh=xh, rs=rs, et=et, t0=torch.tanh(F.linear(et, P['le0'])), t1=torch.tanh(F.linear(et, P['le1'])))


def chain_b(P, tp, e_in, n2e, emod, m3, m4, dtype=torch.float64):
    """e + g1 node2edge -> LayerNorm2 -> modulate -> ff_linear3 -> SiLU, dropout -> ff_linear4 -> dropout -> gate -> readout
    (mol_gnn.py:313-317, :570).  n2e: node2edge_lin(hhat) per node WITHOUT its bias; m3 [R, r De], m4 [R, De]: dropout multipliers."""
    P = {k: c_(v, dtype) for k, v in P.items()}
    e_in, n2e, emod, m3, m4 = (c_(t, dtype) for t in (e_in, n2e, emod, m3, m4))
    De, m = e_in.shape[1], tp['edge_mol']
    x1 = e_in + emod[m, 2 * De:3 * De] * (n2e[tp['edge_a']] + n2e[tp['edge_c']] + P['n2e_b'])
    xh, rs = ln_rs(x1)
    en = xh * (1 + emod[m, 4 * De:5 * De]) + emod[m, 3 * De:4 * De]
    f3 = F.linear(en, P['ff3_w'], P['ff3_b'])
    a3 = F.silu(f3) * m3
    f4 = F.linear(a3, P['ff4_w'], P['ff4_b'])
    e_out = en + emod[m, 5 * De:6 * De] * (f4 * m4)
    return dict(xh=xh, rs=rs, en=en, f3=f3, a3=a3, f4=f4, e_out=e_out, ro=F.linear(e_out, P['ero_w'], P['ero_b']))


def chain_c(P, tp, e_in, G, hr, hc, qmod, dtype=torch.float64):
    """input_lin([h_row ; h_col ; e ; G]) -> LayerNorm -> modulate -> coord_mlp.0 -> SiLU -> coord_mlp.2 -> tanh   (mol_gnn.py:71-84).
    hr / hc: W_row h, W_col h per node."""
    P = {k: c_(v, dtype) for k, v in P.items()}
    e_in, G, hr, hc, qmod = (c_(t, dtype) for t in (e_in, G, hr, hc, qmod))
    D, De, m = hr.shape[1], e_in.shape[1], tp['edge_mol']
    W = P['in_w']
    pre = F.linear(e_in, W[:, 2 * D:2 * D + De]) + F.linear(G, W[:, 2 * D + De:]) + P['in_b'] + hr[tp['edge_a']] + hc[tp['edge_c']]
    xh, rs = ln_rs(pre)
    u = xh * (1 + qmod[m, D:]) + qmod[m, :D]
    c0pre = F.linear(u, P['c0_w'], P['c0_b'])
    c0a = F.silu(c0pre)
    return dict(xh=xh, rs=rs, u=u, c0pre=c0pre, c0a=c0a, inv=torch.tanh(F.linear(c0a, P['c2_w'])))


# ---- their backward chains ------------------------------------------------------------------------------------------------------
def bwd_c(P, tp, inv, dinv, c0pre, xh, rs, qmod, de0, dtype=torch.float64):
    """dinv: gradient of the tanh OUTPUT; de0: what `de` holds before the call (the kernel adds into it)."""
    P = {k: c_(v, dtype) for k, v in P.items()}
    inv, dinv, c0pre, xh, rs, qmod, de0 = (c_(t, dtype) for t in (inv, dinv, c0pre, xh, rs, qmod, de0))
    D, De, m = xh.shape[1], de0.shape[1], tp['edge_mol']
    dpt = dinv * (1 - inv * inv)
    dc0 = (dpt @ P['c2_w']) * dsilu(c0pre)
    du = dc0 @ P['c0_w']
    dpre = ln_mod_bwd(du, xh, rs, qmod[m, D:])
    W = P['in_w']
    return dict(dinv=dpt, dc0=dc0, du=du, dpre=dpre, de=de0 + dpre @ W[:, 2 * D:2 * D + De], dG=dpre @ W[:, 2 * D + De:])


def bwd_b(P, tp, de_out, f4, f3, xh, rs, emod, m3, m4, dtype=torch.float64):
    P = {k: c_(v, dtype) for k, v in P.items()}
    de_out, f4, f3, xh, rs, emod, m3, m4 = (c_(t, dtype) for t in (de_out, f4, f3, xh, rs, emod, m3, m4))
    De, m = de_out.shape[1], tp['edge_mol']
    f4d = f4 * m4
    df4 = emod[m, 5 * De:6 * De] * de_out * m4
    dhid = (df4 @ P['ff4_w']) * m3 * dsilu(f3)
    den = de_out + dhid @ P['ff3_w']
    return dict(f4d=f4d, df4=df4, dhid=dhid, den=den, de_prev=ln_mod_bwd(den, xh, rs, emod[m, 4 * De:5 * De]))


def bwd_a(P, tp, dt1, dt0, xh, rs, emod, dG0, de_prev0, dtype=torch.float64):
    """dt1 / dt0: gradients of the PRE-tanh values.  dG0 / de_prev0: contents before the call (both are added into)."""
    P = {k: c_(v, dtype) for k, v in P.items()}
    dt1, dt0, xh, rs, emod, dG0, de_prev0 = (c_(t, dtype) for t in (dt1, dt0, xh, rs, emod, dG0, de_prev0))
    De, m = xh.shape[1], tp['edge_mol']
    det = dt1 @ P['le1'] + dt0 @ P['le0']
    de1 = ln_mod_bwd(det, xh, rs, emod[m, De:2 * De])
    W = P['edge_emb_w']
    return dict(det=det, de1=de1, dG=dG0 + de1 @ W[:, :De], de_prev=de_prev0 + de1 @ W[:, De:])


def bwd_a_2d(P, tp, dt1, dt0, xh, rs, emod, de_prev0, dtype=torch.float64):
    P = {k: c_(v, dtype) for k, v in P.items()}
    dt1, dt0, xh, rs, emod, de_prev0 = (c_(t, dtype) for t in (dt1, dt0, xh, rs, emod, de_prev0))
    De, m = xh.shape[1], tp['edge_mol']
    det = dt1 @ P['le1'] + dt0 @ P['le0']
    return dict(det=det, de_prev=de_prev0 + ln_mod_bwd(det, xh, rs, emod[m, De:2 * De]))


# ---- node rows ------------------------------------------------------------------------------------------------------------------
def node_ln_mod(a, res_b, row_mol, mods, g_off, sh_off, sc_off, dtype=torch.float64):
    a, res_b, mods = c_(a, dtype), c_(res_b, dtype), c_(mods, dtype)
    Fw = a.shape[1]
    mr = mods[row_mol]
    x = a if res_b is None else a + mr[:, g_off:g_off + Fw] * res_b
    xh, rs = ln_rs(x)
    return dict(xh=xh, rs=rs, y=xh * (1 + mr[:, sc_off:sc_off + Fw]) + mr[:, sh_off:sh_off + Fw])


def node_ln_mod_bwd(dy, xh, rs, row_mol, mods, sc_off, dx0=None, dtype=torch.float64):
    dy, xh, rs, mods, dx0 = (c_(t, dtype) for t in (dy, xh, rs, mods, dx0))
    dx = ln_mod_bwd(dy, xh, rs, mods[row_mol][:, sc_off:sc_off + dy.shape[1]])
    return dict(dx=dx if dx0 is None else dx0 + dx)


# ---- attention (layers.py:131-186): per molecule, rows (a, c) = (source, target) at edge_off[b] + a n + c ------------------------------
def attn_fwd(nn, H, XH, SC, q, k, v, t0, t1, adj2d, adjsp, dtype=torch.float64):
    """q, k [Nn, QK], v [Nn, D], t0 [R, QK], t1 [R, D] (tanh outputs), adj2d / adjsp [R] -> alpha [R, H], hhat [Nn, D]."""
    q, k, v, t0, t1, adj2d, adjsp = (c_(t, dtype) for t in (q, k, v, t0, t1, adj2d, adjsp))
    D = v.shape[1]
    C, SH = D // H, H - XH
    alphas, hhats, n0, e0 = [], [], 0, 0
    for n in nn:
        sl, el = slice(n0, n0 + n), slice(e0, e0 + n * n)
        qq, kk = q[sl].reshape(n, SH, SC), k[sl].reshape(n, SH, SC)
        S = (qq[None, :] * kk[:, None] * t0[el].reshape(n, n, SH, SC)).sum(-1) / math.sqrt(C)           # [a, c, SH]
        adj = [torch.where(t[el].reshape(n, n) > 0, 1.0, -1e10).to(dtype)[..., None] for t in (adj2d, adjsp)[:XH]]
        S = torch.cat(adj + [S], dim=-1)
        if n > 1:
            Sm = S + torch.where(torch.eye(n, dtype=torch.bool), float('-inf'), 0.0).to(dtype)[..., None]
            ex = (Sm - Sm.max(dim=0, keepdim=True).values).exp()
            alpha = ex / (ex.sum(0, keepdim=True) + 1e-16)
        else:
            alpha = torch.zeros_like(S)
        hh = (v[sl].reshape(n, 1, H, C) * t1[el].reshape(n, n, H, C) * alpha[..., None]).sum(0).reshape(n, D)
        alphas.append(alpha.reshape(n * n, H)); hhats.append(hh)
        n0 += n; e0 += n * n
    return dict(alpha=torch.cat(alphas), hhat=torch.cat(hhats))


def attn_bwd(nn, H, XH, SC, dhhat, q, k, v, t0, t1, alpha, dtype=torch.float64):
    """-> dS [R, H] (gradient of the scores, adjacency heads included), dt1 / dt0 (gradients of the PRE-tanh values), dq, dk, dv."""
    dhhat, q, k, v, t0, t1, alpha = (c_(t, dtype) for t in (dhhat, q, k, v, t0, t1, alpha))
    D = v.shape[1]
    C, SH = D // H, H - XH
    isc = 1.0 / math.sqrt(C)
    out = dict(dS=[], dt1=[], dt0=[], dq=[], dk=[], dv=[])
    n0, e0 = 0, 0
    for n in nn:
        sl, el = slice(n0, n0 + n), slice(e0, e0 + n * n)
        dh, vv = dhhat[sl].reshape(1, n, H, C), v[sl].reshape(n, 1, H, C)
        tt1, al = t1[el].reshape(n, n, H, C), alpha[el].reshape(n, n, H)
        dal = (dh * vv * tt1).sum(-1)                                                                  # [a, c, H]
        dS = al * (dal - (al * dal).sum(0, keepdim=True))
        out['dS'].append(dS.reshape(n * n, H))
        out['dt1'].append((dh * vv * al[..., None] * (1 - tt1 * tt1)).reshape(n * n, D))
        out['dv'].append((dh * tt1 * al[..., None]).sum(1).reshape(n, D))
        qq, kk, tt0 = q[sl].reshape(1, n, SH, SC), k[sl].reshape(n, 1, SH, SC), t0[el].reshape(n, n, SH, SC)
        ds = dS[..., XH:, None] * isc
        out['dq'].append((ds * kk * tt0).sum(0).reshape(n, SH * SC))
        out['dk'].append((ds * qq * tt0).sum(1).reshape(n, SH * SC))
        out['dt0'].append((ds * qq * kk * (1 - tt0 * tt0)).reshape(n * n, SH * SC))
        n0 += n; e0 += n * n
    return {k_: torch.cat(v_) for k_, v_ in out.items()}


# ---- Gaussian layer backward (layers.py CondGaussianLayer) ---------------------------------------------------------------------------
def gbf_bwd(d2, row_mol, gm, means, stds, dG, dd2_0=None, dtype=torch.float64):
    """dG [R, De]: gradient of [x', gaussians].  -> dxp [R], dd2 [R] (= dd2_0 + dxp (1 + scale)), part_m / part_s [ceil(R / 32), De - 1]:
    the sums of d means / d stds over chunks of 32 rows."""
    d2, gm, means, stds, dG, dd2_0 = (c_(t, dtype) for t in (d2, gm, means, stds, dG, dd2_0))
    R, K = d2.shape[0], means.shape[0]
    g0 = gm[row_mol, 0] + 1
    x = d2 * g0 + gm[row_mol, 1]
    sd, sg = stds.abs() + 1e-5, torch.sign(stds)
    z = (x[:, None] - means) / sd
    gk = torch.exp(-0.5 * z * z) / (A_GAUSS * sd)
    dg = dG[:, 1:] * gk
    dxp = (dg * (-z / sd)).sum(-1) + dG[:, 0]
    nch = (R + 31) // 32
    pad = nch * 32 - R
    chunks = lambda t: torch.cat([t, t.new_zeros(pad, K)]).reshape(nch, 32, K).sum(1)
    return dict(dxp=dxp, dd2=dxp * g0 if dd2_0 is None else dd2_0 + dxp * g0, part_m=chunks(dg * (z / sd)),
                part_s=chunks(dg * ((z * z - 1) / sd) * sg))


# ---- shapes and inputs shared by the two test files -------------------------------------------------------------------------------
def dims(D, r, QK, nco, ce):
    return dict(D=D, De=D // 4, r=r, QK=QK, nco=nco, ce=ce)


# one case per compiled instantiation of k_chain_c / k_bwd_c and per ragged width (QK = 378: a partial last 32-block of lin_edge0)
DIMS_3D = [dims(128, 2, 126, 3, 8), dims(256, 2, 252, 3, 16), dims(384, 4, 378, 3, 19),
           dims(256, 2, 256, 1, 16), dims(128, 2, 128, 1, 8), dims(384, 4, 384, 1, 19)]
ROWS = (1, 31, 32, 33, 95)


def rand_params(d, seed, two_d=False):
    """The parameters of one block the fused chains read, randn / sqrt(fan_in) (PyTorch layouts), float64."""
    g = torch.Generator().manual_seed(seed)
    D, De, r, QK, ce, nco = d['D'], d['De'], d['r'], d['QK'], d['ce'], d['nco']
    w = lambda o, i: torch.randn(o, i, generator=g, dtype=torch.float64) / math.sqrt(i)
    b = lambda o: torch.randn(o, generator=g, dtype=torch.float64) * 0.5
    P = dict(edge_emb_w=w(De, 2 * De), edge_emb_b=b(De), le0=w(QK, De), le1=w(D, De), ff3_w=w(r * De, De), ff3_b=b(r * De), ff4_w=w(De, r * De),
             ff4_b=b(De), ero_w=w(ce, De), ero_b=b(ce), in_w=w(D, 2 * D + 2 * De), in_b=b(D), c0_w=w(D, D), c0_b=b(D), c2_w=w(nco, D), n2e_b=b(De),
             gbf_means=torch.rand(De - 1, generator=g, dtype=torch.float64) * 3,
             gbf_stds=(0.3 + torch.rand(De - 1, generator=g, dtype=torch.float64)) * torch.where(torch.rand(De - 1, generator=g) < 0.3, -1.0, 1.0))
    return {k: v.float().double() for k, v in P.items()}          # exactly representable in float32: the kernel reads the same numbers


def rand_topo(R, seed, B=7):
    """R edge rows over B molecules of unequal row counts (ids ascending, changing inside 32-row strips; fewer molecules when R < B),
    each with 2 - 5 atoms of its own; edge_a / edge_c random atoms of the row's molecule."""
    g = torch.Generator().manual_seed(seed)
    B = min(B, R)
    cuts = sorted(torch.randperm(R - 1, generator=g)[:B - 1].add(1).tolist()) if B > 1 else []
    counts = [b_ - a_ for a_, b_ in zip([0] + cuts, cuts + [R])]
    nn = torch.randint(2, 6, (B,), generator=g).tolist()
    node_off = np.concatenate([[0], np.cumsum(nn)])
    mol = torch.cat([torch.full((c,), b, dtype=torch.long) for b, c in enumerate(counts)])
    ea = torch.tensor([int(node_off[m]) + int(torch.randint(0, nn[m], (1,), generator=g)) for m in mol.tolist()])
    ec = torch.tensor([int(node_off[m]) + int(torch.randint(0, nn[m], (1,), generator=g)) for m in mol.tolist()])
    return dict(R=R, B=B, Nn=int(node_off[-1]), edge_a=ea, edge_c=ec, edge_mol=mol)


def mol_topo(nn):
    """The training path's own tables of a batch of molecules (dgt_train.hip): R = sum n^2, row (a, c) at edge_off[b] + a n + c."""
    nn = [int(n) for n in nn]
    node_off = np.concatenate([[0], np.cumsum(nn)]).astype(np.int64)
    edge_off = np.concatenate([[0], np.cumsum([n * n for n in nn])]).astype(np.int64)
    ea, ec, em, nm = [], [], [], []
    for b, n in enumerate(nn):
        a = torch.arange(n)
        ea.append((node_off[b] + a[:, None].expand(n, n)).reshape(-1)); ec.append((node_off[b] + a[None, :].expand(n, n)).reshape(-1))
        em.append(torch.full((n * n,), b, dtype=torch.long)); nm.append(torch.full((n,), b, dtype=torch.long))
    return dict(R=int(edge_off[-1]), B=len(nn), Nn=int(node_off[-1]), N=max(nn), nn=nn, node_off=torch.from_numpy(node_off),
                edge_off=torch.from_numpy(edge_off), edge_a=torch.cat(ea), edge_c=torch.cat(ec), edge_mol=torch.cat(em), node_mol=torch.cat(nm))


def randn64(g, *shape, scale=1.0):
    """unit-scale values that float32 holds exactly (the kernel and both restatements start from the same numbers)"""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()
