"""numpy oracle of the two stability rules and of fragments, reading a StabilityRules (jodo_amd/evaluation/rules.py).

3-D rule: for every pair i < j of a molecule's atoms, d = |p_i - p_j| in float32; the ordered type pair is (type[i], type[j]) when
rules.pair_order is 'index' and the pair sorted by type index when it is 'type'; with (t1, t2, t3) = rules.thr[first, second] the order
is 0 unless t1 > 0 and 100 d < t1, then 1 unless t2 > 0 and 100 d < t2, then 2 unless t3 > 0 and 100 d < t3, then 3.  The valence of an
atom is the sum of its pairs' orders; the atom is stable when the valence is in its type's list.
Bond rule: the valence of atom i is the sum over j of edge_type[min(i, j), max(i, j)] for entries 1..3; an entry above 3 (4 = aromatic) is
counted per molecule and enters no valence; the atom is stable when the valence is in the list of (type, charge), a charge the element
does not list reading the element's list for charge 0.
Fragments: connected components over the pairs with an order (entry) above 0; an atom without bonds is one.
"""
import numpy as np


def orders_3d(rules, pos, types):
    """[n, n] integer bond orders of one molecule (symmetric, zero diagonal)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    types = np.asarray(types).astype(np.int64)
    n = len(types)
    diff = pos[:, None, :] - pos[None, :, :]
    d = np.sqrt((diff * diff).sum(-1, dtype=np.float32), dtype=np.float32)
    pm = np.float32(100.) * d
    T = rules.n_types
    known = types < T
    tc = np.minimum(types, T - 1)
    first, second = np.broadcast_to(tc[:, None], (n, n)), np.broadcast_to(tc[None, :], (n, n))
    if rules.pair_order == 'type':
        first, second = np.minimum(first, second), np.maximum(first, second)
    t = rules.thr[first, second].astype(np.float32)             # [n, n, 3]: row i, column j looks (i, j) up — used for i < j only
    o1 = (t[..., 0] > 0) & (pm < t[..., 0]) & known[:, None] & known[None, :]
    o2 = o1 & (t[..., 1] > 0) & (pm < t[..., 1])
    o3 = o2 & (t[..., 2] > 0) & (pm < t[..., 2])
    upper = np.triu(o1.astype(np.int64) + o2 + o3, 1)
    return upper + upper.T


def fragments(adj):
    """number of connected components of a boolean [n, n] adjacency (either triangle may hold a bond)."""
    adj = np.asarray(adj, dtype=bool)
    adj = adj | adj.T
    n = adj.shape[0]
    seen = np.zeros(n, dtype=bool)
    count = 0
    for s in range(n):
        if seen[s]:
            continue
        count += 1
        stack = [s]
        seen[s] = True
        while stack:
            i = stack.pop()
            for j in np.nonzero(adj[i] & ~seen)[0]:
                seen[j] = True
                stack.append(int(j))
    return count


def stability_3d(rules, pos, types):
    """-> dict(stable_atoms, atoms, valence [n], stable [n] bool, orders [n, n], fragments, needs_kekulize = 0)"""
    types = np.asarray(types).astype(np.int64)
    orders = orders_3d(rules, pos, types)
    val = orders.sum(1)
    stable = np.array([t < rules.n_types and int(v) in rules.allowed[min(t, rules.n_types - 1)] for t, v in zip(types, val)], dtype=bool)
    return dict(stable_atoms=int(stable.sum()), atoms=len(types), valence=val, stable=stable, orders=orders,
                fragments=fragments(orders > 0), needs_kekulize=0)


def stability_bonds(rules, types, fc, edge_type):
    """-> dict(stable_atoms, atoms, valence [n], stable [n] bool, fragments, needs_kekulize); the strict upper triangle of edge_type
    only is read."""
    types = np.asarray(types).astype(np.int64)
    n = len(types)
    fc = np.zeros(n, np.int64) if np.asarray(fc).size == 0 else np.asarray(fc).astype(np.int64).reshape(n)
    up = np.triu(np.asarray(edge_type).astype(np.int64).reshape(n, n), 1)
    counted = np.where(up <= 3, up, 0)
    val = counted.sum(0) + counted.sum(1)
    stable = np.zeros(n, dtype=bool)
    for i, (t, q, v) in enumerate(zip(types, fc, val)):
        if t < rules.n_types:
            table = rules.allowed_fc[t]
            stable[i] = int(v) in table.get(int(q), table[0])
    return dict(stable_atoms=int(stable.sum()), atoms=n, valence=val, stable=stable, fragments=fragments(up > 0),
                needs_kekulize=int((up > 3).sum()))


def batch(rules, rule, pos, at, fc, et, n_nodes):
    """Padded batch arrays (the decode's layout) -> (per_mol int [B, 4], totals int [4], orders uint8 [B, N, N] | None); a molecule with
    n <= 0 gets a zero row and counts in no total."""
    B, N = at.shape
    per_mol = np.zeros((B, 4), dtype=np.int64)
    totals = np.zeros(4, dtype=np.int64)
    orders = np.zeros((B, N, N), dtype=np.uint8) if rule == '3d' else None
    for b in range(B):
        n = int(n_nodes[b])
        if n <= 0:
            continue
        if rule == '3d':
            r = stability_3d(rules, pos[b, :n], at[b, :n])
            orders[b, :n, :n] = r['orders']
        else:
            r = stability_bonds(rules, at[b, :n], fc[b, :n], et[b, :n, :n])
        per_mol[b] = (r['stable_atoms'], n, r['fragments'], r['needs_kekulize'])
        totals += (int(r['stable_atoms'] == n), r['stable_atoms'], n, int(r['fragments'] == 1))
    return per_mol, totals, orders
