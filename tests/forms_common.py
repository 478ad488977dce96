"""Shared helpers of the launch-form tests (test_forms_host.py, test_forms_gpu.py, the full-size test of test_dgt_gpu.py): control
over WHICH plan and WHICH scratch a forward runs on.

A forward finds its plan by the storage address of the node mask (`_DGTBase._plan`), and every cached plan keeps its mask alive: a
test that moves its masks to the device on every call gets a new address, hence a new, unpinned plan on freshly zeroed scratch, on
every call.  `DeviceBatch` holds the masks on the device once; `plan_of` + `poison` put finite garbage into a plan's scratch before
any kernel has written it; `strip_order` / `seam_batch` / `seams` restate the node-strip layout of csrc/dgt_plan.cpp so that a
batch can be built to sit exactly on the strip counts at which the node-class launches change form (csrc/dgt_forward.hip,
launch_node_post_256: full rounds of 1024 strips + a remainder of r strips in 4 / 2 / 1 waves)."""
import torch

DEV = 'cuda:0'
ROUND = 1024                       # node strips of one full round of k_node_post (one wave per SIMD)
# strip counts at which launch_node_post_256 changes form (r = strips beyond the full rounds): below the switch | r = 0 | r = 1 |
# last four-wave remainder (r = 256) | first two-wave | last two-wave (r = 512) | first one-wave remainder, unmixed
SEAM_SIZES = (1023, 1024, 1025, 1280, 1281, 1536, 1537)
LIVE_LAST = 27                     # live rows of the last strip in those cases: it has padded lanes

# the plain form of the nf 256 tuned kernel set: every launch merger off, one wave per node strip, never pinned
# (include/jodo_hip.h: 0 FUSE_NEXT_QKV, 2 NODE_POST_WAVES, 7 NODE_MIX, 8 HEADS_MIX, 9 HALF_ROWS, 10 PRE_EMBED, 11 AB_PRE)
PLAIN = {0: 0, 7: 0, 8: 0, 9: 0, 10: 0, 11: 0, 2: 1}


class DeviceBatch:
    """One batch on the device: masks moved ONCE (their address is the plan key), inputs moved once.  `__call__` evaluates a model
    on it; `pin(model)` pins the plan of the last call, and from then on every call asserts AFTER it ran that it really ran on that
    pinned plan."""

    def __init__(self, xh, ex, nl, nm, em, ctx=None, dev=DEV):
        d = lambda x: None if x is None else x.to(dev)
        self.dev = dev
        self.xh, self.ex, self.nl, self.nm, self.em, self.ctx = d(xh), d(ex), d(nl), d(nm), d(em), d(ctx)
        self._pinned = {}                                        # id(model) -> the plan dicts that pin() pinned

    def pin(self, model):
        model.pin_paths()
        plans = list(model._last_plans)
        assert plans and all(p.get('pinned') for p in plans), "pin_paths() left the plan(s) of the last call unpinned"
        self._pinned[id(model)] = plans
        return plans[0]

    def unpin(self, model):
        model.unpin_paths()
        self._pinned.pop(id(model), None)

    def assert_ran_pinned(self, model):
        """After a call: the plan it ran on is pinned and is the very dict that was pinned (not a new plan for a new mask address)."""
        want = self._pinned[id(model)]
        assert model._last_plan.get('pinned'), "the call ran on an unpinned plan (%d plans cached)" % len(model._plans)
        assert model._last_plan is want[0] and len(model._last_plans) == len(want) and all(a is b for a, b in zip(model._last_plans, want)), \
            "the call ran on another plan than the pinned one (%d plans cached)" % len(model._plans)

    def __call__(self, model, cx=None, cex=None, xh=None, ex=None, nl=None, cpu=True):
        d = lambda x: None if x is None else x.to(self.dev)
        nl_ = self.nl if nl is None else d(nl)
        with torch.no_grad():
            o = model(nl_, self.xh if xh is None else d(xh), self.nm, self.em, edge_x=self.ex if ex is None else d(ex), cond_x=d(cx),
                      cond_edge_x=d(cex), noise_level=nl_, context=self.ctx)
        torch.cuda.synchronize()
        if id(model) in self._pinned:
            self.assert_ran_pinned(model)
        return (o[0].cpu(), o[1].cpu()) if cpu else o


def assert_pinned_call(model, plans):
    """For tests with their own call helpers: after a call made under pin_paths(), it ran on the pinned plan dict(s) `plans`."""
    plans = list(plans)
    assert all(p.get('pinned') for p in model._last_plans), "the call ran on an unpinned plan (%d plans cached)" % len(model._plans)
    assert len(model._last_plans) == len(plans) and all(a is b for a, b in zip(model._last_plans, plans)), \
        "the call ran on another plan than the pinned one (%d plans cached)" % len(model._plans)
    assert model._last_plan is plans[0]


def poison(buf, seed):
    """Overwrite a uint8 device buffer with float32 values uniform in [-8, 8] from a seeded generator: finite and of the magnitude of
    real activations, so a row that a launch form forgets to write is read back as plausible data, not as zero."""
    assert buf.dtype == torch.uint8 and buf.is_cuda
    g = torch.Generator(device=buf.device)
    g.manual_seed(int(seed))
    n = buf.numel() // 4
    view = buf[:4 * n].view(torch.float32)
    step = 1 << 26                                               # in pieces: no second buffer of the workspace's size
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        view[lo:hi] = torch.rand(hi - lo, generator=g, device=buf.device, dtype=torch.float32) * 16.0 - 8.0
    if buf.numel() > 4 * n:
        buf[4 * n:] = 0x41
    torch.cuda.synchronize()
    return buf


def fill_nan(buf):
    assert buf.dtype == torch.uint8 and buf.is_cuda
    n = buf.numel() // 4
    buf[:4 * n].view(torch.float32).fill_(float('nan'))
    torch.cuda.synchronize()
    return buf


def plan_of(model, batch):
    """The plan of `batch` BEFORE its first forward (the forward then finds it in the cache): its scratch can be poisoned before any
    kernel has written it."""
    return model._plan(batch.nm, batch.em, batch.nm.device)


def align32(x):
    return (x + 31) // 32 * 32


def strip_order(n_nodes):
    """csrc/dgt_plan.cpp restated: molecules sorted stably by descending size and packed back to back; Nn_pad = align32(sum n); node
    strip s holds packed rows 32 s .. 32 s + 31.  Returns dict(order, Nn, Nn_pad, n_strips, first (packed row of molecule b),
    owners (per strip: the molecules, original indices, that own rows of it, in packed order), atom_strip (strip of every packed
    atom))."""
    n_nodes = [int(n) for n in n_nodes]
    order = sorted(range(len(n_nodes)), key=lambda b: -n_nodes[b])          # sorted() is stable
    Nn = sum(n_nodes)
    Nn_pad = align32(Nn)
    n_strips = Nn_pad // 32
    owners = [[] for _ in range(n_strips)]
    first = [0] * len(n_nodes)
    atom_strip = []
    v = 0
    for b in order:
        first[b] = v
        for s in range(v // 32, (v + n_nodes[b] - 1) // 32 + 1):
            owners[s].append(b)
        atom_strip.extend((v + i) // 32 for i in range(n_nodes[b]))
        v += n_nodes[b]
    return dict(order=order, Nn=Nn, Nn_pad=Nn_pad, n_strips=n_strips, first=first, owners=owners, atom_strip=atom_strip)


def straddler(n_nodes, boundary=ROUND):
    """The molecule with rows on both sides of the strip boundary (strips boundary - 1 and boundary), or None."""
    so = strip_order(n_nodes)
    if so['n_strips'] <= boundary:
        return None
    both = [b for b in so['owners'][boundary - 1] if b in so['owners'][boundary]]
    assert len(both) <= 1
    return both[0] if both else None


SPLIT_GATE_PATTERN = [29, 17, 23, 12, 9, 28, 19, 21, 18, 20]     # the repeating sizes of test_split_gate.py's 1805-molecule case


def seam_batch(S, live_last):
    """A QM9-sized list of atom counts (1 .. 29) with exactly S node strips and `live_last` live rows in the last one; whenever
    S > 1024 one molecule straddles strips 1023 and 1024.  The repeating pattern of test_split_gate trimmed, topped up with small
    molecules (always a 3, a 2 and a 1, so that the last strip holds the smallest sizes), in the pattern's order with the top-up
    at the end — the plan sorts by size itself."""
    assert S >= 2 and 1 <= live_last <= 32
    target = (S - 1) * 32 + live_last
    base = []
    while sum(base) + SPLIT_GATE_PATTERN[len(base) % 10] <= target - 6:
        base.append(SPLIT_GATE_PATTERN[len(base) % 10])
    for drop in range(0, 40):
        body = base[:len(base) - drop]
        rest = target - 6 - sum(body)
        top = []
        # the remainder as molecules of 9 .. 15 atoms first (sizes that sort behind the pattern's bulk), then one smaller piece
        k = 9 + drop % 7
        while rest >= k + 1:
            top.append(k)
            rest -= k
        if rest:
            top.append(rest)
        n_nodes = body + top + [3, 2, 1]
        if max(n_nodes) > 29 or min(n_nodes) < 1 or sum(n_nodes) != target:
            continue
        if S <= ROUND or straddler(n_nodes) is not None:
            return n_nodes
    raise AssertionError("no seam batch for S = %d, live_last = %d" % (S, live_last))


def seams(n_nodes):
    """The molecules (original indices, ascending) that own rows in strips 0, 1023, 1024 and n_strips - 1, plus the molecule that
    straddles 1023 / 1024: where a launch form that mis-places its strip base, its remainder or its Gram-tile prefix goes wrong first."""
    so = strip_order(n_nodes)
    pick = set()
    for s in (0, ROUND - 1, ROUND, so['n_strips'] - 1):
        if 0 <= s < so['n_strips']:
            pick.update(so['owners'][s])
    st = straddler(n_nodes)
    if st is not None:
        pick.add(st)
    return sorted(pick)


def sub_batch(idx, n_nodes, *tensors):
    """Molecules `idx` cut out of batch tensors ([B, N, ..] node-shaped or [B, N, N, ..] edge-shaped; None and [B] / [B, c] pass
    through by row) and trimmed to the sub-batch's own padded width.  Returns (atom counts, [cut tensors])."""
    pn = [int(n_nodes[b]) for b in idx]
    Ns, N = max(pn), max(int(n) for n in n_nodes)
    out = []
    for t in tensors:
        if t is None:
            out.append(None)
        elif t.dim() >= 4 and t.shape[1] == N and t.shape[2] == N:
            out.append(t[idx][:, :Ns, :Ns])
        elif t.dim() == 3 and t.shape[1] == N:
            out.append(t[idx][:, :Ns])
        else:
            out.append(t[idx])
    return pn, out
