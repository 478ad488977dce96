"""CPU: the sharded 2-D sampling function through its private builder (the seam `_get_sampling_fn_2d` takes a CPU device for `shard=` with
torch-drawn noise; the model is the dense oracle tests/oracle2d.OracleModel2D), world size 2 over gloo; the gather of rounds without
positions; the public entry's refusal of the GPU-only options on a CPU device."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

SEED, BATCH, SAMPLES, STEPS = 77, 5, 9, 3


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup():
    from helpers import make_config, make_model, state_dict_cpu, GOLDEN
    from jodo_amd.diffusion.noise_schedule import NoiseScheduleVP
    from jodo_amd.models import get_node_dist
    from jodo_amd.utils import get_data_inverse_scaler
    import oracle2d as O2
    cfg = make_config('vpsde_zinc_2d_jodo')
    cfg.device = 'cpu'
    cfg.sampling.steps = STEPS
    model = O2.OracleModel2D(state_dict_cpu(make_model(cfg, 5, head_gain=30.0)), O2.Hyper2D.from_config(cfg))
    ns = NoiseScheduleVP(cfg.sde.schedule, continuous_beta_0=cfg.sde.continuous_beta_0, continuous_beta_1=cfg.sde.continuous_beta_1)
    nodes_dist = get_node_dist(O2.load_n_nodes_hist(os.path.join(GOLDEN, 'n_nodes_2d.json'), 'zinc250k'))
    return cfg, model, ns, nodes_dist, get_data_inverse_scaler(cfg)


def _builder(cfg, ns, nodes_dist, inv, **kw):
    from jodo_amd.sampling import _get_sampling_fn_2d
    return _get_sampling_fn_2d(cfg, ns, nodes_dist, BATCH, SAMPLES, inv, 1e-3, **kw)


def _by_value(m):
    return tuple(None if t is None else t.numpy().copy() for t in m)


def _sample_worker(rank, world, port, mode, assign, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from jodo_amd.dist import gather_sampled
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg, model, ns, nodes_dist, inv = _setup()
    torch.manual_seed(1234 + rank)                       # whatever the process did before must not matter
    fn = _builder(cfg, ns, nodes_dist, inv, shard=(rank, world), shard_mode=mode, shard_assign=assign, seed=SEED)
    mols = fn(model)
    full = gather_sampled(fn.last_decoded, fn.last_indices)
    assert len(mols) == len(fn.last_indices)
    assert all(r[0] is None for r in fn.last_decoded)
    q.put((rank, fn.last_indices, [_by_value(m) for m in full]))      # by value (no shared-memory handles)
    dist.barrier()
    dist.destroy_process_group()


def _run_world2(mode, assign='contiguous'):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sample_worker, args=(r, 2, port, mode, assign, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    return [(r, idx, [tuple(None if a is None else torch.from_numpy(a) for a in m) for m in mols]) for r, idx, mols in res]


def _same(a, b):
    eq = lambda x, y: (x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y))
    return len(a) == len(b) and all(len(m) == len(w) and all(eq(x, y) for x, y in zip(m, w)) for m, w in zip(a, b))


def test_sharded_2d_sampling_parity_mode_reproduces_the_unsharded_run():
    """world 2, shard_mode='parity': the gathered molecules equal the world-size-1 unsharded run bit for bit; 9 samples in rounds of 5."""
    threads = torch.get_num_threads()
    torch.set_num_threads(2)                  # as the workers: CPU GEMM blocking (hence low bits) depends on the thread count
    try:
        cfg, model, ns, nodes_dist, inv = _setup()
        torch.manual_seed(SEED)
        want = _builder(cfg, ns, nodes_dist, inv, return_raw=True)(model)                   # the reference's procedure
        one = _builder(cfg, ns, nodes_dist, inv, shard=(0, 1), shard_mode='parity', seed=SEED)
        got1 = one(model)
        assert one.last_indices == list(range(10)) and _same(got1, want)
        res = _run_world2('parity')
        assert sorted(res[0][1] + res[1][1]) == list(range(10)) and not set(res[0][1]) & set(res[1][1])
        assert res[0][1] == [0, 1, 2, 5, 6, 7]                  # contiguous slice of every round
        for _, _, full in res:
            assert _same(full, want)
        assert all(m[0] is None for m in want) and len({int(m[1].shape[0]) for m in want}) > 1      # 2-D tuples, not a degenerate batch
    finally:
        torch.set_num_threads(threads)


def test_sharded_2d_sampling_perf_mode_rng_contract_and_lpt():
    """shard_mode='perf': molecules are dealt before rounds are cut, atom counts come from the shared seed whatever the ranks' prior RNG
    state, both ranks hold the same gathered list in global order, `lpt` deals by assign_lpt."""
    from jodo_amd.dist import assign_lpt
    res = _run_world2('perf')
    assert res[0][1] == list(range(0, 5)) and res[1][1] == list(range(5, 10))
    assert _same(res[0][2], res[1][2])
    cfg, model, ns, nodes_dist, inv = _setup()
    torch.manual_seed(SEED)
    n_all = nodes_dist.sample(10).tolist()
    assert [int(m[1].shape[0]) for m in res[0][2]] == n_all     # shared-seed atom counts, global order restored
    assert all(m[0] is None for m in res[0][2])
    lpt = _run_world2('perf', 'lpt')
    assert sorted(lpt[0][1] + lpt[1][1]) == list(range(10))
    assert [int(m[1].shape[0]) for m in lpt[0][2]] == n_all and _same(lpt[0][2], lpt[1][2])
    assert assign_lpt(n_all, 2) == [lpt[0][1], lpt[1][1]]


def test_gather_sampled_without_positions_world1():
    from jodo_amd.dist import gather_sampled
    g = torch.Generator().manual_seed(3)
    n = torch.tensor([4, 2, 7], dtype=torch.int32)
    B, N = 3, 7
    at = torch.randint(0, 9, (B, N), generator=g).to(torch.uint8)
    ch = torch.randint(-1, 2, (B, N), generator=g).to(torch.int8)
    bd = torch.randint(0, 4, (B, N, N), generator=g).to(torch.uint8)
    pos = torch.randn(B, N, 3, generator=g)
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % _free_port(), rank=0, world_size=1)
    try:
        two_d = gather_sampled([(None, at[:2], ch[:2], bd[:2], n[:2]), (None, at[2:], ch[2:], bd[2:], n[2:])], [2, 0, 1])
        three_d = gather_sampled([(pos, at, ch, bd, n)], [2, 0, 1])
        empty = gather_sampled([], [], with_pos=False)
        with pytest.raises(ValueError):
            gather_sampled([(None, at[:2], ch[:2], bd[:2], n[:2]), (pos[2:], at[2:], ch[2:], bd[2:], n[2:])], [2, 0, 1])
    finally:
        dist.destroy_process_group()
    assert empty == [] and len(two_d) == len(three_d) == 3
    for out_k, src in zip((2, 0, 1), range(3)):              # molecule `src` carries global index [2, 0, 1][src]
        k = int(n[src])
        for m in (two_d[out_k], three_d[out_k]):
            assert torch.equal(m[1], at[src, :k].long()) and torch.equal(m[2], bd[src, :k, :k].float()) and torch.equal(m[3], ch[src, :k].long())
        assert two_d[out_k][0] is None
        assert torch.equal(three_d[out_k][0], pos[src, :k])   # the 3-D tuple is what it was


def test_public_entry_refuses_the_gpu_options_on_a_cpu_device():
    from jodo_amd import sampling as S
    cfg, model, ns, nodes_dist, inv = _setup()
    for kw in (dict(shard=(0, 2)), dict(hip_graph=True), dict(device_noise=True)):
        with pytest.raises(NotImplementedError, match='needs a GPU device'):
            S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, **kw)
    for kw in (dict(hip_graph=True), dict(device_noise=True)):  # the seam takes shard= only
        with pytest.raises(NotImplementedError, match='needs a GPU device'):
            _builder(cfg, ns, nodes_dist, inv, **kw)
    S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv, device_noise=False)      # nothing asked for: still builds
    cfg.sampling.method = 'fast'
    with pytest.raises(NotImplementedError, match='fast'):
        S.get_sampling_fn(cfg, ns, nodes_dist, 4, 4, inv)
