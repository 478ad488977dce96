"""ctypes binding of libjodo_hip.so (the C ABI declared in include/jodo_hip.h).

The product path has no CPU fallback: if the shared library is missing or a symbol cannot be
resolved, importing callers get a RuntimeError that says how to build it (`python -c "import
__graft_entry__ as g; g.build()"`).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# JODO_HIP_LIB: A/B experiments of tools/ load another build of the same library (csrc/Makefile LIB=...); tests and the
# driver never set it
LIB_PATH = os.environ.get('JODO_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libjodo_hip.so')
_lib = None


class JodoHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise JodoHipError(
                "libjodo_hip.so not found at %s — the HIP extension is required (no CPU fallback). "
                "Build it with: python -c 'import __graft_entry__ as g; g.build()'" % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.jodo_last_error.restype = ctypes.c_char_p
        _bind_2d_sampling(_lib)
        _bind_2d_pair(_lib)
        _bind_2d_split(_lib)
        _bind_egnn(_lib)
        _bind_eval(_lib)
        _bind_geometry(_lib)
        _bind_cdgs(_lib)
        _bind_prop(_lib)
    return _lib


def _bind_2d_sampling(L):
    """Argument types of the 2-D round's caller-side exports (include/jodo_hip.h): a library without them is an error here, not at
    the first sampling step."""
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    try:
        step, dec, dpm = L.jodo_sampler_step_2d_rng, L.jodo_decode_2d, L.jodo_dpm_update_2d
    except AttributeError as e:
        raise JodoHipError("%s lacks the 2-D sampling exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    step.argtypes = [i, i, i, i, p, f, f, f, p, p, ctypes.c_uint64, ctypes.c_uint32] + [p] * 9
    dec.argtypes = [i] * 7 + [f, f, f] + [p] * 7
    dpm.argtypes = [i, i, i, i, p, p, p, p, i, i] + [p] * 11
    step.restype = dec.restype = dpm.restype = i
    try:                                                     # the noise-prediction form of the 2-D solver (CDGS under 'dpm_2d')
        e2d, beg = L.jodo_eps_to_data_2d, L.jodo_step_begin_t
    except AttributeError as e:
        raise JodoHipError("%s lacks the noise-form exports of the 2-D solver (%s): rebuild it with python -c 'import __graft_entry__ as g; "
                           "g.build()'" % (LIB_PATH, e))
    e2d.argtypes = [i, i, i, i, p, f, f, p, p, i, i] + [p] * 7
    beg.argtypes = [i, p, p, i, i, p, p, p]
    e2d.restype = beg.restype = i


PROP_MAX_PROPS, PROP_MAX_BINS = 16, 65536       # JODO_PROP_MAX_PROPS, JODO_PROP_MAX_BINS


def _bind_prop(L):
    """Argument types of the property prior's draw (jodo_prop_sample; include/jodo_hip.h)."""
    i, p, u64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64
    try:
        ps = L.jodo_prop_sample
    except AttributeError as e:
        raise JodoHipError("%s lacks the property-prior export (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    ps.argtypes = [i, i, i, i, p, p, p, p, p, p, u64, u64, p, p, p]
    ps.restype = i


WALK_DIRECTED, WALK_PAIR = 0, 1                 # enum jodo2d_walk


def _bind_2d_pair(L):
    """Argument types of the pair-walk exports of the 2-D model (jodo_dgt2d_pair_layout, jodo_dgt2d_pair_fill_desc,
    jodo_dgt2d_forward_walk; include/jodo_hip.h)."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        lay, fill, fwd = L.jodo_dgt2d_pair_layout, L.jodo_dgt2d_pair_fill_desc, L.jodo_dgt2d_forward_walk
    except AttributeError as e:
        raise JodoHipError("%s lacks the 2-D pair-walk exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    lay.argtypes = [p, i, i, p, p]
    fill.argtypes = [p, i, i, p, p, ctypes.c_int64]
    fwd.argtypes = [p, i, i, p, p, p, i, p, p, i] + [p] * 9 + [i, i, p]
    lay.restype = fill.restype = fwd.restype = i


def _bind_2d_split(L):
    """Argument types of the 2-D model's split-bf16 exports (jodo_dgt2d_split_size, jodo_dgt2d_pack_split_host,
    jodo_dgt2d_forward_split, jodo_debug_gemm2d; include/jodo_hip.h)."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        size, pack, fwd, dbg = L.jodo_dgt2d_split_size, L.jodo_dgt2d_pack_split_host, L.jodo_dgt2d_forward_split, L.jodo_debug_gemm2d
    except AttributeError as e:
        raise JodoHipError("%s lacks the 2-D split-bf16 exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    size.argtypes = [p, p, p, i]
    pack.argtypes = [p, p, p, i, p, ctypes.c_size_t]
    fwd.argtypes = [p, i, i, p, p, p, i, p, p, i, p, p] + [p] * 9 + [i, i, p]
    dbg.argtypes = [i, p, i, i, i, p, p, i, p, p]
    size.restype = pack.restype = fwd.restype = dbg.restype = i


def _bind_egnn(L):
    """Argument types of the property classifier's exports (jodo_egnn_*; include/jodo_hip.h, section "property classifier")."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        chk, size, pack, lay, fill, fwd = (L.jodo_egnn_check_cfg, L.jodo_egnn_packed_size, L.jodo_egnn_pack_weights_host, L.jodo_egnn_layout,
                                           L.jodo_egnn_fill_desc, L.jodo_egnn_forward)
    except AttributeError as e:
        raise JodoHipError("%s lacks the property-classifier exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    chk.argtypes = [p]
    size.argtypes = [p, p, p]
    pack.argtypes = [p, p, i, p, ctypes.c_size_t, p, i]
    lay.argtypes = [p, i, i, p, p]
    fill.argtypes = [p, i, i, p, p, ctypes.c_int64]
    fwd.argtypes = [p, i, i, p, p, p, p, i, p, p, p, p, i, p]
    chk.restype = size.restype = pack.restype = lay.restype = fill.restype = fwd.restype = i


PAIR_BY_INDEX, PAIR_BY_TYPE = 0, 1              # enum jodo_pair_order


def _bind_eval(L):
    """Argument types of the stability exports (jodo_stability_3d, jodo_stability_bonds; include/jodo_hip.h, section "evaluation")."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        s3, sb = L.jodo_stability_3d, L.jodo_stability_bonds
    except AttributeError as e:
        raise JodoHipError("%s lacks the stability exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    s3.argtypes = [i, i, i, i] + [p] * 9
    sb.argtypes = [i, i, i, i, i] + [p] * 8
    s3.restype = sb.restype = i


GEOMETRY_MAX_CLASSES, MMD_TILE = 32, 1024       # JODO_GEOMETRY_MAX_CLASSES, JODO_MMD_TILE


def _bind_geometry(L):
    """Argument types of the geometry exports (jodo_geometry_count, jodo_geometry_write, jodo_mmd_batched; include/jodo_hip.h, section
    "sub-structure geometry")."""
    i, p, d, q = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int64
    try:
        cnt, wr, mmd = L.jodo_geometry_count, L.jodo_geometry_write, L.jodo_mmd_batched
    except AttributeError as e:
        raise JodoHipError("%s lacks the geometry exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    cnt.argtypes = [i] * 5 + [p] * 13
    wr.argtypes = [i] * 5 + [p] * 12 + [q, q, q, p]
    mmd.argtypes = [i, i] + [p] * 5 + [d, i, d] + [p] * 4
    cnt.restype = wr.restype = mmd.restype = i


def _bind_cdgs(L):
    """Argument types of the CDGS exports (jodo_cdgs_*; include/jodo_hip.h, section "CDGS")."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        chk, size, pack, lay, fill, fwd = (L.jodo_cdgs_check_cfg, L.jodo_cdgs_packed_size, L.jodo_cdgs_pack_weights_host, L.jodo_cdgs_layout,
                                           L.jodo_cdgs_fill_desc, L.jodo_cdgs_forward)
    except AttributeError as e:
        raise JodoHipError("%s lacks the CDGS exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    chk.argtypes = [p]
    size.argtypes = [p, p, p]
    pack.argtypes = [p, p, i, p, ctypes.c_size_t, p, i]
    lay.argtypes = [p, i, i, p, p]
    fill.argtypes = [p, i, i, p, p, ctypes.c_int64]
    fwd.argtypes = [p, i, i, p, p, p, p, i] + [p] * 6 + [i, p]
    chk.restype = size.restype = pack.restype = lay.restype = fill.restype = fwd.restype = i
    _bind_cdgs_split(L)
    bind_cdgs_train(L)
    try:                                                     # the training GEMM's split-bf16 form on its own (tests, tools)
        gs = L.jodo_train_gemm_s
    except AttributeError as e:
        raise JodoHipError("%s lacks the split-bf16 training GEMM (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    gs.argtypes = [i] * 5 + [p, i, p, i, p, i, p, i, i, p, p, ctypes.c_float, ctypes.c_uint64, i, p, ctypes.c_size_t, p]
    gs.restype = i


def _bind_cdgs_split(L):
    """Argument types of the CDGS split-bf16 exports (jodo_cdgs_split_size, jodo_cdgs_pack_split_host, jodo_cdgs_forward_split,
    jodo_debug_gemm_cdgs; include/jodo_hip.h)."""
    i, p = ctypes.c_int, ctypes.c_void_p
    try:
        size, pack, fwd, dbg = L.jodo_cdgs_split_size, L.jodo_cdgs_pack_split_host, L.jodo_cdgs_forward_split, L.jodo_debug_gemm_cdgs
    except AttributeError as e:
        raise JodoHipError("%s lacks the CDGS split exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    size.argtypes = [p, p, p, i]
    pack.argtypes = [p, p, p, i, p, ctypes.c_size_t]
    fwd.argtypes = [p, i, i, p, p, p, p, i] + [p] * 6 + [i, p] + [p, p, p]
    dbg.argtypes = [i, i, p, i, i, p, p, p, i, i, i, i, p, p, i, p, i, p, p, i, p]
    size.restype = pack.restype = fwd.restype = dbg.restype = i


def bind_cdgs_train(L):
    """Argument types of the CDGS training exports (jodo_cdgs_train_*; include/jodo_hip.h, section "CDGS training").  Also applied by
    jodo_amd.train.TrainEngineCDGS to a library handed to it (the host build of the same source the CPU suite drives)."""
    i, p, f, u64, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t
    try:
        create, destroy, dbytes, wbytes, dhost, upload, setopt, getopt, locate, fwd, bwd = (getattr(L, 'jodo_cdgs_train_' + n) for n in (
            'create', 'destroy', 'desc_bytes', 'workspace_bytes', 'desc_host', 'upload', 'set_option', 'get_option', 'debug_locate', 'forward',
            'backward'))
    except AttributeError as e:
        raise JodoHipError("the library lacks the CDGS training exports (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'" % e)
    create.argtypes = [p, i, i, p, p, i, p]
    destroy.argtypes = dbytes.argtypes = wbytes.argtypes = dhost.argtypes = [p]
    upload.argtypes = [p, p, p]
    setopt.argtypes = [p, i, i]
    getopt.argtypes = [p, i, p]
    locate.argtypes = [p, i, i, p, p]
    fwd.argtypes = [p, p, p, i, p, p, p, p, f, u64, p, p, p, p]
    bwd.argtypes = [p, p, p, p, i, p, p, p, p, f, u64, p, p]
    L.jodo_cdgs_train_debug_drop.argtypes = [f, u64, i, ctypes.c_int64, i, i, p, p]
    L.jodo_cdgs_train_debug_drop.restype = i
    create.restype = upload.restype = setopt.restype = getopt.restype = locate.restype = fwd.restype = bwd.restype = i
    destroy.restype = None
    dbytes.restype = wbytes.restype = z
    dhost.restype = p


# ---- tests: jodo_train_debug_fused (include/jodo_hip.h; csrc/train_debug.hip) — one fused training kernel on caller-owned arrays.
# The two name lists are the header's enums in order (tests/test_fused_kernels_host.py reads the header and compares).
FT_OPS = ('PACK', 'PACK_BWD', 'PACK_2D', 'PACK_2D_BWD', 'CHAIN_A', 'CHAIN_B', 'CHAIN_C', 'BWD_A', 'BWD_B', 'BWD_C', 'CHAIN_A_2D', 'BWD_A_2D',
          'NODE_LN_MOD', 'NODE_LN_MOD_BWD', 'ATTN_FWD', 'ATTN_BWD', 'GBF_BWD')
FT_SLOTS = ('EDGE_EMB_W', 'EDGE_EMB_B', 'LE0', 'LE1', 'FF3_W', 'FF3_B', 'FF4_W', 'FF4_B', 'ERO_W', 'ERO_B', 'IN_W', 'IN_B', 'C0_W', 'C0_B', 'C2_W',
            'N2E_B', 'GBF_MEANS', 'GBF_STDS', 'PACKED', 'POS', 'GM', 'E_IN', 'EMOD', 'D2', 'G', 'XH', 'RS', 'ET', 'T0', 'T1', 'N2E', 'EN', 'F3', 'A3',
            'F4', 'E_OUT', 'EH', 'HR', 'HC', 'QMOD', 'U', 'C0PRE', 'C0A', 'INV', 'DINV', 'DC0', 'DU', 'DPRE', 'DE', 'DG', 'DE_OUT', 'F4D', 'DF4',
            'DHID', 'DEN', 'DE_PREV', 'DT1', 'DT0', 'DET', 'DE1', 'MODS', 'Q', 'K', 'V', 'ADJ2D', 'ADJSP', 'ALPHA', 'HHAT', 'DHHAT', 'DS', 'DQ', 'DK',
            'DV', 'DXP', 'DD2', 'PART_M', 'PART_S')
FT_TOPO = ('edge_a', 'edge_c', 'edge_mol', 'row_mol', 'node_mol', 'nn', 'node_off', 'edge_off')


class FusedTestArgs(ctypes.Structure):
    """jodo_fused_test_args"""
    _fields_ = ([(k, ctypes.c_int32) for k in (
        'op', 'D', 'De', 'r', 'QK', 'ce', 'nco', 'R', 'Nn', 'B', 'N', 'save', 'H', 'XH', 'SC', 'one_wave', 'ldqk', 'ldv', 'ldd_qk', 'ldd_v', 'ld_eh',
        'eh_col', 'ldm', 'g_off', 'sh_off', 'sc_off', 'acc', 'ldg', 'gcol', 'site_a3', 'site_f4')]
                + [('drop_p', ctypes.c_float), ('inv_sqrt_c', ctypes.c_float), ('seed', ctypes.c_uint64)]
                + [(k, ctypes.c_void_p) for k in FT_TOPO]
                + [('topo_dev', ctypes.c_void_p), ('topo_dev_count', ctypes.c_size_t),
                   ('a', ctypes.c_void_p * len(FT_SLOTS)), ('n', ctypes.c_size_t * len(FT_SLOTS))])


def train_debug_fused(args, stream=None):
    """jodo_train_debug_fused(args) -> its return code (0, or a negative JODO_ERR_* with the text in jodo_last_error())."""
    L = lib()
    try:
        fn = L.jodo_train_debug_fused
    except AttributeError as e:
        raise JodoHipError("%s lacks the fused-kernel test entry (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    fn.argtypes = [ctypes.POINTER(FusedTestArgs), ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(args), stream if stream is not None else ctypes.c_void_p(0))


# ---- tests: jodo_egnn_debug_edge (include/jodo_hip.h; csrc/egnn_train.hip) — one fused edge kernel of the classifier on caller-owned
# arrays.  The two name lists are the header's JODO_ET_* enums in order (tests/test_egnn_kernels_host.py reads the header and compares).
ET_OPS = ('OP_FWD', 'OP_BWD')
ET_SLOTS = ('P', 'XC', 'DAGG', 'WR', 'W2', 'B2', 'WA', 'BA', 'DESC', 'IMG', 'AGG', 'EA', 'EZ2', 'EZ1', 'DP', 'Q', 'QB')


class EgnnEdgeTestArgs(ctypes.Structure):
    """jodo_egnn_edge_test_args"""
    _fields_ = ([(k, ctypes.c_int32) for k in ('op', 'nf', 'B', 'grid_cap')] + [('n_nodes', ctypes.c_void_p)]
                + [('a', ctypes.c_void_p * len(ET_SLOTS)), ('n', ctypes.c_size_t * len(ET_SLOTS))])


def egnn_debug_edge(args, stream=None):
    """jodo_egnn_debug_edge(args) -> its return code (0, or a negative JODO_ERR_* with the text in jodo_last_error())."""
    L = lib()
    try:
        fn = L.jodo_egnn_debug_edge
    except AttributeError as e:
        raise JodoHipError("%s lacks the edge-kernel test entry (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH, e))
    fn.argtypes = [ctypes.POINTER(EgnnEdgeTestArgs), ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(args), stream if stream is not None else ctypes.c_void_p(0))


# ---- tests: jodo_cdgs_train_debug_op (include/jodo_hip.h; csrc/cdgs_train.hip) — one launch sequence of the CDGS training step on
# caller-owned arrays.  The two name lists are the header's JODO_CT_* enums in order (tests/test_cdgs_kernels_host.py reads the header and
# compares).
CT_OPS = ('OP_RW', 'OP_ADDT', 'OP_SCALE', 'OP_RELU', 'OP_RELU_BWD', 'OP_PAIR', 'OP_PAIR_BWD', 'OP_OUT_NODES', 'OP_OUT_EDGES', 'OP_SUMS', 'OP_GINE',
          'OP_GINE_BWD', 'OP_GN_FWD', 'OP_GN_BWD', 'OP_EGN_FWD', 'OP_EGN_BWD', 'OP_NORM_GRADS', 'OP_ATTN_FWD', 'OP_ATTN_BWD')
CT_SLOTS = ('EDGE_X', 'ADJ', 'AD', 'PA', 'PB', 'CNT', 'ONEHOT', 'LAND', 'DEG', 'X', 'TB', 'Y', 'Z', 'EPS', 'HS', 'HE', 'AGG', 'DAGG', 'DHE', 'DHS', 'H', 'A',
            'GAMMA', 'BETA', 'XHAT', 'RSTD', 'DY', 'DX', 'PART', 'GSUM', 'DBETA', 'DGAMMA', 'Q', 'K', 'V', 'G0', 'G1', 'ALPHA', 'ATT', 'DATT', 'DV', 'DAL',
            'DT1', 'DT0', 'DQ', 'DK')


class CdgsOpTestArgs(ctypes.Structure):
    """jodo_cdgs_op_test_args"""
    _fields_ = ([(k, ctypes.c_int32) for k in ('op', 'B', 'N', 'D', 'H', 'F', 'K', 'ch', 'mode', 'acc', 'amask', 'drop_site')]
                + [('isc', ctypes.c_float), ('drop_p', ctypes.c_float), ('drop_seed', ctypes.c_uint64), ('rows', ctypes.c_int64),
                   ('n_nodes', ctypes.c_void_p), ('nn_dev', ctypes.c_void_p), ('nn_dev_count', ctypes.c_size_t),
                   ('a', ctypes.c_void_p * len(CT_SLOTS)), ('n', ctypes.c_size_t * len(CT_SLOTS))])


def cdgs_debug_op(args, stream=None, library=None):
    """jodo_cdgs_train_debug_op(args) -> its return code (0, or a negative JODO_ERR_* with the text in jodo_last_error()).  library: a
    handle to call instead of libjodo_hip.so (the host build of the same source the CPU suite drives)."""
    L = lib() if library is None else library
    try:
        fn = L.jodo_cdgs_train_debug_op
    except AttributeError as e:
        raise JodoHipError("%s lacks the CDGS kernel test entry (%s): rebuild it with python -c 'import __graft_entry__ as g; g.build()'"
                           % (LIB_PATH if library is None else 'the given library', e))
    fn.argtypes = [ctypes.POINTER(CdgsOpTestArgs), ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(args), stream if stream is not None else ctypes.c_void_p(0))


def check(code, what=''):
    if code != 0:
        msg = lib().jodo_last_error()
        raise JodoHipError("%s failed (%d): %s" % (what, code, msg.decode() if msg else ''))


def ptr(t):
    """device/host pointer of a torch tensor (or None) as c_void_p"""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class JodoTensor(ctypes.Structure):             # jodo_tensor (include/jodo_hip.h)
    _fields_ = [('name', ctypes.c_char_p), ('data', ctypes.c_void_p), ('shape', ctypes.POINTER(ctypes.c_int64)),
                ('ndim', ctypes.c_int32)]


_PACKED_SIZE = {}


def _marshal(state_dict):
    """state_dict (values on any device) -> (jodo_tensor array of named fp32 host tensors, the list that keeps their storage alive
    for as long as the array is used)."""
    import numpy as np
    keep, arr = [], (JodoTensor * len(state_dict))()
    for i, (k, v) in enumerate(state_dict.items()):
        t = np.ascontiguousarray(v.detach().float().cpu().numpy())
        shp = (ctypes.c_int64 * max(t.ndim, 1))(*t.shape)
        name = k.encode()
        keep.append((t, shp, name))
        arr[i] = JodoTensor(name, t.ctypes.data_as(ctypes.c_void_p), shp, t.ndim)
    return arr, keep


def pack_weights(cfg_struct, state_dict, device=None):
    """state_dict (reference key names; values on any device) -> (blob, woff ctypes int64 array, n_woff) through the
    C packer jodo_dgt_pack_weights[_host].  device=None: blob is a CPU torch tensor; otherwise it is packed straight
    into a device tensor (one host->device copy of the blob inside the call)."""
    import torch
    L = lib()
    arr, keep = _marshal(state_dict)
    # the packed size depends on the configuration only; asking for it runs the whole packer (QR factorisations included), so it
    # is asked once per configuration — a missing or mis-sized tensor is still a named error of the packing call below
    key = bytes(cfg_struct)
    n_floats, n_woff = ctypes.c_size_t(), ctypes.c_int()
    if key in _PACKED_SIZE:
        n_floats.value, n_woff.value = _PACKED_SIZE[key]
    else:
        check(L.jodo_dgt_packed_size(ctypes.byref(cfg_struct), arr, len(keep), ctypes.byref(n_floats), ctypes.byref(n_woff)),
              'jodo_dgt_packed_size')
        _PACKED_SIZE[key] = (n_floats.value, n_woff.value)
    woff = (ctypes.c_int64 * n_woff.value)()
    if device is None:
        blob = torch.empty(n_floats.value, dtype=torch.float32)
        check(L.jodo_dgt_pack_weights_host(ctypes.byref(cfg_struct), arr, len(keep), ctypes.c_void_p(blob.data_ptr()),
                                           ctypes.c_size_t(n_floats.value), woff, n_woff.value), 'jodo_dgt_pack_weights_host')
    else:
        blob = torch.empty(n_floats.value, dtype=torch.float32, device=device)
        check(L.jodo_dgt_pack_weights(ctypes.byref(cfg_struct), arr, len(keep), ctypes.c_void_p(blob.data_ptr()),
                                      ctypes.c_size_t(n_floats.value), woff, n_woff.value, current_stream_ptr()),
              'jodo_dgt_pack_weights')
    return blob, woff, n_woff.value


def _pack_host(abi, cfg_struct, state_dict, device):
    """(blob, woff ctypes int64 array, n_woff) through <abi>_packed_size / <abi>_pack_weights_host: the packers that take the
    configuration alone for the size and pack on the host."""
    import torch
    L = lib()
    arr, keep = _marshal(state_dict)
    n_floats, n_woff = ctypes.c_size_t(), ctypes.c_int()
    check(getattr(L, abi + '_packed_size')(ctypes.byref(cfg_struct), ctypes.byref(n_floats), ctypes.byref(n_woff)), abi + '_packed_size')
    woff = (ctypes.c_int64 * n_woff.value)()
    blob = torch.empty(n_floats.value, dtype=torch.float32)
    check(getattr(L, abi + '_pack_weights_host')(ctypes.byref(cfg_struct), arr, len(keep), ctypes.c_void_p(blob.data_ptr()),
                                                 ctypes.c_size_t(n_floats.value), woff, n_woff.value), abi + '_pack_weights_host')
    return (blob if device is None else blob.to(device)), woff, n_woff.value


def pack_weights_2d(cfg_struct, state_dict, device=None):
    """The 2-D model's state_dict -> (blob, woff ctypes int64 array, n_woff) through jodo_dgt2d_pack_weights_host; device=None keeps
    the blob on the CPU, otherwise it is copied to `device`."""
    return _pack_host('jodo_dgt2d', cfg_struct, state_dict, device)


def pack_weights_egnn(cfg_struct, state_dict, device=None):
    """The property classifier's state_dict -> (blob, woff ctypes int64 array, n_woff) through jodo_egnn_pack_weights_host;
    device=None keeps the blob on the CPU, otherwise it is copied to `device`."""
    return _pack_host('jodo_egnn', cfg_struct, state_dict, device)


def pack_weights_cdgs(cfg_struct, state_dict, device=None):
    """The CDGS state_dict (plus the caller's 'time_freq') -> (blob, woff ctypes int64 array, n_woff) through
    jodo_cdgs_pack_weights_host; device=None keeps the blob on the CPU, otherwise it is copied to `device`."""
    return _pack_host('jodo_cdgs', cfg_struct, state_dict, device)


def _split_tape(abi, cfg_struct, blob_host, woff, n_woff, device):
    """(tape uint8 tensor on the CPU or uploaded to `device`, toff ctypes int64 array — byte offsets into the tape indexed like
    `woff`, -1 for the slots that stay fp32) through <abi>_split_size / <abi>_pack_split_host."""
    import torch
    L = lib()
    total = ctypes.c_size_t()
    toff = (ctypes.c_int64 * n_woff)()
    check(getattr(L, abi + '_split_size')(ctypes.byref(cfg_struct), ctypes.byref(total), toff, n_woff), abi + '_split_size')
    tape = torch.empty(total.value, dtype=torch.uint8)
    check(getattr(L, abi + '_pack_split_host')(ctypes.byref(cfg_struct), ctypes.c_void_p(blob_host.data_ptr()), woff, n_woff,
                                               ctypes.c_void_p(tape.data_ptr()), ctypes.c_size_t(total.value)), abi + '_pack_split_host')
    return (tape if device is None else tape.to(device)), toff


def split_tape_2d(cfg_struct, blob_host, woff, n_woff, device=None):
    """The 2-D model's split-bf16 tape, derived from its packed blob (`blob_host`: the CPU blob of pack_weights_2d with its offset
    table): (tape, toff) as _split_tape returns them, through jodo_dgt2d_split_size / jodo_dgt2d_pack_split_host."""
    return _split_tape('jodo_dgt2d', cfg_struct, blob_host, woff, n_woff, device)


def split_tape_cdgs(cfg_struct, blob_host, woff, n_woff, device=None):
    """The CDGS split-bf16 tape, derived from its packed blob (`blob_host`: the CPU blob of pack_weights_cdgs with its offset table):
    (tape, toff) as _split_tape returns them, through jodo_cdgs_split_size / jodo_cdgs_pack_split_host."""
    return _split_tape('jodo_cdgs', cfg_struct, blob_host, woff, n_woff, device)


def pack_split_tape(cfg_struct, state_dict, device=None):
    """The static weight tape of the OPT-IN split-bf16 pair update (jodo_dgt_pack_split_host; JODO_OPT_SPLIT_BF16): a uint8 tensor
    (CPU, or uploaded to `device`).  Raises JodoHipError for configurations this tape is not built for (nf not 256 / 384; conditional
    models have a tape of their own, pack_split_cond_tape)."""
    import torch
    L = lib()
    arr, keep = _marshal(state_dict)
    total, per_block, node_block, attn_block = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    check(L.jodo_dgt_split_size(ctypes.byref(cfg_struct), ctypes.byref(total), ctypes.byref(per_block), ctypes.byref(node_block), ctypes.byref(attn_block)),
          'jodo_dgt_split_size')
    tape = torch.empty(total.value, dtype=torch.uint8)
    check(L.jodo_dgt_pack_split_host(ctypes.byref(cfg_struct), arr, len(keep), ctypes.c_void_p(tape.data_ptr()), ctypes.c_size_t(total.value)),
          'jodo_dgt_pack_split_host')
    return tape if device is None else tape.to(device)


def pack_split_cond_tape(cfg_struct, state_dict, device=None):
    """The conditional model's tape of the OPT-IN split-bf16 pair update (jodo_dgt_pack_split_cond_host; cond_DGT_concat at nf 256 under
    JODO_OPT_SPLIT_BF16): per block the edge FFN, the readout, input_lin's [e ; G] columns and coord_mlp.0 in the un-folded kernel's
    consumption order, a uint8 tensor (CPU, or uploaded to `device`).  Raises JodoHipError for unconditional models and nf != 256."""
    import torch
    L = lib()
    arr, keep = _marshal(state_dict)
    total, per_block = ctypes.c_size_t(), ctypes.c_size_t()
    check(L.jodo_dgt_split_cond_size(ctypes.byref(cfg_struct), ctypes.byref(total), ctypes.byref(per_block)), 'jodo_dgt_split_cond_size')
    tape = torch.empty(total.value, dtype=torch.uint8)
    check(L.jodo_dgt_pack_split_cond_host(ctypes.byref(cfg_struct), arr, len(keep), ctypes.c_void_p(tape.data_ptr()), ctypes.c_size_t(total.value)),
          'jodo_dgt_pack_split_cond_host')
    return tape if device is None else tape.to(device)
