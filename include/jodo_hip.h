/* libjodo_hip.so — C ABI of the MI355X-native JODO DGT denoising hot path.
 *
 * What this replaces in the reference (GRAPH-0/JODO, pure Python; there is no upstream FFI, so the
 * "reference interface" each entry point stands for is the Python call it makes redundant):
 *
 *   jodo_plan_*          <- the per-call dense->sparse conversion in DGT_concat.forward
 *                           (models/mol_gnn.py:512-514: edge_mask.nonzero(), dense_to_sparse) —
 *                           built once per (batch of atom counts) instead of once per step
 *   jodo_dgt_forward     <- DGT_concat.forward          models/mol_gnn.py:491-594
 *                           Cond_DGT_concat.forward     models/mol_gnn.py:687-794
 *                           (incl. EquivariantMixBlock.forward :270-322, TransMixLayer
 *                           models/layers.py:131-186, MultiCondEquiUpdate :71-94,
 *                           CondGaussianLayer models/layers.py:328-334, time_mlp :481-489)
 *   jodo_debug_mlp       <- (no reference counterpart) hardware self-test of the MFMA lane maps
 *
 * Conventions: every function returns 0 on success or a negative JODO_ERR_* code and records a
 * message retrievable with jodo_last_error() (thread-local).  The library never allocates or frees
 * device memory: the caller (PyTorch) owns every device buffer and passes raw pointers; sizes are
 * queried up front.  All launches go to the hipStream_t passed in (as void*); there are no hidden
 * synchronisations and no internal streams.  A plan handle is host memory owned by the library
 * (jodo_plan_destroy frees it); handles are independent and re-entrant, one handle is not
 * thread-safe.  Tensors are contiguous row-major fp32 in the reference's dense layouts.
 */
#ifndef JODO_HIP_H
#define JODO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define JODO_OK 0
#define JODO_ERR_ARG (-1)
#define JODO_ERR_LAUNCH (-2)
#define JODO_ERR_UNSUPPORTED (-3)

/* Model hyper-parameters (config.model.* / config.data.* of the reference's configs). */
typedef struct {
    int32_t nf;          /* D: node hidden width: 128, 256 or 384 (README.md:150,162 the GEOM "Base" model `--config.model.nf 128`,
                            :168 `--config.model.nf 384`); anything else -> JODO_ERR_UNSUPPORTED */
    int32_t n_layers;    /* L in [1, 32] with: the per-block edge readout 2De // L at most one 32-row block wide (L >= 2 / 4 / 6 at
                            nf 128 / 256 / 384), and the edge head's input De + L * cep a multiple of 32, cep = that readout padded to
                            16 or 32 (at nf 128, and at nf 256 with L >= 8, this means even L); the Python module further asks for
                            L <= 16 and a head input of 96..480 except 448.  Tested: L = 6 (nf 128), 8 and 10 (nf 256), 10 (nf 384) */
    int32_t n_heads;     /* H (16)                                              */
    int32_t n_extra;     /* XH: adjacency heads: 2 (DGT_concat, cond_DGT_concat: 14 learned heads of 18 channels + 2, three coordinate
                            heads) or 0 (DGT_concat_sim: 16 learned heads of 16 channels, one coordinate head; lin_query / lin_key
                            [nf, nf], lin_edge0 [nf, nf/4], coord_mlp.2 [1, nf]).  0 is built for nf 256, layout 0, n_layers >= 8,
                            cond_ch 0, exact fp32 only: anything else -> JODO_ERR_UNSUPPORTED, as are JODO_OPT_SPLIT_BF16,
                            JODO_OPT_ATTN_VARIANT != 0, jodo_plan_set_split_weights and the split tapes on such a configuration;
                            spatial_cut_off / edge_quan_th are not read by its kernels */
    int32_t mlp_ratio;   /* r                                                   */
    int32_t in_node_dim; /* nd = atom_types + include_fc_charge                 */
    int32_t edge_ch;     /* ch                                                  */
    int32_t cond_ch;     /* 0 = DGT_concat, >0 = cond_DGT_concat                */
    float spatial_cut_off;
    float edge_quan_th;
    int32_t layout;      /* q / k / lin_edge0 arrangement: 0 = automatic (nf 256: 8 blocks, two heads per block + tail block,
                            with the nf-256 node kernels and LDS-resident attention weights; otherwise one 32-row block per
                            head); 1 = one block per head even at nf 256 (tests: runs the width-generic instantiations) */
} jodo_cfg;

/* Slots of the weight-offset table handed to jodo_dgt_forward (offsets in floats into the packed
 * weight blob produced by jodo_dgt_pack_weights; tests/test_packing.py keeps this enum, the C packer and the
 * independent Python packer tests/py_packing_model.py in lock-step, blob for blob). */
enum jodo_wslot_global {
    JW_TIME_FREQ = 0, JW_TIME_W1, JW_TIME_B1, JW_TIME_W3, JW_TIME_B3,
    JW_COND_W0, JW_COND_B0, JW_COND_W2, JW_COND_B2, JW_COND_LIN_W, JW_COND_LIN_B,
    JW_MOD_W, JW_MOD_B,
    JW_NODE_EMB_W, JW_NODE_EMB_B, JW_EDGE_EMB_W, JW_EDGE_EMB_B, JW_GBF_TOP,
    JW_NH1_W, JW_NH1_B, JW_NH2_W, JW_NH2_B, JW_NH3_W, JW_NH3_B,
    JW_EH1_W, JW_EH1_B, JW_EH2_W, JW_EH2_B, JW_EH3_W, JW_EH3_B,
    JW_GLOBAL_COUNT
};
/* The last six block slots hold the rotated LayerNorm statistics of equi_update (pair update under a shared modulation row;
 * DESIGN.md 4a): with P the centring projection and Q the orthogonal factor of  Q (P W_in[:, e ; G]) = [L ; 0]:
 * ROWQ = Q P W_row, COLQ = Q P W_col, INQ_B = Q P b, LQ = L (block upper triangular, K = 2 De), INEC = P W_in[:, e ; G],
 * QT = Q^T packed as a D x D projection (right-hand factor of the per-forward fold W0 diag(1 + sc) Q^T). */
enum jodo_wslot_block {
    JB_WQ = 0, JB_BQ, JB_WK, JB_BK, JB_WV, JB_BV,
    JB_EE_W, JB_EE_B, JB_LE0_W, JB_LE1_W, JB_N2E_W, JB_N2E_B,
    JB_FF1_W, JB_FF1_B, JB_FF2_W, JB_FF2_B, JB_FF3_W, JB_FF3_B, JB_FF4_W, JB_FF4_B,
    JB_INE_W, JB_ROW_W, JB_COL_W, JB_IN_B, JB_C0_W, JB_C0_B, JB_C2_W, JB_CSCALE,
    JB_NRO_W, JB_NRO_B, JB_ERO_W, JB_ERO_B, JB_GBF,
    JB_ROWQ_W, JB_COLQ_W, JB_INQ_B, JB_LQ_W, JB_INEC_W, JB_QT_W,
    JB_BLOCK_COUNT
};
/* table length = JW_GLOBAL_COUNT + n_layers * JB_BLOCK_COUNT; block l slot s lives at
 * JW_GLOBAL_COUNT + l * JB_BLOCK_COUNT + s */

/* ---- weights --------------------------------------------------------------------------------------------------
 * jodo_dgt_pack_weights  <- the parameter container of DGT_concat / Cond_DGT_concat: the 351 (QM9) / 431 (GEOM L = 10) /
 *                           357 (conditional) tensors of its state_dict, names and shapes as registered by the
 *                           constructors models/mol_gnn.py:414-489 and :601-684 (a leading "module." — checkpoints
 *                           saved through nn.DataParallel, utils.py:23-30 — is accepted and ignored).
 * A host with nothing but a C FFI hands over the named fp32 tensors (HOST pointers, contiguous, PyTorch [out, in]
 * layout) and receives the packed blob in MFMA A-operand order plus the offset table jodo_dgt_forward takes.
 *   jodo_dgt_packed_size        number of floats of the blob and of offset-table slots for this configuration
 *   jodo_dgt_pack_weights_host  pack into caller-owned host memory (no device work at all)
 *   jodo_dgt_pack_weights       pack and upload into caller-owned DEVICE memory; this load-time call synchronises
 *                               `stream` before returning (its staging buffer lives only for the call)
 * A missing or mis-sized parameter is an error (JODO_ERR_ARG, the name is in jodo_last_error()). */
typedef struct {
    const char* name;       /* state_dict key, e.g. "e_block_3.attn_mpnn.lin_edge0.weight" */
    const float* data;      /* host pointer, contiguous fp32 */
    const int64_t* shape;
    int32_t ndim;
} jodo_tensor;
int jodo_dgt_packed_size(const jodo_cfg* cfg, const jodo_tensor* tensors, int n_tensors, size_t* n_floats, int* n_woff);
int jodo_dgt_pack_weights_host(const jodo_cfg* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                               size_t cap_floats, int64_t* woff_out, int n_woff);
int jodo_dgt_pack_weights(const jodo_cfg* cfg, const jodo_tensor* tensors, int n_tensors, void* packed_dev,
                          size_t cap_floats, int64_t* woff_out, int n_woff, void* stream);

typedef struct jodo_plan jodo_plan;

/* Build the execution plan for a batch: B molecules with n_nodes[b] atoms (host array), padded
 * width N of the dense API tensors.  Molecules are ordered by size internally; masks are implied
 * (prefix masks, diagonal excluded), which is what the reference's samplers produce
 * (sampling.py:193-201).  max_chunk packs three work-item sizes (0 in a field = automatic): bits 0-15 sources per
 * directed edge work item (embeddings, directed update; default 8), bits 16-23 pair offsets per item of the pair update
 * kernel (default 1), bits 24-31 the pair-mode decomposition of the fused attention kernel: 0 = automatic — 256 persistent
 * workgroups on a wrap-around schedule of equal-cost runs of pair offsets; 1..200 = that many pair offsets per
 * item, one workgroup per item; 255 = one workgroup per item with the chunk chosen by the plan's launch model. */
int jodo_plan_create(const jodo_cfg* cfg, int B, int N, const int32_t* n_nodes_host, int max_chunk,
                     jodo_plan** out);
void jodo_plan_destroy(jodo_plan* plan);
/* bytes of the device-side descriptor tables / of the scratch workspace for this plan */
size_t jodo_plan_desc_bytes(const jodo_plan* plan);
size_t jodo_plan_workspace_bytes(const jodo_plan* plan);
/* number of floats in the time-modulation vector of one molecule (for sizing/debug) */
int64_t jodo_plan_mod_len(const jodo_plan* plan);
/* copy the descriptor tables into caller-owned device memory (async on stream) */
int jodo_plan_upload(jodo_plan* plan, void* desc_dev, void* stream);
/* plan statistics: out[0]=packed nodes, [1]=dense edge rows (sum n^2), [2]=directed edges
 * (sum n(n-1)), [3]=node strips, [4]=edge work items, [5]=max parts */
int jodo_plan_stats(const jodo_plan* plan, int64_t* out6);

/* One evaluation of the score network.
 *   packed_w / woff: packed weight blob (device) and its offset table (host, see enums above)
 *   xh [B,N,3+nd], edge_x [B,N,N,ch]; cond_x / cond_edge_x same shapes or NULL (first step);
 *   noise_level [B]; context [B,cond_ch] or NULL
 *   out_xh [B,N,3+nd], out_edge [B,N,N,ch] (fully written, zeros on padding)
 *   flags_dev: int32[8] device scratch; after the call [0] = NaN guard fired (mol_gnn.py:587-589),
 *              [1] reserved (0), [2] = all molecules shared one noise level, [3] = the self-conditioning positions
 *              were not all equal (0 => the batch-global first-step branch of :544 was taken),
 *              [4] = edge inputs were not symmetric (directed kernels used), [5] = STICKY count of calls in which
 *              the NaN guard fired (only ever incremented by the library; the caller clears it when it reads it),
 *              [6] = STICKY pin violations (JODO_OPT_PIN_*: bit 0 symmetry, bit 1 shared row), [7] reserved
 *   workspace: jodo_plan_workspace_bytes() bytes of device scratch, the caller's, kept between calls on the same plan.  What a caller
 *              may leave in it: ANY FINITE float32 values (zero-fill it once before the first call; torch.empty / hipMalloc memory may
 *              hold NaN bit patterns).  Outputs do not depend on the content — neither on another call's leftovers nor on finite garbage
 *              (tests/test_forms_gpu.py poisons it) — with one exception: the two copies of the dense edge state ([sum n^2 + 32, nf / 4]
 *              floats each) must not hold NaN / Inf, because the pair path never writes the diagonal rows (i, i) of a molecule's n x n
 *              tile (nor, under JODO_OPT_HALF_ROWS, the mirror row of a pair) and reads them against a zero weight.  The library never
 *              writes a non-finite value into those rows, so one fill is enough for the life of the workspace; every other array
 *              may hold anything, NaN included.
 *   dbg: optional device buffer for intermediates (tests) or NULL */
int jodo_dgt_forward(jodo_plan* plan, const void* desc_dev, const float* packed_w, const int64_t* woff,
                     int n_woff, const float* xh, const float* edge_x, const float* cond_x,
                     const float* cond_edge_x, const float* noise_level, const float* context,
                     float* out_xh, float* out_edge, int32_t* flags_dev, void* workspace, void* stream);

/* Executed-work model of a plan (measurement): fp32 flops that the kernels of ONE jodo_dgt_forward issue on the matrix pipe
 * (v_mfma_f32_32x32x2_f32 = 4096 flop per instruction), per launch class (enum jodo_prof_class below; array of
 * JODO_PROF_COUNT doubles), counted from the plan's work-item lists and the kernels' loop structure, padded lanes included.
 * uniform_t / symmetric = flags [2] / ![4] of the call being priced (they select the kernel variants that do the work).
 * This is the numerator of bench.py's roofline fraction: work the hardware executes, not the reference formulation's. */
int jodo_plan_work(const jodo_plan* plan, int uniform_t, int symmetric, double* mfma_flops_per_class);

/* Work-decomposition options of a plan (defaults are the measured-best settings).  These replace the
 * environment switches of round 1: the library reads no environment variables. */
enum jodo_plan_option {
    JODO_OPT_FUSE_NEXT_QKV = 0,   /* 1 (default): with >= 1024 node strips k_node_post of block l also produces block l + 1's
                                     q / k / v; 0: always a separate k_node_pre launch */
    JODO_OPT_DIR_SPLIT = 1,       /* 1 (default): pair-update items of a launch's sparsely filled last round get two workgroups,
                                     one per direction; 0: one workgroup per item */
    JODO_OPT_NODE_POST_WAVES = 2, /* 0 (default): automatic; 1 / 2 / 4: waves per strip for every strip of k_node_post;
                                   * 12 / 14: automatic split, 2 / 4 waves per strip of the remainder launch */
    JODO_OPT_ATTN_VARIANT = 3,    /* nf 256 pair attention kernel, weight residency / hand-over granularity: 0 (default), 1, 2, 3 (dgt_kernels_attn.h); other values are rejected */
    /* Path pinning.  By default every forward launches every kernel variant and device flags decide which ones work (no host
     * sync); the idle variants cost a dispatch each (~5 us, 24 per forward at 8 blocks; counted by jodo_profile_read_kernels in
     * tests/test_dgt_gpu.py: 88 -> 62 launches at QM9 B = 2500, i.e. 26 with the heads' two; 81 -> 63 for the conditional model).  Inside one sampling round the inputs
     * stay symmetric and the noise level stays shared, so a caller that has read flags [2] / [4] of one call may pin them for the
     * following calls on this plan: only the working variants are then launched.  A call that violates a pin (e.g. asymmetric
     * inputs under a symmetric pin) is detected on the device: flags[6] gets bit 0 (symmetry pin) / bit 1 (shared-row pin), sticky,
     * and its outputs are unspecified — callers check flags[6] when they read the NaN counter. */
    JODO_OPT_PIN_SYMMETRIC = 4,   /* 0 (default): decided per call on the device; 1: inputs are symmetric (pair kernels only);
                                     2: asymmetric (directed kernels only) */
    JODO_OPT_PIN_UNIFORM_T = 5,   /* 0 (default): per call; 1: one shared modulation row (folded pair update only); 2: per-molecule rows */
    JODO_OPT_ROT_STATS = 6,       /* 1 (default): under a shared modulation row and symmetric inputs the LayerNorm statistics of
                                     equi_update are taken in the rotated basis (Q P W_row h, Q P W_col h per node, the triangular
                                     L [e ; G] per pair, a per-molecule Gram tile — taken around the molecule's first atom, so that a
                                     common component of the two rows is gone before anything is squared — for the rest);
                                     0: from S = W_in [e ; G] itself; 2 (tests): rotated with the uncentred Gram tiles of round 3 */
    JODO_OPT_NODE_MIX = 7,        /* 1 (default): when k_node_post runs as full rounds + a remainder launch, the remainder launch also carries
                                     the k_node_ab items and Gram tiles of the strips the full rounds finished (they fill the SIMDs the
                                     remainder's cooperative workgroups leave idle); 0: separate launches */
    JODO_OPT_HEADS_MIX = 8,       /* 1 (default): under a symmetric pin the node head and the pair form of the edge head share one launch
                                     (node strips first: the edge head's short items fill the SIMDs the node head's last round leaves idle) */
    JODO_OPT_HALF_ROWS = 9,       /* 1 (default): under a symmetric pin, for molecules that fit an attention group (n <= 128), the embedding and the pair
                                     update write the edge state and the head inputs only for the row a pair's evaluating lane reads back —
                                     (i, i + d) of the circulant walk — instead of both mirror rows (the workspace copy of e is then half
                                     stale: jodo_debug_fetch(what = 1) is for unpinned calls) */
    JODO_OPT_PRE_EMBED = 10,      /* 1 (default; nf 256 tuned kernel set): the edge embedding shares a launch with the first block's q / k / v
                                     items (k_pre_embed: HBM-write-bound items beside matrix-bound ones); 0: a launch of its own */
    JODO_OPT_AB_PRE = 11,         /* 1 (default; nf 256 tuned kernel set, fewer than 1024 node strips): the next block's q / k / v items share
                                     the launch of this block's k_node_ab items and Gram tiles (k_node_ab_pre); 0: a k_node_pre launch per block */
    JODO_OPT_Z_SPLIT = 12,        /* 1 (default): when the LAST round of the pair update's launch (n_pitems mod 1024) has at most 256 items, they run as
                                   * workgroups of 4 waves that share the per-pair coord_mlp.0 output blocks (k_edge_update_sym<.., ZW = 4>); 2: also
                                   * 2 waves for 257 .. 512 items (measured slower on MI355X, kept for A/B runs); 0: one wave per item throughout */
    JODO_OPT_SPLIT_BF16 = 13,     /* 0 (default): every projection runs on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).  1 (OPT-IN, nf 256 / 384
                                   * unconditional models, pinned symmetric + shared-row paths, rotated statistics on, weights handed over with
                                   * jodo_plan_set_split_weights): the folded pair update runs its projections in the split-bf16 form — every
                                   * operand as hi + mid + lo bf16 terms, six v_mfma_f32_32x32x16_bf16 products per K = 16 step, fp32
                                   * accumulation: fp32-equivalent arithmetic (dropped terms <= 3 * 2^-26 relative; profiles/r06_split_gate.txt)
                                   * at 6/16 of the matrix cycles (csrc/dgt_kernels_split.h); with the tuned nf 256 kernel set also the node kernels
                                   * (k_node_post_split, k_node_ab_split: csrc/dgt_kernels_split_node.h).  Results differ from the default path in the
                                   * last bits; the default and every headline number stay exact fp32.  Ignored when a precondition fails.
                                   * 2 (experiments): also the fused attention kernel (k_edge_attn variants 4 + 5: two launches that share every
                                   * item by heads; nf 256 tuned set, plans without molecules above an attention group) — parity-tested, measured
                                   * 15 % SLOWER than the fp32 kernel on MI355X (513 against 447 us per block at QM9 B = 2500), DESIGN.md 4i.
                                   * CONDITIONAL models (cond_ch > 0, nf 256): >= 1 runs the UN-FOLDED pair update in the split form
                                   * (k_edge_update_sym_split_cond, csrc/dgt_kernels_split_cond.h; per-molecule modulation rows, so nothing folds
                                   * or rotates and per-molecule noise levels are legal input).  Preconditions: the conditional tape handed over
                                   * (jodo_dgt_pack_split_cond_host -> jodo_plan_set_split_weights), JODO_OPT_PIN_SYMMETRIC = 1,
                                   * JODO_OPT_PIN_UNIFORM_T = 2, one circulant offset per pair item; node and attention kernels stay exact fp32,
                                   * so 2 means the same as 1.  Ignored when a precondition fails. */
    JODO_OPT_COUNT
};
int jodo_plan_set_option(jodo_plan* plan, int option, int value);

/* debug / tests: the pair-mode attention schedule of a plan.  out8 = items, their total pair offsets, partials per atom (max),
 * persistent schedule (0 / 1), and for a persistent schedule: smallest / largest slot load (offsets), most items in a slot, idle slots.
 * Also checks the item lists themselves (every group's pair offsets tiled exactly once, partial indices 0 .. parts - 1, parts as its
 * atoms expect) and returns an error if they are inconsistent. */
int jodo_debug_attn_schedule(const jodo_plan* plan, int64_t* out8);

/* debug: copy an internal per-block intermediate out of the workspace after a forward.
 * what: 0 = h [Nn,D], 1 = e [rows,De], 2 = pos [Nn,4] (raw, not centred), 3 = the attention partials
 * [Nn, parts, D] (unnormalised) of the last block run, 5 = the modulation row, 6 = q.  dst must hold the full array; returns element count via *count. */
int jodo_debug_fetch(jodo_plan* plan, const void* workspace, int what, float* dst_dev, int64_t* count,
                     void* stream);
/* limit the number of DGT blocks executed by jodo_dgt_forward (tests; <0 = all) */
int jodo_debug_set_max_blocks(jodo_plan* plan, int max_blocks);
/* force the directed (per directed edge) kernels even for symmetric inputs (tests; default 0: the
 * symmetric pair kernels are chosen on the device whenever edge_x / cond_edge_x are symmetric) */
int jodo_debug_set_force_directed(jodo_plan* plan, int on);
/* phase-cycle instrumentation of k_edge_update_sym (only in builds with -DJODO_PHASE_TIMING): device
 * buffer of 16 uint64 sums, [15] = number of instrumented waves; NULL disables */
int jodo_debug_set_timing_buffer(jodo_plan* plan, void* dev16xu64);

/* Per-kernel-class timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * enable = 1 makes every subsequent jodo_dgt_forward bracket every launch class with events (two event
 * packets per class boundary cost ~10 us each: ~0.5 ms per forward at 8 blocks); enable = 2 brackets only the
 * dominant class JODO_PROF_EDGE_UPDATE (~0.1 ms); enable = 16 + c brackets only class c (what the roofline leg needs: the class that was largest in
 * this run's warm-up); jodo_profile_read synchronises those events and returns, per class, the summed
 * milliseconds and the number of BRACKETS (event pairs: one per class and block, whatever the plan's pins and options — not kernel
 * launches) since the last read (arrays of JODO_PROF_COUNT), then resets.  jodo_profile_read_kernels returns, per class, the number of
 * KERNEL LAUNCHES issued inside those brackets since its last call (a host counter; idle variants that exit on a device flag count, they
 * are dispatches), then resets: what a pin or a launch-merging option changes. */
enum jodo_prof_class {
    JODO_PROF_PROLOGUE = 0, JODO_PROF_NODE_PRE, JODO_PROF_EDGE_ATTN, JODO_PROF_RESERVED3, JODO_PROF_RESERVED4,
    JODO_PROF_NODE_POST, JODO_PROF_EDGE_UPDATE, JODO_PROF_EPILOGUE, JODO_PROF_COUNT
};
int jodo_profile_enable(jodo_plan* plan, int enable);
int jodo_profile_read(jodo_plan* plan, float* ms_sum, int32_t* launches);
int jodo_profile_read_kernels(jodo_plan* plan, int32_t* kernels);

/* ---- caller-side kernels of the sampling loop ---------------------------
 * jodo_sampler_step  <- the update of AncestralSampler.sampling, sampling.py:536-589, with the noise
 *                       construction of models/utils.py:67-99 folded in:
 *                         mean = c_x * x + c_pred * pred;  next = mean + sigma * eps   (nodes and edges)
 *                       eps_pos [B,N,3], eps_feat [B,N,node_feats-3], eps_edge [B,edge_ch,N,N] are RAW
 *                       N(0,1) draws in the reference's shapes and draw order; masking, centre-of-mass
 *                       removal (positions) and lower-triangle mirroring (edges) happen in the kernel.
 *                       c_x, c_pred, sigma: posterior coefficients of the step (host scalars).
 *                       n_nodes_dev: int32[B] atom counts (prefix masks).  All outputs fully written.
 * jodo_decode        <- post_process sampling.py:53-97 + inverse scaler utils.py:71-105 + the
 *                       per-molecule slicing inputs of mol_process :12-32: positions [B,N,3] f32,
 *                       atom type [B,N] u8 (argmax), formal charge [B,N] i8 (round), bond type [B,N,N] u8
 *                       (compress_edge thresholds, or argmax+1 where any channel > 0.5); zeros on padding. */
int jodo_sampler_step(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred,
                      float sigma, const float* x, const float* edge_x, const float* pred, const float* edge_pred,
                      const float* eps_pos, const float* eps_feat, const float* eps_edge, float* x_next,
                      float* edge_next, float* x_mean, float* edge_mean, void* stream);
/* Graph-replayable form of the same update: the per-step scalars come from a device table
 * coef_tab_dev [steps][4] = (c_x, c_pred, sigma, noise_level) at row *step_dev, so ONE captured hipGraph of a
 * sampling step (jodo_step_begin -> jodo_dgt_forward -> noise draws -> jodo_sampler_step_tab -> jodo_step_end)
 * serves every step.  jodo_step_begin writes noise_level[b] = tab[*step][3] for the forward; jodo_step_end
 * increments *step_dev. */
int jodo_sampler_step_tab(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef_tab_dev,
                          const int32_t* step_dev, const float* x, const float* edge_x, const float* pred,
                          const float* edge_pred, const float* eps_pos, const float* eps_feat, const float* eps_edge,
                          float* x_next, float* edge_next, float* x_mean, float* edge_mean, void* stream);
/* Device-noise form of the same update ("one jodo_sampler_step kernel with Philox"): the three
 * normal draws of models/utils.py:67-99 are generated inside the kernel by a counter-based generator (Philox4x32-10 +
 * Box-Muller) keyed by `seed`, counter = (element, draw index, stream); masking, centre-of-mass removal and lower-triangle
 * mirroring as above.  draw index = `draw` (host scalars; coef_tab_dev = step_dev = NULL) or `draw` + *step_dev with the
 * coefficients from row *step_dev of coef_tab_dev (captured hipGraph).  Same distribution as the reference's draws, a
 * different stream: parity runs keep the replayed-draw form above.  Callers give every rank its own seed. */
int jodo_sampler_step_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred,
                          float sigma, const float* coef_tab_dev, const int32_t* step_dev, uint64_t seed, uint32_t draw,
                          const float* x, const float* edge_x, const float* pred, const float* edge_pred, float* x_next,
                          float* edge_next, float* x_mean, float* edge_mean, void* stream);
int jodo_step_begin(int B, const float* coef_tab_dev, const int32_t* step_dev, float* noise_level_out, void* stream);
int jodo_step_end(int32_t* step_dev, void* stream);
/* jodo_dpm_update  <- one update of the hybrid DPM-Solver++ sampler, mix_dpm_solver.py: positions take the ancestral step
 *                     of :44-59 (pos_out = cx * x_pos + cp * PP + sigma * eps, eps_pos [B,N,3] RAW N(0,1) draws: masking and
 *                     centre-of-mass removal happen in the kernel; sigma = 0 for the last update of a round, :56), every other
 *                     channel of the node tensor and the whole edge tensor take the data-prediction update of :61-265
 *                         out = a * base - b * P - c * (c2 * (DA - DB))
 *                     which covers first order (c = 0, :84-85), single-step second order (:124-125, :137-146: P = DB =
 *                     prediction at the start, DA = prediction at s1), third order (:199-219, c < 0) and second-order
 *                     multistep (:253-260: P = DA = newest prediction, DB = the one before, c2 = 1 / r0).  PP = the
 *                     prediction whose position channels drive the ancestral step.  Tensors: node [B,N,3+nd], edge
 *                     [B,N,N,ch]; e* = the edge counterparts.  Coefficients {cx, cp, sigma, a, b, c, c2, noise_level}: either 8
 *                     host floats, or row *step_dev of a device table (row stride tab_stride floats, first column tab_col) so
 *                     that a captured hipGraph of an outer step replays for every step.
 * jodo_step_begin_at  noise_level[b] = table[*step][tab_col + 7]  (the graph-replayable counterpart of the per-evaluation
 *                     noise level, mix_dpm_solver.py:118,131) */
int jodo_dpm_update(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                    const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x_pos,
                    const float* x_base, const float* edge_base, const float* P, const float* eP, const float* DA, const float* eDA,
                    const float* DB, const float* eDB, const float* PP, const float* eps_pos, float* x_out, float* edge_out,
                    void* stream);
/* jodo_dpm_update with the position noise drawn in the kernel (see jodo_sampler_step_rng): draw index = draw (+ *step_dev *
 * draw_mul with a device table, so that the two updates of a captured outer step use draws 2k and 2k + 1). */
int jodo_dpm_update_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                        const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, uint64_t seed,
                        uint32_t draw, uint32_t draw_mul, const float* x_pos, const float* x_base, const float* edge_base,
                        const float* P, const float* eP, const float* DA, const float* eDA, const float* DB, const float* eDB,
                        const float* PP, float* x_out, float* edge_out, void* stream);
int jodo_step_begin_at(int B, const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col,
                       float* noise_level_out, void* stream);
int jodo_decode(int B, int N, int atom_types, int include_fc, int edge_ch, int compress_edge, int centered,
                float pos_norm, float atom_norm, float fc_norm, float edge_norm, const int32_t* n_nodes_dev,
                const float* xh, const float* edge_x, float* pos_out, uint8_t* atom_type_out, int8_t* fc_out,
                uint8_t* edge_type_out, void* stream);

/* ---- training step: the whole network ------------------------------------------------------------------
 * jodo_train_forward   <- the grad-enabled model call of get_sde_graph_loss_fn, losses.py:335-343 (DGT_concat.forward /
 *                         Cond_DGT_concat.forward under model.train(): dropout in the four FFN positions, mol_gnn.py:262-268; NOT on the
 *                         attention weights — layers.py:179 is an identity because the block builds its TransMixLayer with the default
 *                         dropout = 0, mol_gnn.py:230-231) with every activation the backward needs kept in `workspace`
 * jodo_train_backward  <- loss.backward(), losses.py:109: d loss / d parameter for EVERY tensor of the state_dict, given
 *                         d loss / d out_xh and d loss / d out_edge (the loss itself, losses.py:350-385, stays host code)
 * Parameters are NOT packed here: params_dev[i] / grads_dev[i] are DEVICE pointers to contiguous fp32 tensors in PyTorch layout,
 * in the order of the `params` array given to jodo_train_create (names = state_dict keys, a leading "module." is ignored; `data`
 * of that array is not read, shapes are checked).  grads are fully written (not accumulated).  Inputs need no gradient (the
 * self-conditioning inputs are detached, losses.py:339).  The handle fixes the batch: B molecules with n_nodes[b] atoms, padded
 * width N of the dense tensors (same layouts as jodo_dgt_forward).  dropout_p = config.model.dropout under model.train(), 0 under
 * model.eval(); masks come from a counter-based generator keyed by `seed` (same law as torch's, a different stream) and are
 * regenerated, not stored: pass the same (dropout_p, seed) to the backward.  flags_out (optional): int32[8], [0] = NaN guard
 * fired (mol_gnn.py:587-589: positions zeroed, their gradient is zero), [3] = self-conditioning distances present (0 => the
 * first-step branch of :544).  workspace: jodo_train_workspace_bytes() bytes, kept by the caller between forward and backward.
 * desc_dev: jodo_train_desc_bytes() bytes of device memory filled by jodo_train_upload (synchronises the stream once).
 * jodo_train_create takes cfg->n_extra = 2 (DGT_concat, cond_DGT_concat) or 0 (DGT_concat_sim: EquivariantBlock / Trans_Layer /
 * CondEquiUpdate, mol_gnn.py:949-1124, :97-208, :16-48 — 16 learned heads, the adjacency flags never read, one coordinate head:
 * coord_mlp.2.weight [1, nf], the kept coordinate activation [R, 1]; dropout in the two feed-forwards as above).  n_extra = 0 is taken
 * with nf 256, n_heads 16, n_layers >= 8, layout 0 and cond_ch 0 only; every other n_extra and every other combination ->
 * JODO_ERR_UNSUPPORTED naming the values. */
typedef struct jodo_train jodo_train;
int jodo_train_create(const jodo_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const jodo_tensor* params, int n_params,
                      jodo_train** out);
void jodo_train_destroy(jodo_train* t);
size_t jodo_train_desc_bytes(const jodo_train* t);
size_t jodo_train_workspace_bytes(const jodo_train* t);
/* option 0 = fused per-edge forward chains (csrc/train_fused.hip: edge_emb -> LN -> lin_edge0 / 1; edge FFN; input_lin -> LN -> coord_mlp as
 * one strip-model kernel each, activations saved where the backward expects them): 1 (default) / 0 (one launch per operation);
 * option 1 = the input-gradient side of the same chains in the backward (the weight-gradient products stay GEMMs): 1 (default) / 0;
 * option 2 = 1 (default): forwards keep every activation a backward reads; 0: the following forwards will not be differentiated (the
 *            no-grad self-conditioning forward of a training step, losses.py:335-339) and skip those stores — jodo_train_backward after
 *            such a forward is undefined;
 * option 3 = 1 (default): the backward's weight-gradient products are queued and run in grouped launches (csrc/train_gemm.hip
 *            gemm_dw_group: same plans and arithmetic as one launch each, bit-identical gradients); 0: one launch per product;
 * option 4 = 1 (default where built): the attention of a block as one forward and two backward launches, one to four waves per atom (forward
 *            bit-identical to the op-by-op kernels); 0: scores | softmax | messages and their six backward kernels; 2: the one-wave-per-atom
 *            form of batches above 16 k atoms whatever the batch (tests);
 * option 5 = the Gaussian layer's backward as one wave-per-chunk pass: 1 (default) for batches of >= 4 096 chunks of 32 edge rows (it loses
 *            below), 0 never, 2 always (tests) */
int jodo_train_set_option(jodo_train* t, int option, int value);
/* tests: byte offset and element count of a kept activation inside the workspace; what 0 = hhat [Nn, D] (TransMixLayer's output,
 * layers.py:153), 1 = alpha [R, H] (softmax weights, layers.py:178) of block `layer`; the FFNs (mol_gnn.py:263-268): 2 = f1
 * [Nn, r D] (ff_linear1), 3 = a1 [Nn, r D] (SiLU(f1) x dropout), 4 = f2 [Nn, D] (ff_linear2, before its dropout), 5 = f3 [R, r De]
 * (ff_linear3), 6 = a3 [R, r De] (SiLU(f3) x dropout), 7 = f4 [R, De] (ff_linear4, before its dropout) */
int jodo_train_debug_locate(const jodo_train* t, int what, int layer, size_t* byte_offset, size_t* count);
int jodo_train_upload(jodo_train* t, void* desc_dev, void* stream);
/* the host image jodo_train_upload copies (jodo_train_desc_bytes() bytes, owned by the handle): callers that stage it through pinned
 * memory themselves upload it without jodo_train_upload's stream synchronisation */
const void* jodo_train_desc_host(const jodo_train* t);
int jodo_train_forward(jodo_train* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* xh,
                       const float* edge_x, const float* cond_x, const float* cond_edge_x, const float* noise_level,
                       const float* context, float dropout_p, uint64_t seed, float* out_xh, float* out_edge, int32_t* flags_out,
                       void* workspace, void* stream);
/* jodo_train_backward writes (not accumulates) every gradient: the grads_dev buffers are zeroed first, and where two of them lie less
 * than 16 bytes apart (sub-allocations of one buffer with 16-byte aligned slices, jodo_amd/optim.py slice_offsets) the bytes BETWEEN them
 * are zeroed as well — do not keep live data in such a gap. */
int jodo_train_backward(jodo_train* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                        const float* noise_level, const float* d_out_xh, const float* d_out_edge, float dropout_p, uint64_t seed,
                        void* workspace, void* stream);
/* the training path's fp32 MFMA GEMM on its own (tests):  C[M, N] (+)= op(A) op(B) (+ bias[N]);  tA = 0: A[m lda + k], 1: A[k lda + m];
 * tB = 0: B[k ldb + n], 1: B[n ldb + k];  ws / ws_floats: device scratch for split-K partial tiles (NULL: never split) */
int jodo_train_gemm(int tA, int tB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    const float* bias, int acc, float* ws, size_t ws_floats, void* stream);
/* the same with the fused epilogues the training step uses (tests): act 1: C = tanh(.); act 2: C = pre-activation, out2 = SiLU(.) laid out
 * like C; dbias (tA = 1, act = 0; C is accumulated into): dbias[m] += sum_k A(k, m), the bias gradient riding on a weight-gradient product */
int jodo_train_gemm_ex(int tA, int tB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                       const float* bias, int act, float* out2, float* dbias, float* ws, size_t ws_floats, void* stream);
/* the split-bf16 form of the same product (tests; the training step reaches it through jodo_cdgs_train_set_option 3): both fp32
 * operands are split into hi + mid + lo bf16 terms on their way into LDS, a K = 16 step is the six products h*l, l*h, m*m, h*m, m*h, h*h
 * on v_mfma_f32_32x32x16_bf16 into fp32 accumulators (dropped: m*l, l*m, l*l <= 3 * 2^-26 |a b|).  Same layouts, tiling, split-K
 * slices and slice order as jodo_train_gemm, no atomics.  acc as jodo_train_gemm, act / out2 / dbias as jodo_train_gemm_ex (act is not
 * combined with acc; dbias needs tA = 1 and act = 0 and is always added to); dropout_p / seed / site: the dropout multiplier of
 * element m N + n on out2 (act 2), train_common.h drop_mul.  An output that is a single product with an exactly-bf16 factor (the other K - 1 terms zero) is exact. */
int jodo_train_gemm_s(int tA, int tB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                      const float* bias, int acc, int act, float* out2, float* dbias, float dropout_p, uint64_t seed, int site,
                      float* ws, size_t ws_floats, void* stream);

/* tests: ONE public function of csrc/train_fused.h on caller-owned device arrays (csrc/train_debug.hip; tests/test_fused_kernels_gpu.py
 * compares every array the kernel stores with a float64 restatement).  The entry adds no kernel: it fills FusedDims / FusedBlockParams /
 * FusedTopo / AttnTopo / Drop from the struct and calls the host function named by `op`.  It is the safety boundary of those tests, so
 * nothing is launched unless every check below holds:
 *   - the op's availability predicate (fused_available, fused_chain_b_available, fused2d_available, fused_attention_available; F in
 *     {128, 256, 384} for the node pair, 2 <= De <= 129 for the Gaussian backward) -> JODO_ERR_UNSUPPORTED naming the values;
 *   - the topology is HOST memory: every index is checked against R / Nn / B / N, the offsets for monotonicity and consistency with nn
 *     (node_off[b + 1] = node_off[b] + nn[b], edge_off[b + 1] = edge_off[b] + nn[b]^2, totals Nn and R, node_mol constant on a molecule's
 *     rows); the entry uploads it into topo_dev (int32, topo_dev_count >= what the op uploads) on `stream` in front of the launch;
 *   - every array the op reads or writes is a slot a[JODO_FT_*] with its element count n[.]: non-NULL, 16-byte aligned (4 for the strided arrays, which are
 *     read float by float), and at least as long as what the op touches (strided arrays: (rows - 1) ld + width);
 *   - a NULL pointer, a non-positive count, an unknown op, an offset or stride that does not hold its columns -> JODO_ERR_ARG.
 * Slots an op does not use are ignored.  Which slot is which argument: the table in front of each case in csrc/train_debug.hip;
 * the node pair reads a / res_b from E_IN / N2E and dy from DE_OUT, writes XH / RS / E_OUT (y) and DE_PREV (dx); the attention's q | k | v
 * and d q | d k | d v are three slots each with their own row stride (they may point into one merged array); the Gaussian backward reads
 * its row gradient from DG (ldg, gcol).  Optional slots (NULL allowed): N2E of JODO_FT_NODE_LN_MOD (no residual), DD2. */
enum { JODO_FT_PACK = 0, JODO_FT_PACK_BWD, JODO_FT_PACK_2D, JODO_FT_PACK_2D_BWD, JODO_FT_CHAIN_A, JODO_FT_CHAIN_B, JODO_FT_CHAIN_C,
       JODO_FT_BWD_A, JODO_FT_BWD_B, JODO_FT_BWD_C, JODO_FT_CHAIN_A_2D, JODO_FT_BWD_A_2D, JODO_FT_NODE_LN_MOD, JODO_FT_NODE_LN_MOD_BWD,
       JODO_FT_ATTN_FWD, JODO_FT_ATTN_BWD, JODO_FT_GBF_BWD, JODO_FT_N_OPS };
enum { JODO_FT_EDGE_EMB_W = 0, JODO_FT_EDGE_EMB_B, JODO_FT_LE0, JODO_FT_LE1, JODO_FT_FF3_W, JODO_FT_FF3_B, JODO_FT_FF4_W, JODO_FT_FF4_B,
       JODO_FT_ERO_W, JODO_FT_ERO_B, JODO_FT_IN_W, JODO_FT_IN_B, JODO_FT_C0_W, JODO_FT_C0_B, JODO_FT_C2_W, JODO_FT_N2E_B, JODO_FT_GBF_MEANS,
       JODO_FT_GBF_STDS, JODO_FT_PACKED, JODO_FT_POS, JODO_FT_GM, JODO_FT_E_IN, JODO_FT_EMOD, JODO_FT_D2, JODO_FT_G, JODO_FT_XH, JODO_FT_RS,
       JODO_FT_ET, JODO_FT_T0, JODO_FT_T1, JODO_FT_N2E, JODO_FT_EN, JODO_FT_F3, JODO_FT_A3, JODO_FT_F4, JODO_FT_E_OUT, JODO_FT_EH, JODO_FT_HR,
       JODO_FT_HC, JODO_FT_QMOD, JODO_FT_U, JODO_FT_C0PRE, JODO_FT_C0A, JODO_FT_INV, JODO_FT_DINV, JODO_FT_DC0, JODO_FT_DU, JODO_FT_DPRE,
       JODO_FT_DE, JODO_FT_DG, JODO_FT_DE_OUT, JODO_FT_F4D, JODO_FT_DF4, JODO_FT_DHID, JODO_FT_DEN, JODO_FT_DE_PREV, JODO_FT_DT1, JODO_FT_DT0,
       JODO_FT_DET, JODO_FT_DE1, JODO_FT_MODS, JODO_FT_Q, JODO_FT_K, JODO_FT_V, JODO_FT_ADJ2D, JODO_FT_ADJSP, JODO_FT_ALPHA, JODO_FT_HHAT,
       JODO_FT_DHHAT, JODO_FT_DS, JODO_FT_DQ, JODO_FT_DK, JODO_FT_DV, JODO_FT_DXP, JODO_FT_DD2, JODO_FT_PART_M, JODO_FT_PART_S,
       JODO_FT_N_SLOTS };
typedef struct {
    int32_t op;
    int32_t D, De, r, QK, ce, nco;                 /* FusedDims (De = D / 4; node pair: D = F; Gaussian backward: De alone) */
    int32_t R, Nn, B, N;                           /* edge rows, node rows, molecules, atoms of the largest molecule */
    int32_t save;                                  /* FusedTopo::save */
    int32_t H, XH, SC, one_wave;                   /* attention: heads, adjacency heads in front, channels per learned score head */
    int32_t ldqk, ldv, ldd_qk, ldd_v;              /* AttnTopo row strides */
    int32_t ld_eh, eh_col;                         /* chain B: row stride and first column of the readout inside the head input */
    int32_t ldm, g_off, sh_off, sc_off, acc;       /* node pair: stride and column offsets of mods; acc also of the Gaussian backward */
    int32_t ldg, gcol;                             /* Gaussian backward: row stride and first column of d G */
    int32_t site_a3, site_f4;                      /* dropout sites of chain B / B' (Drop::site) */
    float drop_p, inv_sqrt_c;
    uint64_t seed;
    const int32_t *edge_a, *edge_c, *edge_mol, *row_mol, *node_mol, *nn, *node_off, *edge_off;    /* HOST: [R] x 3, [Nn] x 2, [B], [B + 1] x 2 */
    int32_t* topo_dev;                             /* DEVICE scratch the entry uploads the topology into */
    size_t topo_dev_count;
    float* a[JODO_FT_N_SLOTS];                     /* DEVICE arrays */
    size_t n[JODO_FT_N_SLOTS];                     /* their element counts */
} jodo_fused_test_args;
int jodo_train_debug_fused(const jodo_fused_test_args* args, void* stream);

/* ---- optimiser side of the training step on flat buffers (csrc/train_step.hip; host mirror: jodo_amd/optim.py) ----------------------
 * jodo_adam_step  <- optimizer.step() of the optimisers get_optimizer builds, losses.py:14-26: torch.optim.AdamW(amsgrad=True,
 *   weight_decay=1e-12) (decoupled = 1) or torch.optim.Adam (decoupled = 0: L2 term added to the gradient), torch's single-tensor
 *   formulas, on n contiguous floats at once: every parameter of the module a slice of p, its gradient the same slice of g, m / v / vmax
 *   the moment buffers (vmax only with amsgrad).  step = 1 for the first update (bias corrections 1 - beta^step, formed in double).
 * jodo_gradnorm_clip  <- gradient_clipping, losses.py:29-50, with the history of recent gradient norms (Queue, :53-72) on the device:
 *   state_dev = double[52] (history[50], count, next slot; the caller writes {3000, 0, ..., count = 1, slot = 1} once, :77-78);
 *   norm_dev = the gradient's 2-norm; writes coef_dev = min(1, allowed / (norm + 1e-6)), allowed_dev = min(1.5 mean + 2 std, max_grad),
 *   and pushes min(norm, allowed) to the history.  No host synchronisation: the caller multiplies the flat gradient by *coef_dev. */
int jodo_adam_step(int64_t n, float* p, const float* g, float* m, float* v, float* vmax, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, int decoupled, int amsgrad, void* stream);
int jodo_gradnorm_clip(const float* norm_dev, double* state_dev, double max_grad, float* coef_dev, float* allowed_dev, void* stream);
/* jodo_kabsch_rotations  <- kabsch_batch, losses.py:424-434, behind the covariance einsum: A_dev [B, 3, 3] (A = P^T Q per molecule) ->
 *   R_dev [B, 3, 3] = U diag(1, 1, sign det A) V^T of A = U S V^T.  Replaces torch.linalg.svd + det + diag_embed + einsum, whose error
 *   check synchronises the host with the device (the last synchronisation of a training step). */
int jodo_kabsch_rotations(int B, const float* A_dev, float* R_dev, void* stream);

/* ---- the 2-D model: DGT_concat_2D (models/mol_gnn.py:797-946, blocks :325-407, TransMixLayer with ONE adjacency head) -------------
 * No positions, no batch-global operation.  Supported: nf 256, 16 heads of which 1 adjacency head (15 learned heads of 17 channels),
 * mlp_ratio 2, n_layers 8, time_dim 4 nf, in_node_dim <= 16, edge_ch in {2, 3}; anything else -> JODO_ERR_UNSUPPORTED.
 * The state_dict (235 tensors) is packed by name like the 3-D one (a leading "module." is accepted; a missing or mis-sized tensor is
 * JODO_ERR_ARG with its name in jodo_last_error()).  Slot tables below: offsets in floats into the packed blob.
 *   "tiled" weights: [out block of 32][K chunk of 64][8 quads][64 lanes][4] in MFMA A-operand order, see csrc/dgt2d_pack.cpp. */
typedef struct {
    int32_t nf, n_layers, n_heads, n_extra, mlp_ratio, in_node_dim, edge_ch;
    float edge_quan_th;
} jodo_cfg2d;
enum jodo2d_wslot_global {
    J2_TIME_FREQ = 0, J2_TIME_W1, J2_TIME_B1, J2_TIME_W3, J2_TIME_B3, J2_MOD_W, J2_MOD_B,
    J2_NODE_EMB_W, J2_NODE_EMB_B, J2_EDGE_EMB_W, J2_EDGE_EMB_B,
    J2_NH1_W, J2_NH1_B, J2_NH2_W, J2_NH2_B, J2_NH3_W, J2_NH3_B,
    J2_EH1_W, J2_EH1_B, J2_EH2_W, J2_EH2_B, J2_EH3_W, J2_EH3_B,
    J2_GLOBAL_COUNT
};
enum jodo2d_wslot_block {
    J2B_QKV_W = 0, J2B_QKV_B, J2B_LE_W, J2B_N2E_W, J2B_N2E_B, J2B_FF1_W, J2B_FF1_B, J2B_FF2_W, J2B_FF2_B,
    J2B_FF3_W, J2B_FF3_B, J2B_FF4_W, J2B_FF4_B, J2B_NRO_W, J2B_NRO_B, J2B_ERO_W, J2B_ERO_B,
    J2B_BLOCK_COUNT
};
/* JODO_OK, or JODO_ERR_UNSUPPORTED naming the setting outside the supported set */
int jodo_dgt2d_check_cfg(const jodo_cfg2d* cfg);
int jodo_dgt2d_packed_size(const jodo_cfg2d* cfg, size_t* n_floats, int* n_woff);
int jodo_dgt2d_pack_weights_host(const jodo_cfg2d* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                 size_t cap_floats, int64_t* woff_out, int n_woff);
/* Batch layout: B molecules with n_nodes[b] atoms (prefix masks, diagonal excluded), padded width N <= 64 of the dense tensors.
 * jodo_dgt2d_layout: sizes for the caller's buffers — out[0] = int32 words of the descriptor, out[1] = workspace bytes,
 * out[2] = real atoms Nn, out[3] = rows of the edge state (sum n^2), out[4] / out[5] = byte offsets of h [Nn, nf] and of the edge
 * state [rows, nf / 4] in the workspace (tests read them after a forward that stopped after `max_blocks` blocks; row of (b, r, c) =
 * eoff_b + r n_b + c, with only r < c rows live when the inputs were symmetric), out[6] = unordered pairs, out[7] = reserved.
 * jodo_dgt2d_fill_desc writes the descriptor into HOST memory; the caller copies it to the device. */
int jodo_dgt2d_layout(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, int64_t* out8);
int jodo_dgt2d_fill_desc(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, int32_t* desc_host, int64_t n_words);
/* One evaluation.  xh [B,N,nd], edge_x [B,N,N,ch], cond_x / cond_edge_x both given or both NULL (first step: all-ones adjacency
 * head), noise_level [B] -> out_xh [B,N,nd], out_edge [B,N,N,ch], written fully (zeros on padding and the diagonal).
 * flags_dev int32[8]: [0] = 1 when edge_x and cond_edge_x are symmetric (one pair-update / head evaluation per unordered pair),
 * 0 -> directed fallback; [1] = 1 when all noise levels are equal (one shared modulation row); [2] see jodo_dgt2d_forward_walk;
 * [3] = 1 when the split-bf16 form ran (jodo_dgt2d_forward_split), 0 from this entry and from jodo_dgt2d_forward_walk.
 * force_directed != 0: always the directed fallback (tests).  max_blocks < 0: all blocks. */
int jodo_dgt2d_forward(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev, const float* packed_w,
                       const int64_t* woff, int n_woff, const float* xh, const float* edge_x, const float* cond_x,
                       const float* cond_edge_x, const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev,
                       void* workspace, int force_directed, int max_blocks, void* stream);
/* Pair-symmetric attention walk (opt-in; csrc/dgt2d_forward.hip k2d_attn_pair): with symmetric inputs every unordered pair's edge
 * row is normalised and pushed through lin_edge0 / lin_edge1 + tanh once and serves both directions.  Both atoms of a pair sit in one
 * workgroup: the batch is cut into groups of whole molecules of up to 128 atom slots (largest molecule first, gaps filled with the
 * largest remaining molecule that fits; N <= 64, so every molecule fits).
 * jodo_dgt2d_pair_layout: out[0] = int32 words of the group descriptor, out[1] = groups, out[2] = work items, out[3] / out[4] = word
 * offsets of the item table and of the slot table, out[5] = slots per group (128), out[6] = words per item (4), out[7] = reserved.
 * jodo_dgt2d_pair_fill_desc writes it into HOST memory: items [items][4] = (group, first offset, last offset, 0), longest first (one
 * item per group with the offsets 1 .. max n / 2 of its molecules); slots [groups][128] = (molecule << 8) | atom, a molecule's atoms
 * in consecutive slots, -1 for an unused slot.  The walk: the atom i of a molecule of n atoms meets partner (i + d) mod n at every
 * offset d <= n / 2 of its item; at d = n / 2 of an even n both atoms of a pair meet it and each takes it as a target only. */
enum jodo2d_walk { JODO_2D_WALK_DIRECTED = 0, JODO_2D_WALK_PAIR = 1 };
int jodo_dgt2d_pair_layout(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, int64_t* out8);
int jodo_dgt2d_pair_fill_desc(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, int32_t* desc_host, int64_t n_words);
/* jodo_dgt2d_forward with a walk selector.  walk = JODO_2D_WALK_DIRECTED: exactly jodo_dgt2d_forward (pair_desc_dev is not read).
 * walk = JODO_2D_WALK_PAIR: pair_desc_dev is the device copy of the group descriptor; the choice is made on the device, without a
 * host synchronisation: with flags[0] == 1 k2d_attn_pair does the attention and the directed kernel leaves at once, with
 * flags[0] == 0 (asymmetric inputs, force_directed) it is the other way round.  The kernel that did the work records it in
 * flags_dev[2] (1 = pair walk, 0 = directed); jodo_dgt2d_forward never writes that slot. */
int jodo_dgt2d_forward_walk(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev,
                            const void* pair_desc_dev, int walk, const float* packed_w, const int64_t* woff, int n_woff, const float* xh,
                            const float* edge_x, const float* cond_x, const float* cond_edge_x, const float* noise_level, float* out_xh,
                            float* out_edge, int32_t* flags_dev, void* workspace, int force_directed, int max_blocks, void* stream);
/* Split-bf16 ("bf16x3") form of the 2-D model's node GEMMs and pair update (opt-in; csrc/dgt2d_forward.hip k2d_gemm_s, k2d_pair_s; the
 * arithmetic of csrc/dgt_split.h: w x = six bf16 x bf16 products of the hi / mid / lo terms, accumulated in fp32).  Attention, the
 * edge heads, the embeddings and the one-row time / modulation GEMMs stay exact fp32 and keep reading the fp32 blob, as do all biases.
 * The weight tape is a function of the packed blob: every covered tiled matrix [nb][nk][8 quads][64 lanes][4] floats becomes
 *   bf16 [nb][nk * 4 K16 steps][3 terms: hi, mid, lo][64 lanes][8],
 * element j of lane l in K16 step G of a chunk = the chunk's f32 k-step 8 G + j of the same lane, tile[(8 G + j) / 4][l][(8 G + j) % 4],
 * every term rounded to nearest even (hi + mid + lo is the float exactly).  Covered slots: per block J2B_QKV_W, J2B_N2E_W, J2B_FF1_W,
 * J2B_FF2_W, J2B_NRO_W, J2B_FF3_W, J2B_FF4_W, J2B_ERO_W; global J2_NH1_W, J2_NH2_W, J2_NH3_W.
 * jodo_dgt2d_split_size: *tape_bytes and toff_out[n_woff] = byte offset of every covered slot in the tape (16-byte aligned), indexed
 * like the woff table, -1 for the slots that are not covered.  n_woff must be the table size of jodo_dgt2d_packed_size.
 * jodo_dgt2d_pack_split_host: (packed HOST blob, its woff table) -> the tape in HOST memory; the caller uploads it. */
int jodo_dgt2d_split_size(const jodo_cfg2d* cfg, size_t* tape_bytes, int64_t* toff_out, int n_woff);
int jodo_dgt2d_pack_split_host(const jodo_cfg2d* cfg, const float* packed_host, const int64_t* woff, int n_woff, void* tape_host,
                               size_t cap_bytes);
/* jodo_dgt2d_forward_walk in the split form: tape_dev = device copy of the tape, toff = its HOST offset table.  walk as in
 * jodo_dgt2d_forward_walk (JODO_2D_WALK_DIRECTED: pair_desc_dev is not read).  Records flags_dev[3] = 1. */
int jodo_dgt2d_forward_split(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev,
                             const void* pair_desc_dev, int walk, const float* packed_w, const int64_t* woff, int n_woff,
                             const void* tape_dev, const int64_t* toff, const float* xh, const float* edge_x, const float* cond_x,
                             const float* cond_edge_x, const float* noise_level, float* out_xh, float* out_edge, int32_t* flags_dev,
                             void* workspace, int force_directed, int max_blocks, void* stream);
/* tests: the production row GEMM of the 2-D model on caller-packed device weights, y [rows, n_out] = epi(x [rows, K] W^T + bias),
 * act 1 = SiLU; K a multiple of 64, n_out of 32.  split = 0: w_dev is the f32 packing (k2d_gemm); 1: the split packing (k2d_gemm_s),
 * both as jodo_debug_pack_split emits them. */
int jodo_debug_gemm2d(int split, const float* x, int rows, int K, int n_out, const void* w_dev, const float* bias, int act, float* y,
                      void* stream);
/* Ancestral update of the 2-D sampler (sampling.py:637-658) for a node tensor WITHOUT position channels, replayed-draw form:
 * x_mean = cx x + cp pred, x_next = x_mean + sigma eps_node masked to the real atoms (all node channels are plain masked noise);
 * the edge tensors likewise with eps_edge [B,N,N,ch] read from its strict lower triangle for both orientations of a pair (the
 * triangle sample_symmetric_edge_feature_noise mirrors), masked to real pairs.  All outputs are written fully. */
int jodo_sampler_step_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float cx, float cp, float sigma,
                         const float* x, const float* edge_x, const float* pred, const float* edge_pred, const float* eps_node,
                         const float* eps_edge, float* x_next, float* edge_next, float* x_mean, float* edge_mean, void* stream);
/* The same update with BOTH draws generated in the kernel (Philox4x32-10 + Box-Muller keyed by `seed`, the generator and the element
 * numbering of jodo_sampler_step_rng, so that one restatement covers both): node channel k of atom a = b N + i is component k & 3 of
 * element a * 64 + (k >> 2) of the feature stream, masked to i < n_b (no position channels, no centre-of-mass step); edge channel f of
 * (b, r, c) is component f of cell (b N + max(r, c)) N + min(r, c) of the edge stream, zero on the diagonal and outside n_b — both
 * orientations evaluate the same counter.  Host-scalar form (coef_tab_dev = step_dev = NULL: coefficients by value, draw index `draw`)
 * or table form (row *step_dev of coef_tab_dev [steps][4] = (c_x, c_pred, sigma, noise_level), draw index `draw` + *step_dev: one
 * captured hipGraph of a step replays for every step, between jodo_step_begin and jodo_step_end).  node_feats <= 256, edge_ch <= 4.
 * One launch; all four outputs are written fully, padding included. */
int jodo_sampler_step_2d_rng(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float c_x, float c_pred, float sigma,
                             const float* coef_tab_dev, const int32_t* step_dev, uint64_t seed, uint32_t draw, const float* x,
                             const float* edge_x, const float* pred, const float* edge_pred, float* x_next, float* edge_next,
                             float* x_mean, float* edge_mean, void* stream);
/* jodo_dpm_update_2d  <- one update of DPM-Solver++ for the 2-D models (DPM_Solver_2D, jodo_amd/mix_dpm_solver.py): the position-free
 *                        counterpart of jodo_dpm_update.  Node tensor [B,N,nd] WITHOUT position channels and edge tensor [B,N,N,ch]
 *                        both take the data-prediction update of mix_dpm_solver.py:61-265
 *                            out = a * base - b * P - c * (c2 * (DA - DB))
 *                        (c = 0: first order; single-step second / third order, c < 0 for third; second-order multistep with
 *                        c2 = 1 / r0), products and sums rounded one by one in the order of the framework expression.  Nothing is
 *                        drawn.  Coefficients {a, b, c, c2, -, -, -, noise_level}: either 8 host floats, or the 8 columns from tab_col
 *                        of row *step_dev of a device table (row stride tab_stride floats) for captured hipGraphs; columns 4 - 6 are
 *                        not read and the noise level of the evaluation sits in column 7, where jodo_step_begin_at fetches it.
 *                        ONE launch: the edge output is computed once per unordered pair from cell (b, r, c) with r > c and stored
 *                        to both orientations — symmetric bit for bit, the upper triangle of the inputs is never read; the diagonal,
 *                        padded atoms and padded cells are written as exact zeros; every output element is written, by one thread.
 *                        Aliasing: x_out may be any of its node inputs and edge_out any of its edge inputs (in-place update): a
 *                        thread reads only elements it also writes.  Partial overlap is not allowed. */
int jodo_dpm_update_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, const float* coef8_host,
                       const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x_base,
                       const float* edge_base, const float* P, const float* eP, const float* DA, const float* eDA, const float* DB,
                       const float* eDB, float* x_out, float* edge_out, void* stream);
/* jodo_eps_to_data_2d  <- the conversion that lets DPM_Solver_2D run on a NOISE-predicting 2-D network (CDGS: pred_data = False,
 *                         self_cond = False): DPM-Solver++ updates data predictions, so each network output eps at time t becomes
 *                             d = (x - sigma_t * eps) / alpha_t
 *                         first — three correctly rounded fp32 operations in exactly that order (product, difference, quotient), no
 *                         contraction: the result equals the framework expression bit for bit.  Node tensors x / eps_x / d_x [B,N,nd]
 *                         WITHOUT position channels, edge tensors edge_x / eps_e / d_e [B,N,N,ch]; node_feats <= 256, edge_ch <= 4.
 *                         Coefficients: alpha and sigma by value (coef_tab_dev = step_dev = NULL), or columns tab_col + 5 and
 *                         tab_col + 6 of row *step_dev of a device table (row stride tab_stride floats) for captured hipGraphs.  A
 *                         noise-form table row is {a, b, c, c2, t, alpha_t, sigma_t, noise_level}: columns 0 - 3 and 7 are what
 *                         jodo_dpm_update_2d and jodo_step_begin_at read from a data-form row; 4 - 6, unused there, hold the time and
 *                         the marginal coefficients of the evaluation that the row's update follows.
 *                         Read: x, eps_x on real atoms; edge_x, eps_e on cells (b, r, c) with c < r < n_b — the diagonal, the upper
 *                         triangle and padding of the inputs are never read.  Written: every element of d_x and d_e, each by exactly
 *                         one thread with plain stores, in ONE launch: the edge value is computed once per unordered pair and stored to
 *                         both orientations (symmetric bit for bit); the diagonal, padded atoms and padded cells get exact zeros.
 *                         Aliasing: d_x may be x or eps_x, and d_e may be edge_x or eps_e (in-place conversion): a thread reads only
 *                         elements it also writes.  Partial overlap is not allowed.
 * jodo_step_begin_t    <- t_out[b] = table[*step][tab_col + 4] for b < B, and, when noise_level_out is not NULL,
 *                         noise_level_out[b] = table[*step][tab_col + 7]: the start of a captured evaluation of a network that reads
 *                         the time (CDGS).  jodo_step_begin_at stays the entry of the networks that read the noise level alone. */
int jodo_eps_to_data_2d(int B, int N, int node_feats, int edge_ch, const int32_t* n_nodes_dev, float alpha, float sigma,
                        const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, const float* x,
                        const float* edge_x, const float* eps_x, const float* eps_e, float* d_x, float* d_e, void* stream);
int jodo_step_begin_t(int B, const float* coef_tab_dev, const int32_t* step_dev, int tab_stride, int tab_col, float* t_out,
                      float* noise_level_out, void* stream);
/* jodo_prop_sample  <- the conditioning targets of a round, drawn on the device from the property prior (DistributionProperty,
 *                      jodo_amd/cond_gen/property_distribution.py; the reference's cond_gen/property_distribution.py draws them one
 *                      molecule and property at a time on the host): out[b, p] = one draw of property p for molecule b, normalised.
 *                      ONE launch, one thread per (molecule, property); no atomics, no LDS, no scratch.  A value depends only on
 *                      (seed, global index of the molecule, property column, the tables): not on B, the batch's composition or order.
 *   Tables (device): cum     uint32 [n_prop, n_slots, n_bins]  inclusive cumulative integer weights of the bins; the total T of a row
 *                                                              (its last entry) satisfies 0 < T < 2^31
 *                    minmax  f32    [n_prop, n_slots, 2]       (min, max) of the property at the slot's atom count
 *                    norm    f32    [n_prop, 2]                (mean, mad) of the property; (0, 1) = no normalisation
 *   Per molecule:    slot[b] in [0, n_slots): the table slot of its atom count (slots_host: the same B values on the host, checked
 *                    here before anything is launched; slots_dev: their device copy, which the kernel reads);
 *                    global index g = indices_dev[b] (device int64 [B]) when indices_dev is not NULL, else first_index + b.
 *   Draw:   w = philox4x32_10(counter (g lo, g hi, p, 3), key (seed lo, seed hi))   -- stream 3 beside the sampler's 0 / 1 / 2
 *           a = w[0] >> 8,  u2 = (w[1] >> 8) * 2^-24
 *           (words_dev not NULL, uint32 [B, n_prop, 2]: w[0], w[1] are read from it and Philox is skipped -- tests put a draw
 *           exactly on a bin boundary this way)
 *   Bin:    r = (uint64(a) * T) >> 24;  idx = the smallest bin with cum[idx] > r (binary search): a bin of weight 0 is never chosen,
 *           a = 0 gives the first bin of non-zero weight and a = 2^24 - 1 the last
 *   Value:  the reference's _idx2value with u2 for torch.rand, every fp32 operation rounded on its own (no contraction):
 *           left = fl32(idx / n_bins) * (max - min) + min;  right = fl32((idx + 1) / n_bins) * (max - min) + min
 *           val = u2 * (right - left) + left;  out = (val - mean) / mad   (a correctly rounded division)
 *   Errors, all before any launch: B < 1, n_prop < 1, n_bins < 1, n_slots < 1, a null table / slots / out pointer, a slot outside
 *           [0, n_slots) -> JODO_ERR_ARG; n_prop > 16 or n_bins > 65536 -> JODO_ERR_UNSUPPORTED. */
#define JODO_PROP_MAX_PROPS 16
#define JODO_PROP_MAX_BINS 65536
int jodo_prop_sample(int B, int n_prop, int n_bins, int n_slots, const uint32_t* cum_dev, const float* minmax_dev, const float* norm_dev,
                     const int32_t* slots_host, const int32_t* slots_dev, const int64_t* indices_dev, uint64_t first_index, uint64_t seed,
                     const uint32_t* words_dev, float* out, void* stream);
/* jodo_decode_2d  <- post_process_2D sampling.py:100-141 + the inverse scaler utils.py:71-105 for xh [B,N,atom_types(+1)] without
 *                    positions: the scaler in the framework's fp32 operation order (x * norm, then (x + 1) / 2 when centred, then the
 *                    mask), atom type [B,N] u8 = first maximum, formal charge [B,N] i8 = rintf (0 when include_fc = 0), bond type
 *                    [B,N,N] u8 by the rules of jodo_decode; zeros on padding and the diagonal. */
int jodo_decode_2d(int B, int N, int atom_types, int include_fc, int edge_ch, int compress_edge, int centered, float atom_norm,
                   float fc_norm, float edge_norm, const int32_t* n_nodes_dev, const float* xh, const float* edge_x,
                   uint8_t* atom_type_out, int8_t* fc_out, uint8_t* edge_type_out, void* stream);

/* ---- training step of the 2-D model (csrc/dgt2d_train.hip) ---------------------------------------------------------------------
 * jodo_train2d_* mirror jodo_train_* one for one (same conventions: parameters by name in PyTorch layouts, workspace kept by the
 * caller between forward and backward, gradients fully written — bytes in gaps under 16 bytes between two gradient buffers included —
 * in a fixed launch order without atomics) for DGT_concat_2D: the grad-enabled model call of get_sde_2D_loss_fn (losses.py:210-283)
 * and its loss.backward().  Dense directed n x n tiles per molecule like the 3-D engine (the reference draws the edge FFN's dropout per
 * directed edge).  xh [B,N,nd], edge_x [B,N,N,ch], cond_x / cond_edge_x both given or both NULL, noise_level [B]; `context` must be
 * NULL.  Dropout: the 3-D path's four sites and element numbering (site = 8 l + 1 .. 4, edge element = row of the dense tile).
 * jodo_train2d_set_option: 0 / 1 = fused forward / backward chains (csrc/train_fused.hip k2d_chain_a, k2d_bwd_a, chain B / B', node
 * LayerNorms): 0 (default: one launch per operation) / 1 (JODO_ERR_UNSUPPORTED for widths the chains are not built for);
 * 2 = 1 (default) / 0 the following forwards are (not) followed by a backward (the fused chains then skip backward-only stores).
 * jodo_train2d_debug_locate: selectors 0 .. 7 as jodo_train_debug_locate; 8 = xhat of the edges' LayerNorm1 [R, De], 9 = its rstd [R],
 * 10 = et [R, De], 11 = t0 = tanh(lin_edge0 et) [R, QK], 12 = t1 = tanh(lin_edge1 et) [R, D]. */
typedef struct jodo_train2d jodo_train2d;
int jodo_train2d_create(const jodo_cfg2d* cfg, int B, int N, const int32_t* n_nodes_host, const jodo_tensor* params, int n_params,
                        jodo_train2d** out);
void jodo_train2d_destroy(jodo_train2d* t);
size_t jodo_train2d_desc_bytes(const jodo_train2d* t);
size_t jodo_train2d_workspace_bytes(const jodo_train2d* t);
const void* jodo_train2d_desc_host(const jodo_train2d* t);
int jodo_train2d_upload(jodo_train2d* t, void* desc_dev, void* stream);
int jodo_train2d_set_option(jodo_train2d* t, int option, int value);
int jodo_train2d_debug_locate(const jodo_train2d* t, int what, int layer, size_t* byte_offset, size_t* count);
int jodo_train2d_forward(jodo_train2d* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* xh,
                         const float* edge_x, const float* cond_x, const float* cond_edge_x, const float* noise_level,
                         const float* context, float dropout_p, uint64_t seed, float* out_xh, float* out_edge, int32_t* flags_out,
                         void* workspace, void* stream);
int jodo_train2d_backward(jodo_train2d* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                          const float* noise_level, const float* d_out_xh, const float* d_out_edge, float dropout_p, uint64_t seed,
                          void* workspace, void* stream);

/* ---- property classifier: the masked EGNN of the conditional evaluation (cond_gen/model.py: EGNN / E_GCL_mask) ---------------------
 * One float per molecule from atom features h0 [B,N,in_node_nf] and positions x [B,N,3]; positions are never updated, the radial
 * |x_i - x_j|^2 is the same in every layer.  Stateless like the 2-D section: explicit stream, caller-owned memory.  Exact fp32 on
 * v_mfma_f32_32x32x2_f32 (csrc/egnn_forward.hip): real atoms compact at noff_b + i, prefix masks, no scatter, no atomics, the per-edge
 * message never reaches memory.  Supported: hidden_nf a multiple of 64 in [64, 256], n_layers 1..16, in_node_nf 1..16, attention and
 * node_attr 0 / 1, SiLU, no edge attributes, padded width N <= 255; anything else -> JODO_ERR_UNSUPPORTED naming the setting.
 * The state_dict (80 tensors at 7 layers with attention) is packed by name (a leading "module." is accepted; a missing or mis-sized
 * tensor is JODO_ERR_ARG with its name in jodo_last_error()).  Slot tables: offsets in floats into the packed blob; the table holds
 * JE_GLOBAL_COUNT global slots, then JEL_LAYER_COUNT per layer.  "Tiled" weights as in the 2-D section.
 *   JEL_P_W: edge_mlp.0 hoisted to the nodes, rows [W_src ; W_tgt] (2 nf x nf), JEL_P_B = [b1 ; 0]; JEL_WR = its radial column;
 *   JEL_N0_W: node_mlp.0 over [h | agg (| h0)], K = 2 nf (+ in_node_nf with node_attr, zero-padded to a K chunk).
 * These entry points are the inference side; fitting the classifier is the next section (jodo_egnn_train_*), whose forward runs the
 * same kernels on a blob it rebuilds on the device. */
typedef struct {
    int32_t hidden_nf, n_layers, in_node_nf, attention, node_attr;
} jodo_egnn_cfg;
enum jodo_egnn_wslot_global {
    JE_EMB_W = 0, JE_EMB_B, JE_ND0_W, JE_ND0_B, JE_ND2_W, JE_ND2_B, JE_GD0_W, JE_GD0_B, JE_GD2_W, JE_GD2_B,
    JE_GLOBAL_COUNT
};
enum jodo_egnn_wslot_layer {
    JEL_P_W = 0, JEL_P_B, JEL_WR, JEL_W2, JEL_B2, JEL_ATT_W, JEL_ATT_B, JEL_N0_W, JEL_N0_B, JEL_N2_W, JEL_N2_B,
    JEL_LAYER_COUNT
};
/* JODO_OK, or JODO_ERR_UNSUPPORTED naming the setting outside the supported set */
int jodo_egnn_check_cfg(const jodo_egnn_cfg* cfg);
int jodo_egnn_packed_size(const jodo_egnn_cfg* cfg, size_t* n_floats, int* n_woff);
int jodo_egnn_pack_weights_host(const jodo_egnn_cfg* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                size_t cap_floats, int64_t* woff_out, int n_woff);
/* jodo_egnn_layout: out[0] = int32 words of the descriptor, out[1] = workspace bytes, out[2] = real atoms Nn, out[3] = byte offset of
 * the hidden state h [Nn, hidden_nf] in the workspace (molecule b's atom i in row noff_b + i), out[4..7] = reserved (0).
 * jodo_egnn_fill_desc writes the descriptor into HOST memory: n_b [B], noff_b [B], then (b << 8) | i per real atom; the caller
 * copies it to the device. */
int jodo_egnn_layout(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes_host, int64_t* out8);
int jodo_egnn_fill_desc(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes_host, int32_t* desc_host, int64_t n_words);
/* One evaluation: out [B].  max_layers < 0: all layers and the readout.  max_layers >= 0 (tests): stops after that many layers, leaves
 * h in the workspace (out8[3] of jodo_egnn_layout) and does not write `out`. */
int jodo_egnn_forward(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev, const float* packed_w,
                      const int64_t* woff, int n_woff, const float* h0, const float* x, float* out, void* workspace, int max_layers,
                      void* stream);

/* ---- training the property classifier (csrc/egnn_train.hip) ----------------------------------------------------------------------------
 * jodo_egnn_train_* mirror jodo_train2d_* one for one: parameters by name in their PyTorch layouts at create (every tensor of the
 * state_dict; a leading "module." is accepted), params_dev / grads_dev pointer tables in that order, explicit stream, caller-owned
 * workspace that carries the kept tensors from forward to backward, gradients fully written (gaps under 16 bytes between two gradient
 * buffers included) in a fixed launch order without atomics.  The supported set is jodo_egnn_check_cfg's, N <= 255.
 * Forward: the kernels of jodo_egnn_forward in the same order, each layer's per-atom tensors kept (O(L Nn nf) floats, no per-edge
 * tensor); the tiled weight image is rebuilt on the device from params_dev on every call, so out [B] is bit-identical to
 * jodo_egnn_forward on the same weights and follows any in-place update of them.
 * Backward: d <d_out, out> / d parameter for d_out [B]; nothing with respect to h0 or x.  The message is recomputed per edge by the fused
 * kernel kegnn_edge_bwd, which writes 3 hidden_nf floats per edge (a, dz2, dz1: compact edge rows, reused by every layer).
 * jodo_egnn_train_set_option: option 2 only (accepted for parity with jodo_train2d_set_option; the forward keeps the same tensors either
 * way).  jodo_egnn_train_debug_locate: 0 = h_layer [Nn, nf] (layer 0 .. n_layers), 1 = P [Nn, 2 nf], 2 = agg [Nn, nf],
 * 3 = SiLU(node_mlp.0 .) [Nn, nf]. */
typedef struct jodo_egnn_train jodo_egnn_train;
int jodo_egnn_train_create(const jodo_egnn_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const jodo_tensor* params, int n_params,
                           jodo_egnn_train** out);
void jodo_egnn_train_destroy(jodo_egnn_train* t);
size_t jodo_egnn_train_desc_bytes(const jodo_egnn_train* t);
size_t jodo_egnn_train_workspace_bytes(const jodo_egnn_train* t);
const void* jodo_egnn_train_desc_host(const jodo_egnn_train* t);
int jodo_egnn_train_upload(jodo_egnn_train* t, void* desc_dev, void* stream);
int jodo_egnn_train_set_option(jodo_egnn_train* t, int option, int value);
int jodo_egnn_train_debug_locate(const jodo_egnn_train* t, int what, int layer, size_t* byte_offset, size_t* count);
int jodo_egnn_train_forward(jodo_egnn_train* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* h0,
                            const float* x, float* out, void* workspace, void* stream);
int jodo_egnn_train_backward(jodo_egnn_train* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                             const float* d_out, void* workspace, void* stream);

/* tests: ONE fused edge kernel of the classifier on caller-owned device arrays (csrc/egnn_train.hip; tests/test_egnn_kernels_gpu.py
 * compares every array the kernel stores with a float64 restatement).  The entry adds no kernel: it builds the descriptor tables as
 * jodo_egnn_train_create does, makes the two tiled images of W2 with kegnn_pack (kinds 0 and 1), and calls the host launcher that
 * jegnn::run / the training backward call, through the same switch over hidden_nf / 32.
 *   op JODO_ET_OP_FWD: kegnn_edge                       reads P, XC, WR, W2, B2 (WA, BA); writes AGG [Nn, nf]
 *   op JODO_ET_OP_BWD: kegnn_edge_bwd, kegnn_tgt_sum    reads the same and DAGG [Nn, nf]; writes EA, EZ2, EZ1 [E, nf] (compact edge rows
 *                      e = eoff_b + i (n - 1) + (j < i ? j : j - 1)), DP [Nn, 2 nf] (both halves), Q [Nn, 2 nf], QB [Nn]
 * P [Nn, 2 nf] = P_src + b1 | P_tgt, XC [Nn, 4], WR [nf], W2 [nf, nf] in the PyTorch layout, B2 [nf], WA [nf] and BA [1] (both NULL:
 * no attention), Nn = sum n, E = sum n (n - 1).  Scratch: DESC (3 B + Nn floats' worth of int32), IMG (2 nf^2: the two images).
 * grid_cap: 0 = the production cap of the persistent grid, otherwise at most that many workgroups.
 * Nothing is launched unless every check holds: nf in {64, 128, 192, 256} and 1 <= n <= 255 for every molecule (n > 255:
 * JODO_ERR_UNSUPPORTED; n < 1: JODO_ERR_ARG), a HIP device (JODO_ERR_UNSUPPORTED); every slot the op uses non-NULL (unless it has no
 * element: E = 0 is legal), 16-byte aligned (BA: 4) and with exactly the op's element count in n[.], scratch slots at least theirs
 * (JODO_ERR_ARG).  Slots an op does not use are ignored. */
enum { JODO_ET_OP_FWD = 0, JODO_ET_OP_BWD, JODO_ET_N_OPS };
enum { JODO_ET_P = 0, JODO_ET_XC, JODO_ET_DAGG, JODO_ET_WR, JODO_ET_W2, JODO_ET_B2, JODO_ET_WA, JODO_ET_BA, JODO_ET_DESC, JODO_ET_IMG,
       JODO_ET_AGG, JODO_ET_EA, JODO_ET_EZ2, JODO_ET_EZ1, JODO_ET_DP, JODO_ET_Q, JODO_ET_QB, JODO_ET_N_SLOTS };
typedef struct {
    int32_t op, nf, B, grid_cap;
    const int32_t* n_nodes;                        /* HOST [B] */
    float* a[JODO_ET_N_SLOTS];                     /* DEVICE arrays */
    size_t n[JODO_ET_N_SLOTS];                     /* their element counts */
} jodo_egnn_edge_test_args;
int jodo_egnn_debug_edge(const jodo_egnn_edge_test_args* args, void* stream);

/* ---- evaluation: atom and molecule stability of decoded molecules (csrc/eval_kernels.hip; evaluation/stability.py:17-161 of the
 * reference: check_stability, and check_2D_stability for molecules without aromatic bonds) ----
 * Inputs are the decode's device tensors (jodo_decode): pos f32 [B,N,3], atom_type u8 [B,N], fc i8 [B,N], edge_type u8 [B,N,N],
 * n_nodes i32 [B].  Atoms at index >= n_nodes[b] do not exist, whatever the padding holds; a molecule with n_nodes <= 0 gets a zero row
 * and counts in no total.  N <= 256, T <= 255 (JODO_ERR_UNSUPPORTED beyond).  The rule tables are the caller's DATA:
 *   thr_dev        i32 [T][T][3]: single / double / triple thresholds of the ORDERED type pair in integer picometres, margins included,
 *                  0 = no such bond; not symmetric.  pair_order says which ordered pair is looked up for atoms i < j:
 *                  JODO_PAIR_BY_INDEX (type[i], type[j]), JODO_PAIR_BY_TYPE (the smaller type index first).
 *                  Order of a pair at d = sqrtf(dx^2 + dy^2 + dz^2): 0 unless 100 d < t1; then 1 unless t2 > 0 and 100 d < t2; then 2
 *                  unless t3 > 0 and 100 d < t3; then 3.
 *   allowed_dev    u32 [T]: bit v set = valence v is allowed for the type (valence >= 32: unstable)
 *   allowed_fc_dev u32 [T][fc_hi - fc_lo + 1]: the same per (type, formal charge), fc_lo <= 0 <= fc_hi; a charge outside the range reads
 *                  the column of charge 0
 * jodo_stability_3d: valence = integer sum of the pair orders.  order_out (optional, may be NULL): u8 [B,N,N] pair orders, symmetric,
 *   zero on the diagonal and outside the molecule.
 * jodo_stability_bonds: valence of atom i = sum over j of edge_type[min(i,j)][max(i,j)] (the upper triangle only is read) for orders 1-3;
 *   an entry above 3 (4 = aromatic) is counted once in the molecule's needs_kekulize column and enters no valence.
 * per_mol_out  i32 [B][4]: stable atoms, atoms, fragments, needs_kekulize (always 0 for the 3-D rule).  Fragments = connected components
 *   over the bonds of order > 0 (derived orders / edge_type entries), an isolated atom being one.
 * totals_out   i64 [4]: stable molecules, stable atoms, atoms, connected molecules (one fragment); zeroed by the call, then reduced
 *   with integer atomics.  No host synchronisation; both calls may be captured into a graph. */
enum jodo_pair_order { JODO_PAIR_BY_INDEX = 0, JODO_PAIR_BY_TYPE = 1 };
int jodo_stability_3d(int B, int N, int T, int pair_order, const int32_t* thr_dev, const uint32_t* allowed_dev, const int32_t* n_nodes_dev,
                      const float* pos, const uint8_t* atom_type, int32_t* per_mol_out, uint8_t* order_out, int64_t* totals_out,
                      void* stream);
int jodo_stability_bonds(int B, int N, int T, int fc_lo, int fc_hi, const uint32_t* allowed_fc_dev, const int32_t* n_nodes_dev,
                         const uint8_t* atom_type, const int8_t* fc, const uint8_t* edge_type, int32_t* per_mol_out, int64_t* totals_out,
                         void* stream);

/* ---- evaluation: sub-structure geometry and its MMD (csrc/geometry_kernels.hip; evaluation/cal_geometry.py and evaluation/mmd.py of the
 * reference) ----
 * Extraction.  Inputs are the decode's device tensors as above (pos, atom_type, edge_type, n_nodes); keep (optional, may be NULL) u8 [B]:
 * 0 = the molecule contributes nothing.  The molecule is the one check_2D_stability builds: a bond (i < j) for every nonzero
 * edge_type[i][j] of the upper triangle, in row-major order; bond code 1, 2, 3, or 12 for edge_type 4.  Classes are integer tuples
 * (atom-type index, code, atom-type index per bond): cls_b i32 [Cb][3], cls_a i32 [Ca][6], cls_d i32 [Cd][9], at most
 * JODO_GEOMETRY_MAX_CLASSES per group; whole tuples are compared, the forward tuple first, then the reversed one.  Enumeration and
 * multiplicities are cal_bond_distance / cal_bond_angle / cal_dihedral_angle's.  Values are float32: length in Angstrom,
 * angle in degrees [0, 180], dihedral in degrees, signed; a non-finite value is dropped and counted.  N <= 256 (JODO_ERR_UNSUPPORTED).
 * jodo_geometry_count: counts_out i32 [Cb+Ca+Cd][B] values per (class, molecule); offsets_out i64 [Cb+Ca+Cd][B] their exclusive scan
 *   per group (class-major, molecule-minor: where a molecule's values of a class start in the group's array); sizes_out i64 [Cb+Ca+Cd]
 *   values per class; dropped_out i64 [3] non-finite values per group.
 * jodo_geometry_write: the same inputs and the offsets; out_b / out_a / out_d f32 of n_b / n_a / n_d values (the sums of sizes_out per
 *   group; a pointer may be NULL when its size is 0).  The order inside a molecule is the reference's, the whole output is a function of
 *   the input alone.  No host synchronisation in either call. */
#define JODO_GEOMETRY_MAX_CLASSES 32
int jodo_geometry_count(int B, int N, int Cb, int Ca, int Cd, const int32_t* cls_b_dev, const int32_t* cls_a_dev, const int32_t* cls_d_dev,
                        const int32_t* n_nodes_dev, const uint8_t* keep, const float* pos, const uint8_t* atom_type,
                        const uint8_t* edge_type, int32_t* counts_out, int64_t* offsets_out, int64_t* sizes_out, int64_t* dropped_out,
                        void* stream);
int jodo_geometry_write(int B, int N, int Cb, int Ca, int Cd, const int32_t* cls_b_dev, const int32_t* cls_a_dev, const int32_t* cls_d_dev,
                        const int32_t* n_nodes_dev, const uint8_t* keep, const float* pos, const uint8_t* atom_type,
                        const uint8_t* edge_type, const int64_t* offsets, float* out_b, float* out_a, float* out_d, int64_t n_b, int64_t n_a,
                        int64_t n_d, void* stream);

/* compute_mmd(source, target, kernel_mul, kernel_num, fix_sigma) of the reference for S segments in three launches.
 * seg_dev i64 [S][4]: source offset, n_s, target offset, n_t (offsets into src / tgt, f32).  tiles_dev i32 [T][4]: segment, kind
 * (0 source x source, 1 target x target, 2 source x target), x0, y0 — every JODO_MMD_TILE x JODO_MMD_TILE tile of kind 2, and of kinds
 * 0 / 1 the tiles with y0 >= x0 (x0, y0 multiples of JODO_MMD_TILE; a tile above the diagonal is doubled), the tiles of a segment
 * contiguous; tile_start_dev i32 [S+1] their ranges.  params_ws f32 [S][12], partials_ws f64 [T].  out_dev f64 [S]:
 * XX / n_s^2 + YY / n_t^2 - 2 XY / (n_s n_t), diagonals included; NaN for an empty side or a zero bandwidth, as in the reference.
 * fix_sigma 0 = the bandwidth of the data.  kernel_num 1 .. 8.  Bit-identical from run to run (no float atomics). */
#define JODO_MMD_TILE 1024
int jodo_mmd_batched(int S, int T, const int64_t* seg_dev, const int32_t* tiles_dev, const int32_t* tile_start_dev, const float* src,
                     const float* tgt, double kernel_mul, int kernel_num, double fix_sigma, float* params_ws, double* partials_ws,
                     double* out_dev, void* stream);

const char* jodo_last_error(void);

/* measurement helper (synchronises, default stream): fp32 MFMA throughput of the box in TFLOP/s from a
 * register-only kernel; chains = 8 independent accumulator chains per wave (pipe ceiling) or 1 dependent chain
 * (what one projection block is); waves_per_simd x 1024 waves are launched.  sink_dev: any device float. */
int jodo_debug_mfma_peak(int iters, int chains, int waves_per_simd, float* sink_dev, float* tflops_out);

/* same, one dependent chain per wave (waves_per_simd x 1024 waves) with nv independent v_fma (and nt transcendentals)
 * issued after every MFMA: tells whether vector work hides under the matrix pipe.  (nv, nt) in
 * {(0,0),(4,0),(8,0),(12,0),(16,0),(4,1),(4,2)}. */
int jodo_debug_mfma_valu(int iters, int nv, int nt, int waves_per_simd, float* sink_dev, float* tflops_out);

/* ---- opt-in split-bf16 pair update (JODO_OPT_SPLIT_BF16; no reference counterpart: an alternative arithmetic form of
 * MultiCondEquiUpdate + the edge FFN, models/mol_gnn.py:71-94, :313-317) ----
 * jodo_dgt_split_size: bytes of the static weight tapes for this configuration — all of them, one block's PAIR tape (edge FFN, readout,
 *   triangular factor of the rotated statistics: k_edge_update_sym_split), one block's NODE tape (node2edge, node FFN, rotated W_row /
 *   W_col, readout, the next block's q / k / v: k_node_post_split; 0 when the width-generic node kernels run, jodo_cfg.layout = 1), one
 *   block's ATTENTION tapes (two cyclic tapes, one per launch of k_edge_attn variants 4 / 5: edge_emb, that launch's blocks of lin_edge0 and
 *   lin_edge1; 0 outside the tuned nf 256 set);
 *   JODO_ERR_UNSUPPORTED unless nf is 256 or 384 and cond_ch = 0.  Layout of the buffer: L pair tapes, then L node tapes, then L attention tapes.
 * jodo_dgt_pack_split_host: the tapes (hi | mid | lo bf16 terms of every weight, in consumption order) from the same named fp32 tensors
 *   jodo_dgt_pack_weights takes, into a host buffer.
 * jodo_plan_set_split_weights: device copy of that tape for this plan (caller-owned, must outlive the plan's forwards; NULL clears). */
int jodo_dgt_split_size(const jodo_cfg* cfg, size_t* total_bytes, size_t* pair_block_bytes, size_t* node_block_bytes, size_t* attn_block_bytes);
int jodo_dgt_pack_split_host(const jodo_cfg* cfg, const jodo_tensor* tensors, int n_tensors, void* host, size_t cap_bytes);
int jodo_plan_set_split_weights(jodo_plan* plan, const void* tape_dev, size_t bytes);
/* The CONDITIONAL model's tape (cond_ch > 0, nf 256; k_edge_update_sym_split_cond, csrc/dgt_kernels_split_cond.h): a pair tape only — per
 *   block the edge FFN and the readout as above, then input_lin's [e ; G] columns (8 output blocks x 8 K16 steps) and coord_mlp.0
 *   (8 x 16): every weight of the un-folded pair update is static, so nothing comes from the workspace.  228 steps of 3 KiB per block at
 *   mlp_ratio 2, 260 at 4; layout of the buffer: L pair tapes.  JODO_ERR_UNSUPPORTED unless nf = 256 and cond_ch > 0 (jodo_dgt_split_size /
 *   jodo_dgt_pack_split_host keep refusing conditional configurations).  jodo_plan_set_split_weights takes this tape for a conditional plan. */
int jodo_dgt_split_cond_size(const jodo_cfg* cfg, size_t* total_bytes, size_t* pair_block_bytes);
int jodo_dgt_pack_split_cond_host(const jodo_cfg* cfg, const jodo_tensor* tensors, int n_tensors, void* host, size_t cap_bytes);

/* ---- gate experiments of the opt-in split-bf16 (three-term, fp32-equivalent) MFMA form (csrc/dgt_split.{h,hip}; no reference
 * counterpart; measurement helpers, never on the data path) ----
 * jodo_debug_mfma_bf16_valu: `chains` (1 | 2) dependent v_mfma_f32_32x32x16_bf16 chains per wave with nv in {0,2,4,6,8,16} (one chain)
 *   or {0,4,8,16} (two chains) independent v_fma issued behind every MFMA; returns the matrix TFLOP/s (bf16 flops).
 * jodo_debug_pack_split: a row-major [n_out, n_in] matrix -> its f32 packing and its split packing (hi / mid / lo bf16 terms), host.
 * jodo_debug_chain: y [rows, 256] = W x for x [rows, K], K in {128, 256}, in the strip model with streamed weights; mode 0 exact fp32
 *   MFMA, 1 split form (one accumulator), 2 split form (corrections in their own accumulator); tiles = item tiles per wave (2: split
 *   modes, K = 128).  iters > 1 repeats the projection in registers (timing; y then holds a digest); ms_out != NULL times the launch
 *   with HIP events (synchronises). */
int jodo_debug_mfma_bf16_valu(int iters, int nv, int chains, int waves_per_simd, float* sink_dev, float* tflops_out);
int jodo_debug_pack_split(const float* W, int n_out, int n_in, float* f32_packed_host, void* split_packed_host);
int jodo_debug_chain(int mode, int K, int tiles, const float* x, int rows, const float* wf, const void* wsp, float* y, int iters,
                     float* ms_out, void* stream);

int jodo_debug_mlp(const float* x, int rows, const float* w1, const float* b1, const float* w2,
                   const float* b2, float* y, void* stream);

/* ---- CDGS: the 2-D graph noise-prediction network (reference models/cdgs.py; csrc/cdgs_forward.hip, csrc/cdgs_pack.cpp) ----
 * Inference only, exact fp32 (fp32 MFMA for every projection), no float atomics: two calls on the same inputs give the same bits.
 * Supported: nf 256, n_heads 16, 1 <= n_layers <= 16, atom_ch 1..16, edge_ch 2 | 3, rw_depth 1..16, padded width N <= 181
 * (JODO_CDGS_MAX_N); anything else -> JODO_ERR_UNSUPPORTED naming the setting.
 * Weights: the reference's state_dict by name (`all_modules.<i>...`; 4-D [out, in, 1, 1] conv weights accepted as matrices), plus one
 * caller-made tensor "time_freq" [nf / 2] (the sinusoid's frequencies, which the reference computes per call).  Slot tables: offsets in
 * floats into the packed blob; the table holds JCG_GLOBAL_COUNT + n_layers * JCB_BLOCK_COUNT entries.
 * Widths: cat = 2 nf / n_layers readout channels per block, stored at a stride of catp = cat rounded up to 32.  The node head reads rows
 * [hids (n_layers catp) | atom_cate (154)] and the edge heads [hids | dense_cate (77, at +0) | dense_exist (77, at +96)], each padded to a
 * multiple of 64; the packer permutes and zero-pads the first head layers' columns accordingly.
 * Layout: real atoms compact (row noff_b + i); the edge state keeps n_b^2 rows of nf floats per molecule, row eoff_b + r n_b + c, the
 * diagonal rows included (they are zero between blocks and carry FF(2 h_i) inside the edge GroupNorm statistics).
 * jodo_cdgs_layout: out[0] = int32 words of the descriptor, out[1] = workspace bytes, out[2] = Nn, out[3] = R = sum n_b^2, byte offsets
 * into the workspace of out[4] = h [Nn, nf], out[5] = e [R, nf], out[6] = the distance codes (int32 [R]), out[7] = the landing
 * probabilities (float [Nn, 16], the first rw_depth live).  The workspace is the caller's.  What it may hold: any FINITE float32
 * values (zero-fill it once).  Outputs do not depend on them (every forward writes the zero row of its [h ; 0] GEMM itself); NaN / Inf
 * are not allowed because the head inputs are padded to a multiple of 64 columns (the edge head's also between dense_cate and
 * dense_exist, columns 77 .. 95) that no kernel writes and that meet zero weight columns.
 * jodo_cdgs_fill_desc writes the descriptor into HOST memory: n_b [B], noff_b [B], eoff_b [B], b per real atom [Nn], b per edge row [R].
 * jodo_cdgs_forward: t [B], x [B, N, atom_ch], edge_x [B, N, N, edge_ch] -> out_x [B, N, atom_ch], out_e [B, N, N, edge_ch], masked.
 * max_blocks in [0, n_layers]: stop after that many blocks (0: after the embeddings) with h and e in the workspace; the outputs are then
 * not written. */
#define JODO_CDGS_MAX_N 181
typedef struct {
    int32_t nf, n_layers, n_heads, atom_ch, edge_ch, rw_depth;
} jodo_cdgs_cfg;
enum jodo_cdgs_wslot_global {
    JCG_FREQ, JCG_T1_W, JCG_T1_B, JCG_T2_W, JCG_T2_B, JCG_TMOD_W, JCG_TMOD_B, JCG_EC_W, JCG_EC_B, JCG_EX_W, JCG_EX_B, JCG_SPD_W, JCG_SPD_B,
    JCG_EEMB_W, JCG_EEMB_B, JCG_AD_W, JCG_AD_B, JCG_AC_W, JCG_AC_B, JCG_AR_W, JCG_AR_B, JCG_NEMB_W, JCG_NEMB_B, JCG_AH1_W, JCG_AH1_B,
    JCG_AH2_W, JCG_AH2_B, JCG_AH3_W, JCG_AH3_B, JCG_EH1_W, JCG_EH1_B, JCG_EH2_W, JCG_EH2_B, JCG_EH3_W, JCG_EH3_B, JCG_GLOBAL_COUNT
};
enum jodo_cdgs_wslot_block {
    JCB_EPS, JCB_GIN1_W, JCB_GIN1_B, JCB_GIN2_W, JCB_GIN2_B, JCB_QKV_W, JCB_QKV_B, JCB_E01_W, JCB_NL_G, JCB_NL_B, JCB_NA_G, JCB_NA_B,
    JCB_FF1_W, JCB_FF1_B, JCB_FF2_W, JCB_FF2_B, JCB_NN_G, JCB_NN_B, JCB_FF3_W, JCB_FF3_B, JCB_FF4_W, JCB_FF4_B, JCB_NE_G, JCB_NE_B,
    JCB_RN_W, JCB_RN_B, JCB_RE_W, JCB_RE_B, JCB_BLOCK_COUNT
};
int jodo_cdgs_check_cfg(const jodo_cdgs_cfg* cfg);
int jodo_cdgs_packed_size(const jodo_cdgs_cfg* cfg, size_t* n_floats, int* n_woff);
int jodo_cdgs_pack_weights_host(const jodo_cdgs_cfg* cfg, const jodo_tensor* tensors, int n_tensors, float* packed_host,
                                size_t capacity_floats, int64_t* woff, int n_woff);
int jodo_cdgs_layout(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, int64_t* out8);
int jodo_cdgs_fill_desc(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, int32_t* desc_host, int64_t n_words);
int jodo_cdgs_forward(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev, const float* packed_w,
                      const int64_t* woff, int n_woff, const float* t, const float* x, const float* edge_x, float* out_x, float* out_e,
                      void* workspace, int max_blocks, void* stream);
/* Split-bf16 ("bf16x3") form of CDGS — OPT-IN, never the default path.  Every row GEMM over node rows or edge rows runs on the bf16 MFMA
 * with three-term operands (kernel kc_gemm_s; the arithmetic of csrc/dgt_split.h, as in the 2-D model's form above): the embeddings
 * JCG_NEMB_W, JCG_EEMB_W; per block JCB_GIN1_W, JCB_GIN2_W, JCB_QKV_W, JCB_E01_W, JCB_FF1_W .. JCB_FF4_W, JCB_RN_W, JCB_RE_W; the heads
 * JCG_AH1_W .. JCG_AH3_W, JCG_EH1_W .. JCG_EH3_W.  The three GEMMs over the B time-embedding rows (T1, T2, TMOD) stay exact fp32, so the
 * time shifts are the same bits in both forms; GINE, attention, the GroupNorms, the random-walk features, the embedding inputs and the
 * outputs are unchanged, as are all biases (read from the fp32 blob).
 * The tape is a function of the packed blob with the semantics of jodo_dgt2d_split_size / jodo_dgt2d_pack_split_host: every covered tiled
 * matrix [nb][nk][8 quads][64 lanes][4] floats becomes bf16 [nb][nk * 4 K16 steps][3 terms: hi, mid, lo][64 lanes][8], every term rounded
 * to nearest even.  jodo_cdgs_split_size: *tape_bytes and toff_out[n_woff] = byte offset of every covered slot (16-byte aligned), indexed
 * like the woff table, -1 for the slots that are not covered; n_woff must be the table size of jodo_cdgs_packed_size.
 * jodo_cdgs_pack_split_host: (packed HOST blob, its woff table) -> the tape in HOST memory; the caller uploads it.
 * jodo_cdgs_forward_split: jodo_cdgs_forward plus tape_dev (device copy of the tape), toff (its HOST offset table) and flags_dev (4 int32
 * on the device): same launch sequence, max_blocks honoured; its first launch writes flags_dev[0..3] = {0, 0, 0, 1} ([3]: the split form
 * ran, the word the 2-D model uses).  Every covered slot must have an aligned place in toff, else JODO_ERR_ARG. */
int jodo_cdgs_split_size(const jodo_cdgs_cfg* cfg, size_t* tape_bytes, int64_t* toff_out, int n_woff);
int jodo_cdgs_pack_split_host(const jodo_cdgs_cfg* cfg, const float* packed_host, const int64_t* woff, int n_woff, void* tape_host,
                              size_t cap_bytes);
int jodo_cdgs_forward_split(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev, const float* packed_w,
                            const int64_t* woff, int n_woff, const float* t, const float* x, const float* edge_x, float* out_x,
                            float* out_e, void* workspace, int max_blocks, void* stream, const void* tape_dev, const int64_t* toff,
                            int32_t* flags_dev);
/* tests: the production row GEMM of CDGS on caller-packed device weights, y [rows, n_out] (stride ldy) = residual + act(x' W^T + bias);
 * x' by mode: 0 row of x [rows, K] (stride ldx); 1 that row plus row (molecule of the edge row) of xadd (stride ldadd); 2 x[atom r] +
 * x[atom c] of the edge row, x [Nn, K].  act 0 none, 1 SiLU, 2 ReLU, 3 tanh; residual (stride ldy) may be y or NULL; bias may be NULL.
 * K a multiple of 64, n_out of 32, else JODO_ERR_ARG (null x / w_dev / y likewise).  Modes 1 and 2 read desc_dev, the descriptor of
 * (cfg, B, N, n_nodes_host), and rows must equal its edge-row count; mode 0 ignores them.  split = 0: w_dev is the f32 packing
 * (kc_gemm); 1: the split packing (kc_gemm_s with the forward's dispatch), both as jodo_debug_pack_split emits them. */
int jodo_debug_gemm_cdgs(int split, int mode, const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const void* desc_dev,
                         const float* x, int ldx, int rows, int K, int n_out, const void* w_dev, const float* bias, int act,
                         const float* xadd, int ldadd, const float* residual, float* y, int ldy, void* stream);

/* ---- CDGS training (csrc/cdgs_train.hip): forward with kept activations + the gradient of every parameter ----
 * jodo_cdgs_train_* mirror jodo_train2d_* one for one: tensors by name in their PyTorch layouts at create (every tensor of the
 * state_dict, the GINE `local_model.eps` buffers included; a leading "module." is accepted), params_dev / grads_dev pointer tables in
 * that order, explicit stream, caller-owned workspace that carries the kept tensors from forward to backward, gradients fully written
 * (gaps under 16 bytes between two gradient buffers included) in a fixed launch order without atomics: two backward calls on the same
 * activations give the same bits.  The eps buffers are inputs: their value is used, their grads_dev entry must be NULL.
 * Layout: the reference's dense padded tensors, node row b N + i, edge row (b N + r) N + c, padded and diagonal rows included; the
 * edge feed-forward, its residual and norm2_edge run over all B N^2 rows, for every dropout probability.  Any N; B N^2 <= 2^30.
 * Dropout (train_common.h drop_mul): site = 8 l + {1 h_local, 2 h_attn, 3 node FF hidden, 4 node FF out, 5 edge FF hidden, 6 edge FF
 * out}, element = flat index of the reference's own dense tensor.  Supported: nf a multiple of 32 with GroupNorm groups of 8 channels
 * (nf 256), n_heads dividing nf, 1 <= n_layers <= 16, edge_ch >= 2.
 * Inputs: time_freq [nf / 2] (the sinusoid's frequencies, caller-made as for jodo_cdgs_pack_weights_host), t [B], x [B, N, atom_ch],
 * edge_x [B, N, N, edge_ch]; the backward reads x and edge_x again (embedding weight gradients).  No input gradients.
 * jodo_cdgs_train_set_option: option 2 (0 / 1, accepted for parity; the forward keeps the same tensors either way) and option 3 =
 * the product forms that run in split-bf16 (csrc/train_gemm.hip k_gemm_s: three bf16 terms per fp32 operand, six bf16 MFMAs per K = 16
 * step, fp32 accumulation, same plan and slice order as the fp32 product, bit-reproducible), a bit mask: 1 forward products (every
 * Linear / 1x1 convolution, the tanh and SiLU x dropout epilogues included), 2 data gradients, 4 weight gradients with their bias
 * sums; 0 = every product in exact fp32, the default.  The mask covers EVERY product of the step, the time MLP's and the per-block
 * time shifts over the B rows included; GINE, attention, the GroupNorms, the random-walk features and all reductions stay fp32 code.
 * The forward and the backward read the mask when they run.  Values outside 0..7: JODO_ERR_ARG; a non-zero mask on the host build of
 * the file (no matrix instructions: exact fp32 only): JODO_ERR_UNSUPPORTED.  jodo_cdgs_train_get_option reads an option back (2: 1).
 * jodo_cdgs_train_debug_locate: 0 = h after `layer` blocks [B N, nf], 1 = e after `layer` blocks [B N^2, nf], 2 = alpha of block
 * `layer` [B N^2, n_heads], 3 = xhat of its norm2_edge [B N^2, nf]. */
typedef struct jodo_cdgs_train jodo_cdgs_train;
int jodo_cdgs_train_create(const jodo_cdgs_cfg* cfg, int B, int N, const int32_t* n_nodes_host, const jodo_tensor* params, int n_params,
                           jodo_cdgs_train** out);
void jodo_cdgs_train_destroy(jodo_cdgs_train* t);
size_t jodo_cdgs_train_desc_bytes(const jodo_cdgs_train* t);
size_t jodo_cdgs_train_workspace_bytes(const jodo_cdgs_train* t);
const void* jodo_cdgs_train_desc_host(const jodo_cdgs_train* t);
int jodo_cdgs_train_upload(jodo_cdgs_train* t, void* desc_dev, void* stream);
int jodo_cdgs_train_set_option(jodo_cdgs_train* t, int option, int value);
int jodo_cdgs_train_get_option(const jodo_cdgs_train* t, int option, int* value);
int jodo_cdgs_train_debug_locate(const jodo_cdgs_train* t, int what, int layer, size_t* byte_offset, size_t* count);
/* tests: out[rows, F] = the dropout multipliers of rows row0 .. row0 + rows - 1 of a [., F] tensor at `site`, element row * F + f */
int jodo_cdgs_train_debug_drop(float dropout_p, uint64_t seed, int site, int64_t row0, int rows, int F, float* out, void* stream);
int jodo_cdgs_train_forward(jodo_cdgs_train* t, const void* desc_dev, const float* const* params_dev, int n_params, const float* time_freq,
                            const float* t_in, const float* x, const float* edge_x, float dropout_p, uint64_t seed, float* out_x, float* out_e,
                            void* workspace, void* stream);
int jodo_cdgs_train_backward(jodo_cdgs_train* t, const void* desc_dev, const float* const* params_dev, float* const* grads_dev, int n_params,
                             const float* x, const float* edge_x, const float* d_out_x, const float* d_out_e, float dropout_p, uint64_t seed,
                             void* workspace, void* stream);

/* tests: ONE launch sequence (or one single launch) of the CDGS training step on caller-owned device arrays (csrc/cdgs_train.hip;
 * tests/test_cdgs_kernels_gpu.py compares every array an op stores with a float64 restatement).  The entry adds no kernel and no copy of
 * a launch sequence: every multi-launch op is the host function that jodo_cdgs_train_forward / _backward call on the workspace.
 * Geometry: n_nodes [B] in HOST memory, uploaded by the entry into nn_dev (device, nn_dev_count >= B int32); M = B N node rows (b N + i),
 * R = B N^2 tile rows ((b N + r) N + c), G = D / 8 GroupNorm groups.  `rows` = 0: every row of the op's tensor (M in mode 1, R in
 * modes 0 and 2); otherwise the op runs on the first `rows` rows of it (SCALE, RELU, RELU_BWD, NORM_GRADS only; 1 <= rows <= that count).
 * op                  kernels                                            reads                          writes
 * RW                  kc_adj, kc_adnorm, kc_rw_step x K, kc_onehot,      EDGE_X [R, ch]                 ADJ, AD, CNT [R], ONEHOT [R, K + 1],
 *                     kc_deg                                                                            LAND [M, K], DEG [M, ch]; PA, PB [R] scratch
 * ADDT                kc_addt (mode 1 | 2)                               X [rows, F], TB [B, F]         Y [rows, F]
 * SCALE               kc_scale (mode 0 | 1 | 2, acc, dropout)            X [rows, F] (acc: and Y)       Y [rows, F]
 * RELU / RELU_BWD     kc_relu / kc_relu_bwd                              X [rows, F]                    Y [rows, F] (RELU_BWD: in place on Y)
 * PAIR / PAIR_BWD     kc_pair / kc_pair_bwd                              X [M, D] / X [R, D]            Y [R, D] / Y [M, D]
 * OUT_NODES           kc_out_nodes                                       X [M, F]                       Y [M, F]
 * OUT_EDGES           kc_out_edges                                       X [R, ch]                      Y [R, ch]
 * SUMS                kc_sum_cols, kc_sum_nodes (mode = masked 0 | 1)    X [R, F]                       Y [M, F], Z [B, F]
 * GINE                kc_gine                                            EPS [1], HS [M, D], HE [R, D], ADJ [R]    AGG [M, D]
 * GINE_BWD            kc_gine_bwd_e, kc_gine_bwd_n                       the same and DAGG [M, D]       DHE [R, D], DHS [M, D]
 * GN_FWD              kc_gn_fwd (amask, acc, dropout)                    H, A [M, D], GAMMA, BETA [D] (acc: and Y)   XHAT [M, D], RSTD [M, G], Y [M, D]
 * GN_BWD              kc_gn_bwd (acc)                                    DY, XHAT [M, D], RSTD [M, G], GAMMA [D] (acc: and DX)   DX [M, D]
 * EGN_FWD             kc_egn_part mode 0, kc_egn_fin, kc_egn_apply       XHAT [R, D] (x, turned into xhat IN PLACE), GAMMA, BETA [D]   XHAT, RSTD [B, G], Y [R, D]
 * EGN_BWD             kc_egn_part mode 2 with gamma, kc_egn_fin,         DY [R, D], XHAT [R, D], RSTD [B, G], GAMMA [D]   DX [R, D]
 *                     kc_egn_bwd
 * NORM_GRADS          kc_colsum_part, _mid, _fin (mode 1 | 2)            DY, XHAT [rows, F]             DBETA, DGAMMA [F]
 * ATTN_FWD            kc_attn_logit, kc_attn_softmax, kc_attn_msg        Q, K, V [M, D], G0, G1 [R, D]  ALPHA [R, H] (logits, then alpha in place), ATT [M, D]
 * ATTN_BWD            the seven kc_attn_bwd_* kernels                    DATT [M, D], Q, K, V, G0, G1, ALPHA [R, H]   DV, DQ, DK [M, D], DAL [R, H] (d alpha,
 *                                                                                                       then d logit in place), DT1, DT0 [R, D]
 * Double scratch (sizes in floats, the engine's own rule): PART >= 4 M G (EGN_*) or 4 (nchunk + nchunk / 32 + 1) F with
 * nchunk = ceil(rows / 64) (NORM_GRADS); GSUM >= 4 B G (EGN_*).  isc multiplies the logits (the step passes 1 / sqrt(D / H)).
 * Nothing is launched unless every check holds: a known op, B, N >= 1, B N^2 <= 2^30, every n_nodes[b] in 1 .. N, D % 8 == 0, H
 * dividing D, F, K >= 1, ch >= 2, D, F <= 4096 and K, ch <= 256 (JODO_ERR_UNSUPPORTED for the sizes, JODO_ERR_ARG for the rest), mode / acc /
 * amask / rows in the op's range, 0 <= drop_p < 1, and every slot the op touches non-NULL, 16-byte aligned and with exactly the op's
 * element count in n[.] (scratch slots and nn_dev: at least theirs) (JODO_ERR_ARG).  Slots an op does not use are ignored. */
enum { JODO_CT_OP_RW = 0, JODO_CT_OP_ADDT, JODO_CT_OP_SCALE, JODO_CT_OP_RELU, JODO_CT_OP_RELU_BWD, JODO_CT_OP_PAIR, JODO_CT_OP_PAIR_BWD,
       JODO_CT_OP_OUT_NODES, JODO_CT_OP_OUT_EDGES, JODO_CT_OP_SUMS, JODO_CT_OP_GINE, JODO_CT_OP_GINE_BWD, JODO_CT_OP_GN_FWD, JODO_CT_OP_GN_BWD,
       JODO_CT_OP_EGN_FWD, JODO_CT_OP_EGN_BWD, JODO_CT_OP_NORM_GRADS, JODO_CT_OP_ATTN_FWD, JODO_CT_OP_ATTN_BWD, JODO_CT_N_OPS };
enum { JODO_CT_EDGE_X = 0, JODO_CT_ADJ, JODO_CT_AD, JODO_CT_PA, JODO_CT_PB, JODO_CT_CNT, JODO_CT_ONEHOT, JODO_CT_LAND, JODO_CT_DEG, JODO_CT_X,
       JODO_CT_TB, JODO_CT_Y, JODO_CT_Z, JODO_CT_EPS, JODO_CT_HS, JODO_CT_HE, JODO_CT_AGG, JODO_CT_DAGG, JODO_CT_DHE, JODO_CT_DHS, JODO_CT_H,
       JODO_CT_A, JODO_CT_GAMMA, JODO_CT_BETA, JODO_CT_XHAT, JODO_CT_RSTD, JODO_CT_DY, JODO_CT_DX, JODO_CT_PART, JODO_CT_GSUM, JODO_CT_DBETA,
       JODO_CT_DGAMMA, JODO_CT_Q, JODO_CT_K, JODO_CT_V, JODO_CT_G0, JODO_CT_G1, JODO_CT_ALPHA, JODO_CT_ATT, JODO_CT_DATT, JODO_CT_DV,
       JODO_CT_DAL, JODO_CT_DT1, JODO_CT_DT0, JODO_CT_DQ, JODO_CT_DK, JODO_CT_N_SLOTS };
typedef struct {
    int32_t op, B, N, D, H, F, K, ch, mode, acc, amask, drop_site;
    float isc, drop_p;
    uint64_t drop_seed;
    int64_t rows;
    const int32_t* n_nodes;                        /* HOST [B] */
    int32_t* nn_dev;                               /* DEVICE scratch: the entry uploads n_nodes here */
    size_t nn_dev_count;                           /* its int32 count, >= B */
    float* a[JODO_CT_N_SLOTS];                     /* DEVICE arrays */
    size_t n[JODO_CT_N_SLOTS];                     /* their element counts (floats) */
} jodo_cdgs_op_test_args;
int jodo_cdgs_train_debug_op(const jodo_cdgs_op_test_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
